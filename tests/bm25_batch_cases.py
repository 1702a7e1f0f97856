"""Cases of the batched BM25 search, shared by ``tests/test_gpu_bm25_batch.py`` (runs them on the device) and
``tests/test_bm25_batch_host.py`` (shows on the CPU, with the oracle alone, that each meets the condition it was built for).

A plain module: no fixtures, no import of the product.  Corpora and query strings are those of ``oracle/text_cases.py``;
postings come from the library's own ``build_postings``, which the callers pass in.  Expected values are
``oracle.bm25.search_postings`` per question and, with an allow-set,
``select_topk(where(allowed, merged_scores(...), 0), k)``; they are computed once per (case, k, merge) and shared.
"""
from __future__ import annotations

import itertools
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import bm25 as ob
from oracle import text_cases as tc

Question = Tuple[Any, ...]                      # strings, or (term ids, idfs) pairs for hand-made postings


def bits(ranked):
    return [(int(d), np.float64(s).view(np.uint64)) for d, s in ranked]


def case_named(name: str) -> tc.Bm25Case:
    return next(c for c in tc.BM25_CASES if c.name == name)


def case_postings(name: str, build_postings: Callable) -> Dict[str, Any]:
    """Postings of a corpus of ``oracle/text_cases.py``, by the name of a case that uses it (built once per session and
    shared with ``tests/test_gpu_text_channel.py``)."""
    return tc.bm25_postings(case_named(name), build_postings)


ZIPF_CASE, KINDS_CASE, SAME_CASE = "many-queries", "stride-b-rare-term", "stride-a-one-tie-group"

_POSTINGS: Dict[Any, Dict[str, Any]] = {}


def postings_of(key, rows_fn: Callable[[], Any], build_postings: Callable, k1: float = 1.5, b: float = 0.75) -> Dict[str, Any]:
    """``build_postings(rows_fn(), k1, b)`` of a corpus of this module, built once per ``(key, k1, b)``."""
    full = (key, k1, b)
    if full not in _POSTINGS:
        _POSTINGS[full] = build_postings(rows_fn(), k1, b)
    return _POSTINGS[full]


_EXPECTED: Dict[Any, List[List[Tuple[int, float]]]] = {}


def expected(tag, p: Dict[str, Any], questions: Sequence[Question], k: int, merge: str, k1: float = 1.5,
             allowed: Optional[np.ndarray] = None) -> List[List[Tuple[int, float]]]:
    """One oracle ranking per question; ``tag`` (hashable, names the postings, the questions and the mask) keys the cache."""
    key = (tag, k, merge, k1)
    if key not in _EXPECTED:
        out = []
        for qs in questions:
            if allowed is None:
                out.append(ob.search_postings(p, list(qs), k, merge, k1))
            else:
                out.append(ob.select_topk(np.where(allowed, ob.merged_scores(p, list(qs), merge, k1), 0.0), k))
        _EXPECTED[key] = out
    return _EXPECTED[key]


def cut(strings: Sequence[Any], sizes: Sequence[int]) -> List[Question]:
    """``strings`` cut into questions of ``sizes`` queries in rotation until they run out (the last one takes what is left)."""
    out, at = [], 0
    for n in itertools.cycle(sizes):
        if at >= len(strings):
            break
        out.append(tuple(strings[at:at + n]))
        at += n
    return out


# ------------------------------------------------------------------------------------------------ 1 grouping
GROUP_K = 200
ROTATION = (0, 1, 2, 3, 5)


def grouping_singles() -> List[Question]:
    return [(s,) for s in tc.many_queries()]


def grouping_rotation() -> List[Question]:
    return cut(tc.many_queries(), ROTATION)


# ------------------------------------------------------------------------------------------------ 2 position independence
PROBE: Question = ("w3 w17 w3 w1200", "w5 w9 w29", "nosuchterm w2")
POSITION_N = 300


def position_batch(where: int) -> List[Question]:
    """300 questions of 0-3 queries with ``PROBE`` at index ``where``."""
    fill = cut(tc.many_queries()[:600], (2, 3, 1, 0, 2))[:POSITION_N - 1]
    assert len(fill) == POSITION_N - 1
    return fill[:where] + [PROBE] + fill[where:]


def other_size_batch() -> List[Question]:
    return cut(tc.many_queries()[600:640], (5, 1, 3))


# ------------------------------------------------------------------------------------------------ 3 chunk boundary
CHUNK_ROWS = 3                                   # score rows the scratch limit of this case admits per chunk
CHUNK_SIZES = (1, 3, 1, 4, 0, 2, 2, 1, 3, 0, 1)  # queries per question: 11 questions, 18 rows
SMALL_SETTINGS = (("default", 1.5, 0.75), ("k1-0", 0.0, 0.75), ("b-0", 1.5, 0.0), ("b-1", 1.5, 1.0))


def chunk_questions() -> List[Question]:
    strings = [s for qs in tc._SMALL_QUERIES for s in qs]
    pool = list(itertools.islice(itertools.cycle(strings), sum(CHUNK_SIZES)))
    out, at = [], 0
    for n in CHUNK_SIZES:
        out.append(tuple(pool[at:at + n]))
        at += n
    return out


def chunk_limit(n_docs: int) -> int:
    return CHUNK_ROWS * n_docs * 8


def chunks_of(sizes: Sequence[int], rows_cap: int) -> List[List[int]]:
    """The chunking rule of the batch search: questions in order, whole, while their rows fit ``rows_cap``;
    a question without queries needs no row.  -> question indexes per chunk (questions with a query only)."""
    out: List[List[int]] = []
    rows = 0
    for g, n in enumerate(sizes):
        if n == 0:
            continue
        if not out or rows + n > rows_cap:
            out.append([])
            rows = 0
        out[-1].append(g)
        rows += n
    return out


# ------------------------------------------------------------------------------------------------ 4 above the selection grid
KINDS_QUESTIONS: Tuple[Question, ...] = (("rare",), ("alpha beta",), ("alpha beta beta", "rare"))
KINDS_KS = (1500, 4096)
SAME_QUESTIONS: Tuple[Question, ...] = (("alpha beta beta",), ("alpha beta beta",))
SAME_KS = (1, 4096)

# ------------------------------------------------------------------------------------------------ 5 through the C ABI
LOW_QUERY = ([0], [0.7])
LOW_QUESTIONS: Tuple[Question, ...] = ((LOW_QUERY,), (LOW_QUERY,), (LOW_QUERY,))
LOW_KS = (10, 257)
NEG_QUESTIONS: Tuple[Question, ...] = tuple(tuple(qs) for qs in tc._NEG)
NEG_KS = (50, 600)

# ------------------------------------------------------------------------------------------------ 6 allow-set
ALLOW_N_QUESTIONS = 64
ALLOW_K = 200
ALLOW_FEW = (31, 32, 63, 64, 19_999)
SAME_CUT_N = 1000                               # 31 * 32 + 8: a partial last word
SAME_CUT_K = 100


def allow_questions() -> List[Question]:
    """64 questions of 1-3 queries of at least 3 known-looking tokens each, from the pool of ``many_queries``."""
    strings = [s for s in tc.many_queries() if len(s.split()) >= 3 and "unknown" not in s]
    return cut(strings, (1, 2, 3))[:ALLOW_N_QUESTIONS]


def same_cut_rows():
    return tc.rows_same()[:SAME_CUT_N]


def allow_masks(p: Dict[str, Any], build_top1: Callable[[], List[int]]) -> Dict[str, np.ndarray]:
    """name -> bool mask over the documents.  ``build_top1``: the unfiltered top-1 document of the first 8 questions."""
    n = p["N"]
    third = np.zeros(n, dtype=bool)
    third[::3] = True
    few = np.zeros(n, dtype=bool)
    few[list(ALLOW_FEW)] = True
    no_top1 = np.ones(n, dtype=bool)
    no_top1[build_top1()] = False
    return {"all": np.ones(n, dtype=bool), "none": np.zeros(n, dtype=bool), "third": third, "few": few, "no-top1": no_top1}


def unfiltered_top1(p: Dict[str, Any], questions: Sequence[Question]) -> List[int]:
    want = expected("allow-unfiltered", p, questions, ALLOW_K, "max")
    return [want[g][0][0] for g in range(8)]


# ------------------------------------------------------------------------------------------------ 8 searcher
def searcher_rows():
    return tc.rows_zipf(60, 5, 40)


SEARCHER_QUESTIONS: Tuple[Question, ...] = (("w0 w3",), ("w1", "w2 w2 w7"), (), ("nosuchterm",), ("w5 w1 w0", "", "w9"))
