"""Cases for the text channel (BM25), the fusion kernel and the fp64 cosine kernels.

TEST INFRASTRUCTURE (see ``oracle/__init__.py``).  ``tests/test_gpu_text_channel.py`` runs these inputs on the device;
``tests/test_text_channel_host.py`` shows on the CPU, with the oracle alone, that every case meets the condition it was
built for and that the mutants it targets change what the GPU test compares.  Everything is seeded or constructed; there
are no fixtures.

BM25 cases come as rows of text (built by the library's own ``build_postings``, which the callers pass in: this package
never imports the product) or as hand-made CSR postings that go through the C ABI.  Expected results are
``oracle.bm25.search_postings``.

Cosine inputs are multiples of 2**-20 below 4 in magnitude, so dot products and squared norms are exact in int64 and the
reference value is the exact quotient, evaluated in 50-digit decimal arithmetic.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from decimal import Decimal, localcontext
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import bm25 as ob

GRID = ob.SELECT_GRID             # 262 144: documents one sweep of the device's selection grid covers
BM25_MAX_QUERIES = 1024
FUSE_MAX = 4096


# ------------------------------------------------------------------------------------------------ BM25 corpora
def _row(i: int, text: str) -> Dict[str, Any]:
    return {"doc_id": f"T{i // 5}#{i % 5}", "title": f"T{i // 5}", "sent_id": i % 5, "text": text}


STRIDE_N = 300_000
RARE_DOCS = tuple(1000 + 8111 * i for i in range(37))        # 33 below 262 144, 4 at or above it
KIND_A_EVERY = 300                                           # 1000 documents of the better kind, over the whole range


@functools.lru_cache(maxsize=None)
def rows_same() -> List[Dict[str, Any]]:
    """stride (a): one text everywhere -- one tie group of 300 000, the order is decided by the document alone."""
    return [_row(i, "alpha beta beta") for i in range(STRIDE_N)]


@functools.lru_cache(maxsize=None)
def rows_kinds() -> List[Dict[str, Any]]:
    """stride (b), (c): 1000 documents "alpha beta beta" spread evenly, 37 with a rare term, the rest "alpha beta gamma"."""
    rare = set(RARE_DOCS)
    return [_row(i, "alpha beta gamma rare" if i in rare else ("alpha beta beta" if i % KIND_A_EVERY == 7 else "alpha beta gamma"))
            for i in range(STRIDE_N)]


@functools.lru_cache(maxsize=None)
def rows_zipf(n: int, seed: int, vocab: int = 3000) -> List[Dict[str, Any]]:
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocab + 1) ** 1.1
    p /= p.sum()
    lens = rng.integers(3, 25, size=n)
    words = rng.choice(vocab, size=int(lens.sum()), p=p)
    rows, at = [], 0
    for i, ln in enumerate(lens):
        rows.append(_row(i, " ".join(f"w{w}" for w in words[at:at + ln])))
        at += ln
    return rows


@functools.lru_cache(maxsize=None)
def rows_small(n: int) -> List[Dict[str, Any]]:
    rng = np.random.default_rng(100 + n)
    return [_row(i, " ".join(f"w{w}" for w in rng.integers(0, 6, size=int(rng.integers(1, 7))))) for i in range(n)]


def _handmade(indptr, post_doc, post_tf, doc_norm) -> Dict[str, Any]:
    return {"indptr": np.asarray(indptr, dtype=np.int64), "post_doc": np.ascontiguousarray(post_doc, dtype=np.int32),
            "post_tf": np.ascontiguousarray(post_tf, dtype=np.int32), "doc_norm": np.ascontiguousarray(doc_norm, dtype=np.float64),
            "N": len(doc_norm)}


LOW_N = 70_000


@functools.lru_cache(maxsize=None)
def postings_low_bytes(best_last: bool) -> Dict[str, Any]:
    """One term in 70 000 documents, tf = 1, doc_norm 2**-44 apart: scores that differ only below their top 5 bytes.
    ``best_last`` reverses the norms, so that the best scores sit at the HIGHEST documents: with the norms rising, a
    selection that ignored the low score bytes would fall back on the document order and still be right."""
    d = np.arange(LOW_N, dtype=np.float64)
    norm = 1.5 + (d[::-1] if best_last else d) * 2.0 ** -44
    return _handmade([0, LOW_N], np.arange(LOW_N), np.ones(LOW_N), norm)


@functools.lru_cache(maxsize=None)
def postings_negative_idf() -> Dict[str, Any]:
    """600 documents, three terms; the callers weight term 1 negatively, which only a hand-made query can do."""
    n = 600
    t0, t1, t2 = np.arange(n), np.arange(0, n, 2), np.arange(0, n, 3)
    tf = np.concatenate([1 + t0 % 3, 1 + t1 % 2, np.ones(len(t2), dtype=np.int64)])
    return _handmade([0, len(t0), len(t0) + len(t1), len(t0) + len(t1) + len(t2)], np.concatenate([t0, t1, t2]), tf,
                     1.5 * (0.25 + 0.75 * (1 + np.arange(n) % 7) / 4.0))


@functools.lru_cache(maxsize=None)
def many_queries(n_queries: int = BM25_MAX_QUERIES, seed: int = 11) -> Tuple[str, ...]:
    """0-12 tokens each, drawn from a pool of at most 5 words per query (repeats), unknown terms, empty queries."""
    rng = np.random.default_rng(seed)
    out = []
    for q in range(n_queries):
        ln = 0 if q % 97 == 5 else int(rng.integers(0, 13))
        pool = [f"w{int(w)}" for w in rng.integers(0, 3000, size=3)] + [f"w{int(w)}" for w in rng.integers(0, 30, size=2)]
        toks = [pool[int(i)] for i in rng.integers(0, 5, size=ln)]
        if q % 9 == 0 and toks:
            toks[int(rng.integers(0, len(toks)))] = f"unknown{q}"
        out.append(" ".join(toks))
    return tuple(out)


@dataclass(frozen=True)
class Bm25Case:
    name: str
    corpus: Callable[[], Any]                 # rows (via == "text") or hand-made postings (via == "abi")
    query_sets: Tuple[Any, ...]               # each: a tuple of strings, or of (term ids, idfs) pairs
    ks: Tuple[int, ...]
    merges: Tuple[str, ...] = ("max",)
    targets: Tuple[str, ...] = ()
    k1: float = 1.5
    b: float = 0.75
    via: str = "text"
    top_k: Optional[int] = None               # what the caller passes instead of k (small cases: 10**9, k = N)

    def runs(self):
        for qs in self.query_sets:
            for merge in self.merges:
                for k in self.ks:
                    yield list(qs), k, merge


_SMALL_QUERIES = (("w1 w2",), ("w0", "w3 w3 w1"), ("w5 w5 w5 w0 w4",), ("nosuchterm zz",), ("", ""), ("w1", ""), ("w2 nosuchterm w2",))


def _small_cases():
    out = []
    for n in (1, 2, 257):
        for tag, k1, b in (("default", 1.5, 0.75), ("k1-0", 0.0, 0.75), ("b-0", 1.5, 0.0), ("b-1", 1.5, 1.0)):
            out.append(Bm25Case(f"small-{n}-{tag}", functools.partial(rows_small, n), _SMALL_QUERIES, (n,), ("max", "sum"),
                                (), k1, b, "text", 10 ** 9))
    return out


_NEG = (((([0], [0.5]), ([1], [-2.0]))), (([0, 1, 2], [0.5, -2.0, 0.25]),), (([2, 1], [3.0, -0.75]), ([0, 0], [0.125, 0.125])))

BM25_CASES: Tuple[Bm25Case, ...] = (
    Bm25Case("stride-a-one-tie-group", rows_same, (("alpha beta beta",),), (1, 100, 4096), ("max",), ("ties_doc_desc", "skip_255")),
    Bm25Case("stride-b-rare-term", rows_kinds, (("rare",),), (4096,), ("max",), ("first_stride_only",)),
    Bm25Case("stride-c-cut-in-second-group", rows_kinds, (("alpha beta",),), (1500, 4096), ("max", "sum"),
             ("first_stride_only", "ties_doc_desc")),
    Bm25Case("low-bytes", functools.partial(postings_low_bytes, False), ((([0], [0.7]),),), (10, 257), ("max",), ("skip_255",), via="abi"),
    Bm25Case("low-bytes-best-last", functools.partial(postings_low_bytes, True), ((([0], [0.7]),),), (10, 257), ("max",),
             ("score_top5_bytes",), via="abi"),
    Bm25Case("many-queries", functools.partial(rows_zipf, 20_000, 21), (many_queries(),), (200,), ("sum", "max"),
             ("drop_repeats", "tokens_reversed", "sum_is_max", "skip_255")),
    Bm25Case("negative-idf", postings_negative_idf, _NEG, (50, 600), ("sum", "max"), ("cut_before_filter",), via="abi"),
) + tuple(_small_cases())

# the host file's bit-for-bit comparison with Bm25Oracle: a corpus the dict-based oracle still searches in a second
ZIPF_SMALL = (5000, 3)
ZIPF_SMALL_QUERIES = (("w0 w3 w77 w2999",), ("w1 w2", "w9 w9 w1500 w9", "w2998 w17 w2 nosuchterm"), ("w5 w600", "", "w5 w7 w5"),
                      ("", ""), ("nosuchterm",))


def bm25_postings(case: Bm25Case, build_postings: Optional[Callable] = None, _cache: Dict = {}) -> Dict[str, Any]:
    """The case's CSR postings: hand-made, or ``build_postings(rows, k1, b)`` (the library's builder, passed in)."""
    if case.via == "abi":
        return case.corpus()
    key = (case.corpus.func, case.corpus.args, case.k1, case.b) if isinstance(case.corpus, functools.partial) else (case.corpus, case.k1, case.b)
    if key not in _cache:
        _cache[key] = build_postings(case.corpus(), case.k1, case.b)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ fusion
def _hit(i: int, doc: int, sid: int, score: float) -> Dict[str, Any]:
    return {"id": f"x{i}", "score": float(score), "meta": {"doc": f"T{doc}", "sent_id": sid, "text": f"s{i}", "m%d" % (i % 3): i}}


def _nid(doc: int, sid: int) -> str:
    return f"sent::T{doc}::{sid}"


def _channel(rng, n: int, docs: int, draw: Callable[[], float], first: int = 0) -> List[Dict[str, Any]]:
    return [_hit(first + i, int(rng.integers(0, docs)), int(rng.integers(1, 4)), draw()) for i in range(n)]


def _dense(rng, n: int, docs: int, draw: Callable[[], float]) -> Dict[str, float]:
    out: Dict[str, float] = {}
    while len(out) < n:
        out.setdefault(_nid(int(rng.integers(0, docs)), int(rng.integers(1, 4))), draw())
    return out


@dataclass(frozen=True)
class FusionCase:
    name: str
    make: Callable[[], Tuple[List[Dict[str, Any]], List[Dict[str, Any]], Dict[str, float]]]
    alphas: Tuple[float, float, float] = (0.4, 0.2, 0.4)
    top_ks: Tuple[int, ...] = (1, 7, 10 ** 9)
    wants: Tuple[str, ...] = ()               # conditions the host file asserts: see tests/test_text_channel_host.py


@functools.lru_cache(maxsize=None)
def fusion_3000():
    rng = np.random.default_rng(31)
    text = _channel(rng, 1400, 100, lambda: float(np.round(rng.normal(5.0, 2.0), 1)))
    graph = _channel(rng, 400, 40, lambda: float(np.round(rng.normal(-3.0, 2.0), 1)), 5000)
    dense = _dense(rng, 1200, 700, lambda: float(np.round(rng.uniform(-1, 1), 3)))
    return text, graph, dense


@functools.lru_cache(maxsize=None)
def fusion_ties():
    rng = np.random.default_rng(32)
    dy = lambda: float(rng.integers(0, 5)) / 4.0                                  # 0, 1/4 .. 1: min-max leaves them as they are
    return _channel(rng, 600, 60, dy), _channel(rng, 500, 70, dy, 5000), _dense(rng, 400, 200, dy)


def _fusion_sized(n_dense: int):
    rng = np.random.default_rng(33)
    text = _channel(rng, 2000, 200, lambda: float(np.round(rng.normal(0.0, 3.0), 2)))
    graph = _channel(rng, 1000, 100, lambda: float(np.round(rng.normal(1.0, 1.0), 2)), 5000)
    return text, graph, _dense(rng, n_dense, 1500, lambda: float(rng.uniform(-1, 1)))


@functools.lru_cache(maxsize=None)
def fusion_4096():
    return _fusion_sized(FUSE_MAX - 3000)


@functools.lru_cache(maxsize=None)
def fusion_4097():
    return _fusion_sized(FUSE_MAX - 3000 + 1)


@functools.lru_cache(maxsize=None)
def fusion_flat_empty_negative():
    """text: every score equal; graph: empty; dense: negative scores only."""
    rng = np.random.default_rng(34)
    return _channel(rng, 1100, 200, lambda: 2.5), [], _dense(rng, 300, 400, lambda: -float(np.round(rng.uniform(0.1, 9), 2)))


@functools.lru_cache(maxsize=None)
def fusion_negative_flat_empty():
    """text: negative scores only, with duplicates; graph: every score equal; dense: empty."""
    rng = np.random.default_rng(35)
    return (_channel(rng, 800, 150, lambda: -float(np.round(rng.uniform(0.1, 9), 1))), _channel(rng, 400, 150, lambda: -1.0, 5000), {})


FUSION_CASES: Tuple[FusionCase, ...] = (
    FusionCase("3000-entries", fusion_3000, wants=("n>1024", "duplicates", "one-two-three")),
    FusionCase("exact-ties", fusion_ties, (0.5, 0.25, 0.25), (50, 10 ** 9), ("n>1024", "duplicates", "one-two-three", "ties")),
    FusionCase("exactly-4096", fusion_4096, top_ks=(7, 10 ** 9), wants=("n==4096", "duplicates")),
    FusionCase("flat-empty-negative", fusion_flat_empty_negative, top_ks=(7, 10 ** 9), wants=("n>1024",)),
    FusionCase("negative-flat-empty", fusion_negative_flat_empty, top_ks=(7, 10 ** 9), wants=("n>1024",)),
)


def fusion_entries(case_inputs) -> int:
    text, graph, dense = case_inputs
    return len(text) + len(graph) + len(dense)


# ------------------------------------------------------------------------------------------------ cosine
U = 2.0 ** -53
_Q = 20                                         # inputs are multiples of 2**-_Q


def cosine_bound(dim: int) -> float:
    """|computed - exact| for a cosine of ``dim`` fp64 products summed in any order: dim*u on the dot product, dim*u/2 on
    each norm, and the roundings of the two square roots, the product, the division and the reference's conversion
    (8u covers them); u = 2**-53.  Derived, not measured."""
    return (2 * dim + 8) * U


COSINE_F64_N = (1, 2, 3, 5, 201, 1023)
COSINE_F64_DIM = (1, 7, 63, 64, 65, 100, 768)
COSINE_MATRIX_N = (1, 2, 3, 5, 7, 45)
COSINE_MATRIX_DIM = (7, 64, 65)
COSINE_ADJ_N = (0, 1, 2, 5, 6, 258)
COSINE_ADJ_DIM = (7, 64, 65)


def cosine_vectors(n: int, dim: int, seed: int, zero_rows: Sequence[int] = ()) -> np.ndarray:
    """[n, dim] fp64, every entry a multiple of 2**-20 with 0.25 <= |x| < 4 (no zeros: dropping an element always matters)."""
    rng = np.random.default_rng((seed, n, dim))
    x = np.rint((0.25 + 3.74 * rng.random((n, dim))) * 2 ** _Q) / 2 ** _Q * rng.choice([-1.0, 1.0], size=(n, dim))
    for r in zero_rows:
        x[r] = 0.0
    return np.ascontiguousarray(x)


def clustered_vectors(n: int, dim: int, seed: int, groups: int = 5, noise: float = 0.12) -> np.ndarray:
    """Rows around ``groups`` centres: pairs inside a group lie well above 0.9, the others well below."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((groups, dim))
    x = base[np.arange(n) % groups] + noise * rng.standard_normal((n, dim))
    return np.ascontiguousarray(np.rint(np.clip(x, -3.9, 3.9) * 2 ** _Q) / 2 ** _Q)


def _ints(x) -> np.ndarray:
    xi = np.rint(np.asarray(x, dtype=np.float64) * 2 ** _Q)
    assert np.array_equal(xi / 2 ** _Q, np.asarray(x, dtype=np.float64)) and np.abs(xi).max(initial=0) <= 4 * 2 ** _Q
    return xi.astype(np.int64)


def _quot(dot: int, qq: int, vv: int, eps_scaled: Optional[Decimal]) -> Decimal:
    with localcontext() as ctx:
        ctx.prec = 50
        if eps_scaled is None:
            return Decimal(0) if qq == 0 or vv == 0 else Decimal(dot) / (Decimal(qq) * Decimal(vv)).sqrt()
        return Decimal(dot) / ((Decimal(qq) * Decimal(vv)).sqrt() + eps_scaled)


def exact_cosine(q, x) -> List[Decimal]:
    """dot / (|q| |x_i|), 0 when a norm is zero: exact sums (int64, see ``cosine_vectors``), 50-digit quotient."""
    qi, xi = _ints(q), _ints(x)
    dots, qq, vv = xi @ qi, int(qi @ qi), (xi * xi).sum(axis=1)
    return [_quot(int(d), qq, int(v), None) for d, v in zip(dots, vv)]


def exact_matrix(x) -> List[List[Decimal]]:
    xi = _ints(x)
    g = xi @ xi.T
    return [[_quot(int(g[i, j]), int(g[i, i]), int(g[j, j]), None) for j in range(len(xi))] for i in range(len(xi))]


def exact_adjacent(x, eps: float) -> List[Decimal]:
    """dot / (|x_i| |x_i+1| + eps), the segmenter's rule: no zero-norm branch."""
    xi = _ints(x)
    with localcontext() as ctx:
        ctx.prec = 50
        e = Decimal(float(eps)) * Decimal(2 ** (2 * _Q))
    return [_quot(int(xi[i] @ xi[i + 1]), int(xi[i] @ xi[i]), int(xi[i + 1] @ xi[i + 1]), e) for i in range(len(xi) - 1)]


def max_error(got, exact) -> float:
    """max |got - exact| with the difference taken in decimal arithmetic (no rounding of the reference)."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    flat = [e for row in exact for e in row] if exact and isinstance(exact[0], list) else list(exact)
    assert len(flat) == len(got)
    with localcontext() as ctx:
        ctx.prec = 50
        return float(max((abs(Decimal(float(g)) - e) for g, e in zip(got, flat)), default=Decimal(0)))
