"""What the batched BM25 tests can see, established on the CPU with the oracle alone (no kernel runs here): every case of
``tests/bm25_batch_cases.py`` meets the condition it was built for.  Plus the host side of the feature: the two new C
entry points are declared, bound and exported, and ``HipBM25Index`` answers the degenerate calls and packs an allow-set
without touching the device.  Conditions on the inputs, not measurements of the code under test.
"""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import bm25_batch_cases as bc
from oracle import bm25 as ob
from oracle import text_cases as tc

ROOT = Path(__file__).resolve().parents[1]
NEW = {"mrag_bm25_search_batch": 13, "mrag_bm25_set_scratch_limit": 2}


@pytest.fixture(autouse=True)
def _the_feature_exists():
    """The cases below are inputs of ``search_batch``: without it they describe nothing."""
    from mrag_amd import _native as N
    from mrag_amd.text_index import HipBM25Index, HipBM25TextSearcher
    assert set(NEW) <= set(N.EXTENSION_SIGNATURES)
    assert callable(getattr(HipBM25Index, "search_batch", None)) and callable(getattr(HipBM25TextSearcher, "search_batch", None))


def _build():
    from mrag_amd.text_index import build_postings
    return build_postings


# ------------------------------------------------------------------------------------------------ ABI and host side
def test_abi_declares_binds_and_exports_the_batch_entry_points():
    from mrag_amd import _native as N
    hdr = (ROOT / "include" / "mrag_bm25_batch.h").read_text()
    assert '#include "mrag_bm25_batch.h"' in (ROOT / "include" / "mrag.h").read_text()      # mrag.h brings them along
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(mrag_\w+)\(([^;]*)\);", hdr, flags=re.M | re.S)}
    assert set(declared) == set(NEW) == set(N.EXTENSION_SIGNATURES) and not set(NEW) & set(N.SIGNATURES)
    for name, nargs in NEW.items():
        assert len(declared[name].split(",")) == nargs, name
        assert len(N.EXTENSION_SIGNATURES[name]) == nargs, name
    assert "text_index.py:71-97" in hdr[hdr.index("for a BATCH of questions"):hdr.index("int mrag_bm25_search_batch")]
    if not N.lib_path().exists():
        pytest.skip("libmrag_hip.so is not built")
    lib = ctypes.CDLL(str(N.lib_path()))
    for name in NEW:
        assert hasattr(lib, name), name


def test_degenerate_calls_and_keyword_defaults_need_no_device():
    from mrag_amd.text_index import HipBM25Index, HipBM25TextSearcher
    p = inspect.signature(HipBM25Index.search_batch).parameters
    assert (p["top_k"].default, p["alpha_merge"].default, p["allow"].default) == (20, "max", None)
    assert inspect.signature(HipBM25Index.search).parameters["allow"].default is None
    assert callable(HipBM25Index.set_scratch_limit)
    empty = HipBM25Index(rows=[])
    assert empty.search_batch([["a"], [], ["b c", "d"]]) == [[], [], []]
    assert empty.search_batch([]) == []
    assert HipBM25TextSearcher(empty).search_batch(queries=[["a"], ["b"]], top_k=5) == [[], []]
    ix = HipBM25Index.__new__(HipBM25Index)                     # no handle: anything native would fail
    ix.N, ix._h, ix._lib = 70, None, None
    assert ix.search_batch([], top_k=5) == [] and ix.search_batch([["w1"], ["w2"]], top_k=0) == [[], []]


def test_allow_forms_pack_to_the_same_words():
    from mrag_amd.index import allow_bits
    from mrag_amd.text_index import HipBM25Index
    ix = HipBM25Index.__new__(HipBM25Index)
    ix.N = bc.SAME_CUT_N
    mask = np.arange(ix.N) % 2 == 1
    words = ix._allow_words(mask)
    assert words.dtype == np.uint32 and words.shape == ((ix.N + 31) // 32,) and int(words[-1]) == 0b10101010
    for form in (mask.astype(np.uint8), np.nonzero(mask)[0], np.nonzero(mask)[0].astype(np.int32), list(np.nonzero(mask)[0]),
                 allow_bits(mask, ix.N)):
        assert np.array_equal(ix._allow_words(form), words)
    for bad in (np.zeros(ix.N + 1, dtype=bool), np.asarray([ix.N]), np.zeros(3, dtype=np.uint32), np.zeros(ix.N)):
        with pytest.raises(ValueError):
            ix._allow_words(bad)


# ------------------------------------------------------------------------------------------------ the cases
def _no_known_token(p, qs):
    return all(t < 0 for ids, _ in ob.query_term_ids(p, list(qs)) for t in ids)


def test_the_rotation_holds_empty_questions_and_questions_without_a_known_term():
    p = bc.case_postings(bc.ZIPF_CASE, _build())
    singles, rotation = bc.grouping_singles(), bc.grouping_rotation()
    assert len(singles) == tc.BM25_MAX_QUERIES and [s for (s,) in singles] == list(tc.many_queries())
    assert [s for qs in rotation for s in qs] == list(tc.many_queries())          # the same strings, in order
    sizes = [len(qs) for qs in rotation]
    assert sizes[:10] == [0, 1, 2, 3, 5, 0, 1, 2, 3, 5] and set(sizes) == {0, 1, 2, 3, 5}
    empty = [qs for qs in rotation if not qs]
    blank = [qs for qs in rotation if qs and not any(s.strip() for s in qs)]                       # only empty strings
    unknown = [qs for qs in rotation if any(s.strip() for s in qs) and _no_known_token(p, qs)]      # tokens, none of them known
    assert len(empty) >= 90 and len(blank) >= 1 and len(unknown) >= 1
    want = bc.expected(("zipf", "rotation"), p, rotation, bc.GROUP_K, "max")
    assert all(want[g] == [] for g, qs in enumerate(rotation) if not qs or _no_known_token(p, qs))
    assert sum(1 for r in want if len(r) == bc.GROUP_K) > 300                     # and most questions fill their k


def test_the_probe_question_has_a_full_result_and_the_batches_differ_in_size():
    p = bc.case_postings(bc.ZIPF_CASE, _build())
    assert len(bc.expected("probe", p, [bc.PROBE], bc.GROUP_K, "max")[0]) == bc.GROUP_K
    for where in (0, 150, 299):
        batch = bc.position_batch(where)
        assert len(batch) == bc.POSITION_N and batch[where] == bc.PROBE and batch.count(bc.PROBE) == 1
    assert 0 < len(bc.other_size_batch()) != bc.POSITION_N
    assert sum(len(qs) for qs in bc.other_size_batch()) != sum(len(qs) for qs in bc.position_batch(0))


def test_the_chunk_case_crosses_boundaries_of_three_rows():
    questions = bc.chunk_questions()
    sizes = [len(qs) for qs in questions]
    assert sizes == list(bc.CHUNK_SIZES) and sizes[:6] == [1, 3, 1, 4, 0, 2] and len(sizes) == 11
    for n_docs in (257, 1, 2):
        assert bc.chunk_limit(n_docs) // (8 * n_docs) == bc.CHUNK_ROWS            # the limit admits exactly 3 score rows
    chunks = bc.chunks_of(sizes, bc.CHUNK_ROWS)
    assert len(chunks) >= 4 and any(len(c) > 1 for c in chunks)                   # several boundaries, one chunk of two questions
    assert max(sizes) > bc.CHUNK_ROWS and [sizes.index(max(sizes))] in chunks     # a question that needs a chunk of its own
    assert bc.chunks_of(sizes, (1 << 30) // (8 * 257)) == [[g for g, n in enumerate(sizes) if n]]   # default limit: one chunk
    # the questions reach every kind the small cases hold: results, no known term, empty strings, no queries
    p = bc.case_postings("small-257-default", _build())
    want = bc.expected(("small", 257, "default"), p, questions, 257, "max")
    assert any(want) and any(not w for w, qs in zip(want, questions) if qs) and () in questions
    assert len({tuple(bc.bits(w)) for w in want}) >= 5


def test_the_stride_questions_need_the_second_stride_and_are_cut_at_different_places():
    p = bc.case_postings(bc.KINDS_CASE, _build())
    assert p["N"] == tc.STRIDE_N > tc.GRID
    for merge in ("max", "sum"):
        for k in bc.KINDS_KS:
            want = bc.expected("kinds", p, bc.KINDS_QUESTIONS, k, merge)
            for qs, w in zip(bc.KINDS_QUESTIONS, want):
                assert sum(1 for d, _ in w if d >= tc.GRID) >= 4                  # documents the first sweep of the grid does not reach
                assert bc.bits(w) != bc.bits(ob.search_postings(p, list(qs), k, merge, 1.5, "first_stride_only"))
            assert [len(w) for w in want] == [len(tc.RARE_DOCS), k, k]            # one question is not cut at all,
            assert want[1][-1] != want[2][-1] and want[1][-1][0] != want[2][-1][0]   # the others at different documents
            fin = ob.merged_scores(p, list(bc.KINDS_QUESTIONS[1]), merge)
            assert (fin == want[1][-1][1]).sum() > k                               # inside a tie group larger than what is taken
    ps = bc.case_postings(bc.SAME_CASE, _build())
    for k in bc.SAME_KS:
        want = bc.expected("same", ps, bc.SAME_QUESTIONS, k, "max")
        assert [[d for d, _ in w] for w in want] == [list(range(k))] * 2 and len({s for w in want for _, s in w}) == 1


def test_the_abi_batches_repeat_the_single_cases():
    assert bc.LOW_QUESTIONS == ((tc.BM25_CASES[3].query_sets[0][0],),) * 3 and tc.BM25_CASES[3].name == "low-bytes"
    assert bc.LOW_KS == tc.BM25_CASES[3].ks == tc.BM25_CASES[4].ks
    neg = bc.case_named("negative-idf")
    assert bc.NEG_QUESTIONS == tuple(tuple(qs) for qs in neg.query_sets) and bc.NEG_KS == neg.ks and len(bc.NEG_QUESTIONS) == 3
    p = tc.postings_negative_idf()
    for merge in neg.merges:
        want = bc.expected("neg", p, bc.NEG_QUESTIONS, 600, merge)
        assert len({tuple(bc.bits(w)) for w in want}) == 3 and len({len(w) for w in want}) >= 2     # different answers, different counts
        fins = [ob.merged_scores(p, list(qs), merge) for qs in bc.NEG_QUESTIONS]
        assert all((f > 0).any() for f in fins) and any((f < 0).any() for f in fins)    # s > 0 decides what is a candidate


def test_the_masks_change_what_is_expected():
    p = bc.case_postings(bc.ZIPF_CASE, _build())
    questions = bc.allow_questions()
    assert len(questions) == bc.ALLOW_N_QUESTIONS and {len(qs) for qs in questions} == {1, 2, 3}
    base = bc.expected("allow-unfiltered", p, questions, bc.ALLOW_K, "max")
    assert all(len(w) == bc.ALLOW_K for w in base)
    top1 = bc.unfiltered_top1(p, questions)
    assert top1 == [base[g][0][0] for g in range(8)] and len(set(top1)) == 8      # the forbidden documents really led
    masks = bc.allow_masks(p, lambda: top1)
    assert list(masks) == ["all", "none", "third", "few", "no-top1"]
    changed = {}
    for name, mask in masks.items():
        want = bc.expected(("allow", name), p, questions, bc.ALLOW_K, "max", allowed=mask)
        changed[name] = [bc.bits(a) != bc.bits(b) for a, b in zip(want, base)]
        assert all(mask[d] for w in want for d, _ in w)
    assert not any(changed["all"]) and all(changed["none"])
    assert sum(changed["third"]) >= 32 and sum(changed["few"]) >= 32             # at least half of the questions
    assert all(changed["no-top1"][:8]) and masks["no-top1"].sum() == p["N"] - 8
    few = bc.expected(("allow", "few"), p, questions, bc.ALLOW_K, "max", allowed=masks["few"])
    assert {d for w in few for d, _ in w} >= {31, 32, 63, 64} and all(len(w) <= 5 for w in few)     # both sides of a word boundary
    # a score is what it is without the set: idf and avgdl are the corpus's
    third = bc.expected(("allow", "third"), p, questions, bc.ALLOW_K, "max", allowed=masks["third"])
    full = dict(ob.search_postings(p, list(questions[0]), p["N"], "max"))
    assert all(np.float64(s).view(np.uint64) == np.float64(full[d]).view(np.uint64) for d, s in third[0])
    # the tie group of the 1000-document corpus is cut by k inside the odd documents, and its last word is partial
    ps = bc.postings_of("same-cut", bc.same_cut_rows, _build())
    odd = np.arange(ps["N"]) % 2 == 1
    assert ps["N"] == 1000 == 31 * 32 + 8
    want = bc.expected("same-cut", ps, bc.SAME_QUESTIONS, bc.SAME_CUT_K, "max", allowed=odd)
    assert [d for d, _ in want[0]] == list(range(1, 200, 2)) and len({s for _, s in want[0]}) == 1
    whole = bc.expected("same-cut", ps, bc.SAME_QUESTIONS, ps["N"], "max", allowed=odd)
    assert [d for d, _ in whole[1]] == list(range(1, 1000, 2)) and whole[1][-1][0] == 999 >= 31 * 32


def test_the_searcher_corpus_gives_hits_and_empty_lists():
    rows = bc.searcher_rows()
    o = ob.Bm25Oracle(rows)
    hits = [o.hits(list(qs), 60) for qs in bc.SEARCHER_QUESTIONS]
    assert len(rows) == 60 and sum(1 for h in hits if h) >= 3 and sum(1 for h in hits if not h) >= 2
    assert len({h["id"] for hs in hits for h in hs}) > 10 and all(h["meta"]["source"] == "bm25" for hs in hits for h in hs)
    assert any(len(o.hits(list(qs), 5)) == 5 < len(h) for qs, h in zip(bc.SEARCHER_QUESTIONS, hits))        # top_k = 5 cuts
