"""The batched BM25 search (csrc/bm25.hip, ``HipBM25Index.search_batch``) and the allow-set of the text channel on the
device -- the cases of ``tests/bm25_batch_cases.py``; ``tests/test_bm25_batch_host.py`` shows on the CPU what each can see.

No tolerances: every comparison is documents plus score bits.  Expected values are ``oracle.bm25`` per question
(``search_postings``; with an allow-set ``select_topk`` over the masked ``merged_scores``), and where it is cheap the
single search ``HipBM25Index.search`` on the same index as well.
"""
import ctypes as C

import numpy as np
import pytest

import bm25_batch_cases as bc
from oracle import bm25 as ob
from oracle import text_cases as tc

pytestmark = pytest.mark.gpu

_bits = bc.bits
_REAL = {}


def _build():
    """The library's own ``build_postings`` (the tests below replace the module attribute to share one build per corpus)."""
    from mrag_amd import text_index as ti
    return _REAL.setdefault("build_postings", ti.build_postings)


def _index(p, rows, monkeypatch, k1=1.5, b=0.75):
    from mrag_amd import text_index as ti
    _build()
    monkeypatch.setattr(ti, "build_postings", lambda rows_, k1_, b_: p)
    ix = ti.HipBM25Index(rows=rows, k1=k1, b=b)
    assert (ix.N, ix.k1, ix.b) == (p["N"], k1, b)
    return ix


def _all_bits(lists):
    return [_bits(r) for r in lists]


class _Abi:
    """``mrag_bm25_search_batch`` on hand-made postings, queries as (term ids, idfs)."""

    def __init__(self, p, k1=1.5):
        from mrag_amd import _native as N
        self.N, self.lib, self.h, self.n_docs = N, N.load(), C.c_uint64(0), p["N"]
        N.check(self.lib.mrag_bm25_create(0, p["N"], len(p["indptr"]) - 1, p["indptr"].ctypes.data, p["post_doc"].ctypes.data,
                                          p["post_tf"].ctypes.data, p["doc_norm"].ctypes.data, float(k1 + 1), C.byref(self.h)))

    def raw(self, g_ptr, q_ptr, q_terms, q_idf, merge, k, allow=None):
        """-> (status, one ranked list per question)"""
        g_ptr, q_ptr = np.asarray(g_ptr, dtype=np.int32), np.asarray(q_ptr, dtype=np.int32)
        q_terms, q_idf = np.asarray(list(q_terms) or [0], dtype=np.int32), np.asarray(list(q_idf) or [0.0], dtype=np.float64)
        nq = len(g_ptr) - 1
        kk = max(k, 1)
        docs, scores = np.full((nq, kk), 7, dtype=np.int64), np.full((nq, kk), 7.0, dtype=np.float64)
        n = np.full(nq, 7, dtype=np.int32)
        st = self.lib.mrag_bm25_search_batch(self.h, nq, g_ptr.ctypes.data, q_ptr.ctypes.data, q_terms.ctypes.data, q_idf.ctypes.data,
                                             1 if merge == "sum" else 0, k, None if allow is None else allow.ctypes.data,
                                             docs.ctypes.data, scores.ctypes.data, n.ctypes.data, None)
        if st == 0:
            for g in range(nq):                                  # the slots past out_n are (-1, 0.0)
                assert (docs[g, n[g]:] == -1).all() and (scores[g, n[g]:].view(np.uint64) == 0).all()
        return st, [list(zip(docs[g, :n[g]].tolist(), scores[g, :n[g]].tolist())) for g in range(nq)]

    def batch(self, questions, k, merge):
        queries = [q for qs in questions for q in qs]
        g_ptr = np.cumsum([0] + [len(qs) for qs in questions])
        q_ptr = np.cumsum([0] + [len(ids) for ids, _ in queries])
        st, got = self.raw(g_ptr, q_ptr, [t for ids, _ in queries for t in ids], [v for _, idfs in queries for v in idfs], merge,
                           min(k, self.n_docs))
        assert st == 0, self.lib.mrag_last_error()
        return got

    def close(self):
        self.lib.mrag_bm25_destroy(self.h)


# ------------------------------------------------------------------------------------------------ 1 grouping
@pytest.mark.parametrize("merge", ("max", "sum"))
@pytest.mark.parametrize("shape", ("singles", "rotation"))
def test_grouping_equals_the_oracle_and_the_single_search(shape, merge, monkeypatch):
    p = bc.case_postings(bc.ZIPF_CASE, _build())
    questions = bc.grouping_singles() if shape == "singles" else bc.grouping_rotation()
    want = bc.expected(("zipf", shape), p, questions, bc.GROUP_K, merge)
    ix = _index(p, bc.case_named(bc.ZIPF_CASE).corpus(), monkeypatch)
    try:
        got = ix.search_batch(questions, top_k=bc.GROUP_K, alpha_merge=merge)
        assert len(got) == len(questions) == (1024 if shape == "singles" else len(want))
        for g, qs in enumerate(questions):
            assert _bits(got[g]) == _bits(want[g]), (g, qs)
            assert _bits(got[g]) == _bits(ix.search(list(qs), top_k=bc.GROUP_K, alpha_merge=merge)), (g, qs)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 2 position independence
def test_a_question_gets_the_same_bits_wherever_it_stands_and_scratch_is_reused(monkeypatch):
    p = bc.case_postings(bc.ZIPF_CASE, _build())
    probe = _bits(bc.expected("probe", p, [bc.PROBE], bc.GROUP_K, "max")[0])
    assert len(probe) == bc.GROUP_K
    ix = _index(p, bc.case_named(bc.ZIPF_CASE).corpus(), monkeypatch)
    try:
        first = None
        for where in (0, bc.POSITION_N // 2, bc.POSITION_N - 1):
            batch = bc.position_batch(where)
            got = _all_bits(ix.search_batch(batch, top_k=bc.GROUP_K))
            assert len(got) == bc.POSITION_N and got[where] == probe, where
            if where == 0:
                first = got
                assert first[1:] == _all_bits(bc.expected("position-fill", p, batch[1:], bc.GROUP_K, "max"))
        other = bc.other_size_batch()
        assert _all_bits(ix.search_batch(other, top_k=50, alpha_merge="sum")) == _all_bits(bc.expected("other", p, other, 50, "sum"))
        batch = bc.position_batch(0)
        assert _all_bits(ix.search_batch(batch, top_k=bc.GROUP_K)) == first            # after a batch of another size
        assert _all_bits(ix.search_batch(batch, top_k=bc.GROUP_K)) == first            # and twice in a row
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 3 chunk boundary
@pytest.mark.parametrize("n_docs", (257, 1, 2))
def test_chunk_boundaries_do_not_show_in_the_result(n_docs, monkeypatch):
    questions = bc.chunk_questions()
    assert [len(qs) for qs in questions] == list(bc.CHUNK_SIZES)
    for tag, k1, b in bc.SMALL_SETTINGS:
        case = bc.case_named(f"small-{n_docs}-{tag}")
        p = bc.case_postings(case.name, _build())
        ix = _index(p, case.corpus(), monkeypatch, k1, b)
        try:
            for merge in ("max", "sum"):
                want = _all_bits(bc.expected(("small", n_docs, tag), p, questions, n_docs, merge, k1))
                ix.set_scratch_limit(bc.chunk_limit(n_docs))
                cut = _all_bits(ix.search_batch(questions, top_k=10 ** 9, alpha_merge=merge))
                ix.set_scratch_limit(0)
                whole = _all_bits(ix.search_batch(questions, top_k=10 ** 9, alpha_merge=merge))
                assert cut == want and whole == want, (n_docs, tag, merge)
        finally:
            ix.close()


# ------------------------------------------------------------------------------------------------ 4 above the selection grid
@pytest.mark.parametrize("merge", ("max", "sum"))
def test_three_questions_above_the_selection_grid(merge, monkeypatch):
    p = bc.case_postings(bc.KINDS_CASE, _build())
    assert p["N"] == tc.STRIDE_N > tc.GRID
    ix = _index(p, tc.rows_kinds(), monkeypatch)
    try:
        for k in bc.KINDS_KS:
            want = bc.expected("kinds", p, bc.KINDS_QUESTIONS, k, merge)
            got = ix.search_batch(bc.KINDS_QUESTIONS, top_k=k, alpha_merge=merge)
            assert _all_bits(got) == _all_bits(want), (k, merge)
    finally:
        ix.close()


def test_two_questions_that_are_one_tie_group(monkeypatch):
    p = bc.case_postings(bc.SAME_CASE, _build())
    ix = _index(p, tc.rows_same(), monkeypatch)
    try:
        for k in bc.SAME_KS:
            want = bc.expected("same", p, bc.SAME_QUESTIONS, k, "max")
            got = ix.search_batch(bc.SAME_QUESTIONS, top_k=k)
            assert _all_bits(got) == _all_bits(want) and [d for d, _ in got[1]] == list(range(k)), k
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 5 through the C ABI
def test_low_score_bytes_on_two_handles():
    handles = [(best_last, tc.postings_low_bytes(best_last)) for best_last in (True, False)]
    open_ = [(best_last, p, _Abi(p)) for best_last, p in handles]
    try:
        for k in bc.LOW_KS:
            for best_last, p, ix in open_:
                want = _all_bits(bc.expected(("low", best_last), p, bc.LOW_QUESTIONS, k, "max"))
                assert _all_bits(ix.batch(bc.LOW_QUESTIONS, k, "max")) == want, (best_last, k)
    finally:
        for _, _, ix in open_:
            ix.close()


def test_negative_idf_batch():
    p = tc.postings_negative_idf()
    ix = _Abi(p)
    try:
        for merge in ("sum", "max"):
            for k in bc.NEG_KS:
                want = _all_bits(bc.expected("neg", p, bc.NEG_QUESTIONS, k, merge))
                assert _all_bits(ix.batch(bc.NEG_QUESTIONS, k, merge)) == want, (merge, k)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 6 allow-set
def test_allow_set_on_the_zipf_corpus(monkeypatch):
    from mrag_amd.index import allow_bits
    p = bc.case_postings(bc.ZIPF_CASE, _build())
    questions = bc.allow_questions()
    masks = bc.allow_masks(p, lambda: bc.unfiltered_top1(p, questions))
    ix = _index(p, bc.case_named(bc.ZIPF_CASE).corpus(), monkeypatch)
    try:
        plain = _all_bits(ix.search_batch(questions, top_k=bc.ALLOW_K))
        assert plain == _all_bits(bc.expected("allow-unfiltered", p, questions, bc.ALLOW_K, "max"))
        for name, mask in masks.items():
            want = _all_bits(bc.expected(("allow", name), p, questions, bc.ALLOW_K, "max", allowed=mask))
            got = _all_bits(ix.search_batch(questions, top_k=bc.ALLOW_K, allow=mask))
            assert got == want, name
            if name == "all":
                assert got == plain
            if name == "none":
                assert all(r == [] for r in got)
            # row ids and packed bits are the same set; one question through search(allow=) is the batch's entry
            assert _all_bits(ix.search_batch(questions, top_k=bc.ALLOW_K, allow=np.nonzero(mask)[0])) == got, name
            assert _all_bits(ix.search_batch(questions, top_k=bc.ALLOW_K, allow=allow_bits(mask, p["N"]))) == got, name
            for g in (0, 7, 63):
                assert _bits(ix.search(list(questions[g]), top_k=bc.ALLOW_K, allow=mask)) == got[g], (name, g)
        sums = _all_bits(ix.search_batch(questions, top_k=bc.ALLOW_K, alpha_merge="sum", allow=masks["third"]))
        assert sums == _all_bits(bc.expected(("allow", "third"), p, questions, bc.ALLOW_K, "sum", allowed=masks["third"]))
    finally:
        ix.close()


def test_allow_set_cuts_a_tie_group_in_a_partial_last_word(monkeypatch):
    p = bc.postings_of("same-cut", bc.same_cut_rows, _build())
    assert p["N"] == bc.SAME_CUT_N and p["N"] % 32 == 8
    odd = np.arange(p["N"]) % 2 == 1
    ix = _index(p, bc.same_cut_rows(), monkeypatch)
    try:
        for k in (bc.SAME_CUT_K, 10 ** 9):                        # cut by k; and every odd document, the last word included
            want = bc.expected("same-cut", p, bc.SAME_QUESTIONS, min(k, p["N"]), "max", allowed=odd)
            got = ix.search_batch(bc.SAME_QUESTIONS, top_k=k, allow=odd)
            assert _all_bits(got) == _all_bits(want)
            assert [d for d, _ in got[0]] == list(range(1, p["N"], 2))[:k]
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 7 errors
def test_errors_have_the_single_search_status_and_leave_the_handle_usable():
    p = tc.postings_negative_idf()
    ix = _Abi(p)
    ids, idfs = [0, 2], [0.5, 0.25]
    good = (([0], [0.5]), ([2, 0], [0.25, 0.5]))

    def serves():
        want = _all_bits(bc.expected("errors-good", p, [good, good[:1], ()], 50, "sum"))
        assert _all_bits(ix.batch([good, good[:1], ()], 50, "sum")) == want

    try:
        serves()
        st, _ = ix.raw([0, 1, 2], [0, 1, 2], ids, idfs, "max", 4097)
        assert st == -5                                                      # MRAG_ERR_UNSUPPORTED, as mrag_bm25_search
        serves()
        st, _ = ix.raw([0, 1, 1026], list(range(1027)), [0] * 1026, [0.5] * 1026, "max", 10)
        assert st == -5                                                      # 1025 queries in one question
        serves()
        st, got = ix.raw([0, 1024, 2048], list(range(2049)), [0] * 2048, [0.5] * 2048, "max", 10)
        assert st == 0 and len(got[0]) == len(got[1]) == 10                  # 1024 per question is served, twice over
        st, _ = ix.raw([0, 2, 1, 2], [0, 1, 2], ids, idfs, "max", 10)
        assert st == -1                                                      # g_ptr not monotone: MRAG_ERR_INVALID
        serves()
        st, _ = ix.raw([0, 1, 2, 3], [0, 1, 2, 3], [0, 2, 3], [0.5, 0.25, 0.5], "max", 10)
        assert st == -1                                                      # term id 3 of 3 terms, in the last question
        serves()
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 8 searcher
def test_searcher_batch_equals_the_oracle_hits_and_the_single_searcher():
    from mrag_amd.text_index import HipBM25Index, HipBM25TextSearcher
    rows = bc.searcher_rows()
    assert len(rows) == 60
    oracle = ob.Bm25Oracle(rows)
    searcher = HipBM25TextSearcher(HipBM25Index(rows=rows))
    try:
        for top_k in (5, 60):
            got = searcher.search_batch(queries=bc.SEARCHER_QUESTIONS, top_k=top_k)
            assert len(got) == len(bc.SEARCHER_QUESTIONS)
            for qs, hits in zip(bc.SEARCHER_QUESTIONS, got):
                assert hits == oracle.hits(list(qs), top_k)
                assert hits == searcher.search(queries=list(qs), top_k=top_k)
            assert any(got) and not all(got)
        even = np.arange(60) % 2 == 0                              # k = N: nothing is cut, so the filter commutes with the search
        pos = {"sent::%s::%s" % (r["doc_id"], str(r["sent_id"] or "")): i for i, r in enumerate(rows)}
        assert len(pos) == 60
        for qs, hits in zip(bc.SEARCHER_QUESTIONS, searcher.search_batch(queries=bc.SEARCHER_QUESTIONS, top_k=60, allow=even)):
            assert hits == [h for h in oracle.hits(list(qs), 60) if even[pos[h["id"]]]]
    finally:
        searcher.index.close()
