"""GPU tests of the batched dense re-rank: ``mrag_index_score_rows_batch`` against ``mrag_index_score_rows`` bit for bit on
every index case and batch structure of ``tests/rerank_batch_cases.py``, both against the host's restatement of the
summation order, its refusals through ctypes, and
``DenseRetrievalBackend(dense_mode="rerank")`` with ``run_batch`` against ``run``."""
import ctypes as C
import json
import zlib

import numpy as np
import pytest

import rerank_batch_cases as rc

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


_made = {}


def _index(case):
    """one index per case for the whole module, never changed after it is built"""
    from mrag_amd.index import DenseIndex
    if case not in _made:
        dim, dtype, kind = case
        ix = DenseIndex(dim, metric="cosine", dtype=dtype)
        ix.add(rc.make_rows(dim, kind, dtype), normalize=rc.normalize_flag(kind))
        _made[case] = ix
    return _made[case]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for ix in _made.values():
        ix.close()
    _made.clear()


STRUCTURES = rc.structures()


# ------------------------------------------------------------------------------------------------ kernel and entry point
@pytest.mark.parametrize("case", rc.INDEX_CASES, ids=rc.case_id)
def test_every_question_has_the_single_calls_bits(case):
    dim, dtype, kind = case
    ix, norm = _index(case), rc.normalize_flag(kind)
    for name, lists in STRUCTURES.items():
        q = rc.structure_queries(dim, kind, name, lists)
        got = ix.score_rows_batch(q, lists, normalize=norm)
        assert len(got) == len(lists)
        for g, ids in enumerate(lists):
            want = ix.score_rows(q[g], ids, normalize=norm)
            assert (_bits(got[g]) == _bits(want)).all(), (name, g, len(ids))
            out = (ids < 0) | (ids >= rc.N_ROWS)
            assert (_bits(got[g][out]) == 0).all()                                # exactly +0.0
        ptr, flat = rc.to_csr(lists)
        p2, f2 = ix.score_rows_batch(q, (ptr, flat), normalize=norm)             # the CSR form is the same call
        assert (p2 == ptr).all() and (_bits(f2) == _bits(np.concatenate(got) if got else [])).all()
        if name == "a thousand questions":
            a, b, c = (got[g] for g in rc.SAME_AT)
            assert len(a) == rc.R + 7 and (_bits(a) == _bits(b)).all() and (_bits(a) == _bits(c)).all()
        if name == "thirty-three questions of every length":
            perm = np.random.default_rng(9).permutation(len(lists))
            moved = ix.score_rows_batch(q[perm], [lists[g] for g in perm], normalize=norm)
            assert all((_bits(moved[j]) == _bits(got[g])).all() for j, g in enumerate(perm))
            assert (got[1] == 0.0).all() and len(got[1]) == 1


def test_cosine_f16_scores_match_the_oracles_dot():
    from oracle import dense_search as ds
    case = (768, "f16", "cosine")
    ix = _index(case)
    c16 = ds.normalize_round(rc.make_rows(768, "cosine"))
    name = "thirty-three questions of every length"
    lists = STRUCTURES[name]
    q = rc.structure_queries(768, "cosine", name, lists)
    q16 = ds.normalize_round(q).astype(np.float64)
    got = ix.score_rows_batch(q, lists)
    for g, ids in enumerate(lists):
        want = np.asarray([float(c16[i].astype(np.float64) @ q16[g]) if 0 <= i < rc.N_ROWS else 0.0 for i in ids])
        np.testing.assert_allclose(got[g], want, rtol=0, atol=1e-6)


def test_a_search_is_not_disturbed_by_a_thousand_question_rerank():
    """the batch keeps its prepared queries in a buffer of its own: the search's zero-padded query buffer is as it was"""
    case = (200, "f16", "cosine")
    ix = _index(case)
    qs = rc.make_queries(200, "cosine", 5, seed=77)
    before = ix.search(qs, 10)
    name = "a thousand questions"
    ix.score_rows_batch(rc.structure_queries(200, "cosine", name, STRUCTURES[name]), STRUCTURES[name])
    after = ix.search(qs, 10)
    assert (before[1] == after[1]).all() and (_bits(before[0]) == _bits(after[0])).all()
    one_b = ix.search(qs[:1], 10)
    ix.score_rows_batch(rc.make_queries(200, "cosine", 300), [np.arange(5)] * 300)
    one_a = ix.search(qs[:1], 10)
    assert (one_b[1] == one_a[1]).all() and (_bits(one_b[0]) == _bits(one_a[0])).all() and (one_a[1][0] == after[1][0]).all()


def test_a_search_is_not_disturbed_by_a_single_lookup():
    """the single call prepares its query in row 0 of the search's query buffer and records that, so the next search
    finds its zero padding as it needs it"""
    ix = _index((200, "f16", "cosine"))
    qs = rc.make_queries(200, "cosine", 5, seed=77)
    lookup = rc.make_queries(200, "cosine", 1, seed=78)[0]
    for part in (qs, qs[:1]):
        before = ix.search(part, 10)
        ix.score_rows(lookup, np.arange(200))
        after = ix.search(part, 10)
        assert (before[1] == after[1]).all() and (_bits(before[0]) == _bits(after[0])).all()


@pytest.mark.parametrize("case", [c for c in rc.INDEX_CASES if c[2] == "wide"], ids=rc.case_id)
def test_wide_scores_are_the_contracts_sum_bit_for_bit(case):
    """A wide case is stored and asked without normalisation, so the kernel's operands are the storage roundings of the
    host's values and its score is ``sum_kernel_order`` of their exact products.  Asked: the anchor query over the
    cancelling rows, whose float32 score depends on that order (tests/test_rerank_batch_host.py), by both entry points."""
    dim, dtype, kind = case
    ix = _index(case)
    q = rc.anchor_query(dim, kind)
    ids = np.arange(rc.N_ROWS - rc.N_CANCEL, rc.N_ROWS, dtype=np.int64)
    rows16 = rc.round_storage(rc.make_rows(dim, kind, dtype)[ids], dtype)
    want = rc.sum_kernel_order(rc.products(rows16, rc.round_storage(q, dtype)))
    single = ix.score_rows(q, ids, normalize=False)
    batch = ix.score_rows_batch(q[None, :], [ids], normalize=False)[0]
    assert (_bits(single) == _bits(want)).all(), np.flatnonzero(_bits(single) != _bits(want))
    assert (_bits(batch) == _bits(want)).all(), np.flatnonzero(_bits(batch) != _bits(want))


def test_refusals_name_the_question_and_leave_the_handle_usable():
    from mrag_amd import _native as N
    lib = N.load()
    ix = _index((64, "f16", "cosine"))
    q = np.ascontiguousarray(rc.make_queries(64, "cosine", 3))
    ids = np.arange(6, dtype=np.int64)
    good = np.asarray([0, 2, 2, 6], dtype=np.int64)
    out = np.full(6, 7.0, dtype=np.float32)
    want = np.concatenate(ix.score_rows_batch(q, [ids[0:2], ids[2:2], ids[2:6]]))

    def call(h=None, queries=q, q_dtype=N.MRAG_F32, nq=3, ptr=good, row_ids=ids, scores=out):
        p = lambda a: None if a is None else a.ctypes.data                        # noqa: E731
        return lib.mrag_index_score_rows_batch(ix._h if h is None else h, p(queries), q_dtype, 1, nq, p(ptr), p(row_ids), p(scores), None)

    def refused(st, *words):
        msg = lib.mrag_last_error().decode()
        assert st == -1 and all(w in msg for w in words), (st, msg)
        assert (out == 7.0).all()                                                 # before any device work: nothing written
        assert call() == 0 and (_bits(out) == _bits(want)).all()                  # and the handle serves the next call
        out[:] = 7.0

    refused(call(nq=-1), "n_questions")
    refused(call(ptr=np.asarray([1, 2, 2, 6], dtype=np.int64)), "row_ptr[0]", "question 0")
    refused(call(ptr=np.asarray([0, 4, 2, 6], dtype=np.int64)), "decreases", "question 1")
    refused(call(ptr=np.asarray([0, 2, 6, 5], dtype=np.int64)), "decreases", "question 2")
    refused(call(queries=None), "NULL")
    refused(call(row_ids=None), "NULL")
    refused(call(scores=None), "NULL")
    refused(call(ptr=None), "row_ptr")
    refused(call(q_dtype=9), "dtype 9")
    refused(call(h=C.c_uint64(0xdead)), "invalid handle")
    # nothing to do is not an error and needs no buffer
    assert call(nq=0, queries=None, ptr=None, row_ids=None, scores=None) == 0
    assert call(ptr=np.zeros(4, dtype=np.int64), queries=None, row_ids=None, scores=None) == 0 and (out == 7.0).all()


# ------------------------------------------------------------------------------------------------ the backend
WORDS = ["alpha", "beta", "gamma", "delta", "river", "city", "king", "queen", "novel", "author", "film", "league", "team",
         "science", "island", "bridge", "album", "born"]


def _pm1_vec(text, dim=64):
    """16 entries of +-1: every cosine is a multiple of 1/16 that any summation order gives exactly -- no encoder enters"""
    rng = np.random.default_rng(zlib.crc32(text.encode("utf-8")))
    v = np.zeros(dim, dtype=np.float32)
    v[rng.choice(dim, size=16, replace=False)] = rng.choice([-1.0, 1.0], size=16)
    return v.tolist()


class _Router:
    def embed(self, *, model_hint, texts, require=None):
        return {"vectors": [_pm1_vec(t) for t in texts]}


def _synthetic_rows():
    return [{"doc_id": f"T{i // 4}#{i % 4}", "title": f"T{i // 4}", "sent_id": i % 4,
             "text": f"sentence {i} about topic {i % 37} and {i % 11}"} for i in range(1500)]


@pytest.fixture(scope="module", params=["f3", "synthetic"])
def docs(request, tmp_path_factory, golden_dir):
    from mrag_amd import corpus
    rows = (json.loads((golden_dir / "f3_hybrid_run.json").read_text())["docs_rows"] if request.param == "f3" else _synthetic_rows())
    path = tmp_path_factory.mktemp("rerank_batch_" + request.param) / "docs.jsonl"
    corpus.write_docs_jsonl(path, rows)
    corpus.drop_shared("dense-index|"); corpus.drop_shared("bm25-index|")
    yield str(path), rows
    corpus.drop_shared("dense-index|"); corpus.drop_shared("bm25-index|")


def _reqs(n, synthetic):
    from mrag_amd.dto import RetrievalIn
    rng = np.random.default_rng(17)
    if synthetic:      # that corpus speaks in numbers
        queries = [f"sentence {rng.integers(1500)} topic {rng.integers(37)} and {rng.integers(11)}" for _ in range(n)]
    else:
        queries = [" ".join(rng.choice(WORDS, size=int(rng.integers(2, 5)))) for _ in range(n)]
    return [RetrievalIn(query=q, graph_id="", top_k=(1, 15, 40)[g % 3], trace_id=f"t{g}") for g, q in enumerate(queries)]


def test_rerank_run_batch_is_run_and_stays_inside_the_bm25_pool(docs, monkeypatch):
    from mrag_amd import fusion
    from mrag_amd.backend import DenseRetrievalBackend
    from mrag_amd.index import DenseIndex
    path, rows = docs
    kw = dict(index_path=path, text_channel="bm25", dense_pool_k=20, fuse_on_device=True)
    be = DenseRetrievalBackend(_Router(), dense_mode="rerank", **kw)
    calls = []
    real = DenseIndex.score_rows_batch
    monkeypatch.setattr(DenseIndex, "score_rows_batch", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    reqs = _reqs(64, len(rows) == 1500)
    want = [be.run(r) for r in reqs]
    assert not calls                                                              # run scores by the single call
    for B in (1, 7, 64):
        got = be.run_batch(reqs[:B])
        assert len(calls) == 1 and len(got) == B                                  # ONE batched lookup per run_batch
        calls.clear()
        for g in range(B):
            assert got[g]["hits"] == want[g]["hits"], (B, g)
            diag = dict(got[g]["diagnostics"])
            assert diag.pop("batch_size") == B and diag == want[g]["diagnostics"]
    # every hit is one of the question's BM25 candidates; the corpus-wide mode finds hits outside them
    searcher = be.text_search
    wide = DenseRetrievalBackend(_Router(), dense_mode="search", **kw)
    outside = 0
    for r, w in zip(reqs, want):
        d = w["diagnostics"]
        pool = max(r.top_k, 20)
        cand = searcher(queries=[r.query], top_k=pool)
        cand_ids = {fusion.normalize_id(h)[0] for h in cand}
        assert d["dense_mode"] == "rerank" and d["dense_error"] is None and d["text_error"] is None
        assert d["bm25_candidates"] == len(cand) == d["pool"]["dense_pool_k_effective"] and d["dense_scored"] == len(cand_ids)
        assert {h["id"] for h in w["hits"]} <= cand_ids and len(w["hits"]) == min(r.top_k, len(cand_ids))
        stray = {h["id"] for h in wide.run(r)["hits"]} - cand_ids
        if stray:
            outside += 1
            assert not stray & {h["id"] for h in w["hits"]}
    assert outside > 0
