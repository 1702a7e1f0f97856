"""The text channel (csrc/bm25.hip), the fusion kernel (csrc/fuse.hip) and the fp64 cosine kernels (csrc/cosine_pairs.hip) at the sizes and
edges where their launches change shape -- the cases of ``oracle/text_cases.py``; ``tests/test_text_channel_host.py``
shows on the CPU what each of them can see.

BM25: documents and score bits equal ``oracle.bm25.search_postings`` (pinned to the reference's outputs by the host file)
above the 1024 x 256 selection grid, with ties cut by ``k``, with scores that differ only in their low bytes, with 1024
queries, and at corpus sizes 1, 2 and 257.  Fusion: ``fuse_channels_device == fuse_channels`` as whole hit lists beyond
one element per thread, up to the 4096-entry limit.  Cosine: against the exact value, within ``COSINE_BOUND``.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import bm25 as ob
from oracle import text_cases as tc

pytestmark = pytest.mark.gpu

# |computed - exact| <= (2 dim + 8) * 2**-53: dim*u on the dot product and dim*u/2 on each norm for ANY summation order,
# plus the roundings of the square roots, the multiplication and the division; u = 2**-53.  A derived bound, not a
# measurement; it is not fitted to the kernel.
COSINE_BOUND = tc.cosine_bound


def _bits(ranked):
    return [(int(d), np.float64(s).view(np.uint64)) for d, s in ranked]


# ------------------------------------------------------------------------------------------------ BM25
class _AbiIndex:
    """``mrag_bm25_create`` / ``mrag_bm25_search`` on hand-made postings, queries as (term ids, idfs)."""

    def __init__(self, p, k1):
        from mrag_amd import _native as N
        self.N, self.lib, self.h, self.n_docs = N, N.load(), C.c_uint64(0), p["N"]
        N.check(self.lib.mrag_bm25_create(0, p["N"], len(p["indptr"]) - 1, p["indptr"].ctypes.data, p["post_doc"].ctypes.data,
                                          p["post_tf"].ctypes.data, p["doc_norm"].ctypes.data, float(k1 + 1), C.byref(self.h)))

    def search(self, queries, top_k, alpha_merge):
        q_ptr = np.cumsum([0] + [len(ids) for ids, _ in queries]).astype(np.int32)
        q_terms = np.asarray([t for ids, _ in queries for t in ids] or [0], dtype=np.int32)
        q_idf = np.asarray([v for _, idfs in queries for v in idfs] or [0.0], dtype=np.float64)
        k = min(top_k, self.n_docs)
        docs, scores, n = np.empty(k, dtype=np.int64), np.empty(k, dtype=np.float64), C.c_int(0)
        self.N.check(self.lib.mrag_bm25_search(self.h, len(queries), q_ptr.ctypes.data, q_terms.ctypes.data, q_idf.ctypes.data,
                                               1 if alpha_merge == "sum" else 0, k, docs.ctypes.data, scores.ctypes.data,
                                               C.byref(n), None))
        return list(zip(docs[:n.value].tolist(), scores[:n.value].tolist()))

    def close(self):
        self.lib.mrag_bm25_destroy(self.h)


def _postings(case):
    from mrag_amd.text_index import build_postings
    return tc.bm25_postings(case, build_postings)


def _open(case, monkeypatch):
    """The case's index on the device.  Text corpora go through ``HipBM25Index`` (its builder's result is shared with
    the oracle: one build per corpus); hand-made postings go through the C ABI."""
    p = _postings(case)
    if case.via == "abi":
        return _AbiIndex(p, case.k1)
    from mrag_amd import text_index as ti
    monkeypatch.setattr(ti, "build_postings", lambda rows, k1, b: p)
    ix = ti.HipBM25Index(rows=case.corpus(), k1=case.k1, b=case.b)
    assert (ix.N, ix.k1, ix.b) == (p["N"], case.k1, case.b)
    return ix


@pytest.mark.parametrize("case", tc.BM25_CASES, ids=lambda c: c.name)
def test_bm25_equals_the_postings_oracle(case, monkeypatch):
    p = _postings(case)
    ix = _open(case, monkeypatch)
    try:
        for queries, k, merge in case.runs():
            want = ob.search_postings(p, queries, k, merge, case.k1)
            got = ix.search(queries, top_k=case.top_k or k, alpha_merge=merge)
            assert _bits(got) == _bits(want), (case.name, queries[:3], k, merge)
    finally:
        ix.close()


def test_bm25_scratch_reuse_after_1024_queries_and_the_query_limit(monkeypatch):
    from mrag_amd._native import MragError
    case = next(c for c in tc.BM25_CASES if c.name == "many-queries")
    p, queries = _postings(case), list(case.query_sets[0])
    used, fresh = _open(case, monkeypatch), _open(case, monkeypatch)
    try:
        assert len(used.search(queries, top_k=200, alpha_merge="sum")) == 200
        for one in (["w3 w17 w3 w1200"], [queries[1]], ["nosuchterm"]):
            want = ob.search_postings(p, one, 200, "max")
            assert _bits(used.search(one, top_k=200, alpha_merge="max")) == _bits(fresh.search(one, top_k=200, alpha_merge="max")) \
                == _bits(want)
        with pytest.raises(MragError) as e:
            used.search(queries + ["w1"], top_k=200, alpha_merge="max")
        assert e.value.code == -5 and len(queries) + 1 == tc.BM25_MAX_QUERIES + 1            # MRAG_ERR_UNSUPPORTED
        assert _bits(used.search(["w1"], top_k=5, alpha_merge="max")) == _bits(ob.search_postings(p, ["w1"], 5, "max"))
    finally:
        used.close(); fresh.close()


# ------------------------------------------------------------------------------------------------ fusion
def _alphas(case):
    return dict(zip(("alpha_text", "alpha_graph", "alpha_dense"), case.alphas))


@pytest.mark.parametrize("case", tc.FUSION_CASES, ids=lambda c: c.name)
def test_fusion_on_device_equals_host_fusion(case):
    from mrag_amd import fusion
    text, graph, dense = case.make()
    for top_k in case.top_ks:
        host = fusion.fuse_channels(text, graph, dense, top_k=top_k, **_alphas(case))
        dev = fusion.fuse_channels_device(text, graph, dense, top_k=top_k, **_alphas(case))
        assert len(host) > 0 and dev == host, (case.name, top_k)           # ids, scores, norms and meta, in order


def test_fusion_refuses_4097_entries_and_nan():
    from mrag_amd import fusion
    from mrag_amd._native import MragError
    case = next(c for c in tc.FUSION_CASES if c.name == "exactly-4096")
    text, graph, dense = tc.fusion_4097()
    assert tc.fusion_entries((text, graph, dense)) == tc.FUSE_MAX + 1
    with pytest.raises(MragError) as e:
        fusion.fuse_channels_device(text, graph, dense, top_k=7, **_alphas(case))
    assert e.value.code == -5
    text, graph, dense = tc.fusion_3000()
    for where in (0, 1399):
        bad = [dict(h) for h in text]
        bad[where]["score"] = float("nan")
        with pytest.raises(MragError):
            fusion.fuse_channels_device(bad, graph, dense, top_k=7, **_alphas(case))
    with pytest.raises(MragError):
        fusion.fuse_channels_device(text, graph, dict(dense, **{next(iter(dense)): float("nan")}), top_k=7, **_alphas(case))


def test_the_single_question_entry_points_refuse_on_their_own():
    """``mrag_bm25_search`` and ``mrag_fuse_topk`` through ctypes: the Python classes reach the device through the batch
    entry points, so the checks the single-question entry points make before the shared path are asked here -- status,
    message, ``*out_n = 0``, no output slot written, and the next good call served."""
    from mrag_amd import _native as N
    lib = N.load()
    case = next(c for c in tc.BM25_CASES if c.via == "abi")
    p = _postings(case)
    n_terms = len(p["indptr"]) - 1
    ix = _AbiIndex(p, case.k1)
    n = C.c_int(9)
    try:
        docs, scores = np.full(4, 7, dtype=np.int64), np.full(4, 7.0)

        def search(nq, q_ptr, terms, k=4):
            qp, qt = np.asarray(q_ptr, dtype=np.int32), np.asarray(terms or [0], dtype=np.int32)
            qi = np.ones(len(qt))
            return lib.mrag_bm25_search(ix.h, nq, qp.ctypes.data, qt.ctypes.data, qi.ctypes.data, 0, k, docs.ctypes.data,
                                        scores.ctypes.data, C.byref(n), None)

        for want, word, args in ((-5, "exceeds", (1, [0, 1], [0], 4096 + 1)),
                                 (-5, "queries", (tc.BM25_MAX_QUERIES + 1, [0] * (tc.BM25_MAX_QUERIES + 2), [])),
                                 (-1, "monotone", (2, [0, 1, 0], [0])),
                                 (-1, "vocabulary", (1, [0, 1], [n_terms]))):
            n.value = 9
            st = search(*args)
            assert st == want and word in lib.mrag_last_error().decode(), (st, word, lib.mrag_last_error())
            assert n.value == 0 and (docs == 7).all() and (scores == 7.0).all()
        assert search(1, [0, 1], [0]) == 0 and 0 <= n.value <= 4
    finally:
        ix.close()

    keys, zeros = np.zeros(tc.FUSE_MAX + 1, dtype=np.int32), np.zeros(tc.FUSE_MAX + 1)
    nan_at_9 = np.zeros(10)
    nan_at_9[9] = np.nan
    ok, vals = np.full(4, 7, dtype=np.int32), [np.full(4, 7.0) for _ in range(4)]

    def fuse(sizes, sc):
        return lib.mrag_fuse_topk(0, keys.ctypes.data, sc.ctypes.data, *sizes, 0.4, 0.2, 0.4, 4, ok.ctypes.data,
                                  *[v.ctypes.data for v in vals], C.byref(n), None)

    for want, word, sizes, sc in ((-5, "exceed", (tc.FUSE_MAX + 1, 0, 0), zeros), (-5, "exceed", (2000, 97, 2000), zeros),
                                  (-1, "negative", (3, -1, 3), zeros), (-1, "entry 9", (3, 3, 4), nan_at_9)):
        n.value = 9
        st = fuse(sizes, sc)
        assert st == want and word in lib.mrag_last_error().decode(), (st, word, lib.mrag_last_error())
        assert n.value == 0 and (ok == 7).all() and all((v == 7.0).all() for v in vals)
    assert fuse((3, 3, 3), nan_at_9) == 0 and n.value == 1 and ok[0] == 0 and (ok[1:] == -1).all()   # one key, nine entries


# ------------------------------------------------------------------------------------------------ cosine
@pytest.mark.parametrize("dim", tc.COSINE_F64_DIM)
def test_cosine_f64_against_the_exact_value(dim):
    from mrag_amd.index import cosine_f64
    q = tc.cosine_vectors(1, dim, 40)[0]
    for n in tc.COSINE_F64_N:
        zero = (0, n - 1) if n >= 3 else ()
        x = tc.cosine_vectors(n, dim, 41, zero_rows=zero)
        got = cosine_f64(q, x)
        err = tc.max_error(got, tc.exact_cosine(q, x))
        print(f"cosine_f64 n {n} dim {dim}: max error {err:.3e}, bound {COSINE_BOUND(dim):.3e}")
        assert got.shape == (n,) and err <= COSINE_BOUND(dim)
        assert all(got[r] == 0.0 and not np.signbit(got[r]) for r in zero)
        assert (np.abs(got[[r for r in range(n) if r not in zero]]) > 0).all()
        assert (cosine_f64(np.zeros(dim), x) == 0.0).all()


@pytest.mark.parametrize("dim", tc.COSINE_MATRIX_DIM)
def test_cosine_matrix_against_the_exact_value(dim):
    from mrag_amd.pairwise import cosine_matrix
    for n in tc.COSINE_MATRIX_N:
        x = tc.cosine_vectors(n, dim, 42, zero_rows=(1,) if n >= 3 else ())
        got = cosine_matrix(x)
        err = tc.max_error(got, tc.exact_matrix(x))
        print(f"cosine_matrix n {n} dim {dim}: max error {err:.3e}, bound {COSINE_BOUND(dim):.3e}")
        assert got.shape == (n, n) and err <= COSINE_BOUND(dim)
        assert np.array_equal(got.view(np.uint64), got.T.view(np.uint64))               # out[i, j] bit-equal to out[j, i]
        if n >= 3:
            assert (got[1] == 0.0).all() and (got[:, 1] == 0.0).all() and got[1, 1] == 0.0


def test_cosine_matrix_refuses_more_than_32768_rows():
    from mrag_amd import _native as N
    x, out = np.zeros((32769, 1)), np.zeros(4)
    with pytest.raises(N.MragError):                    # refused on the sizes alone: nothing is read or written
        N.check(N.load().mrag_cosine_matrix_f64(0, x.ctypes.data, 32769, 1, out.ctypes.data, 0, None))
    assert (out == 0).all()


def test_cosine_kernels_on_device_pointers():
    """``is_device = 1`` of ``mrag_cosine_f64`` and ``mrag_cosine_matrix_f64``: inputs and output already on the device."""
    import torch
    from mrag_amd import _native as N
    from mrag_amd.index import cosine_f64
    from mrag_amd.pairwise import cosine_matrix
    lib = N.load()
    for n, dim in ((5, 65), (1, 7), (201, 64), (7, 768)):
        q, x = tc.cosine_vectors(1, dim, 43)[0], tc.cosine_vectors(n, dim, 44, zero_rows=(n - 1,) if n > 2 else ())
        dq, dx = torch.from_numpy(q).cuda(), torch.from_numpy(x).cuda()
        out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        N.check(lib.mrag_cosine_f64(0, dq.data_ptr(), dx.data_ptr(), n, dim, out.data_ptr(), 1, None))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert not np.isnan(got).any() and np.array_equal(got.view(np.uint64), cosine_f64(q, x).view(np.uint64))
        mat = torch.full((n, n), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        N.check(lib.mrag_cosine_matrix_f64(0, dx.data_ptr(), n, dim, mat.data_ptr(), 1, None))
        torch.cuda.synchronize()
        got = mat.cpu().numpy()
        assert not np.isnan(got).any() and np.array_equal(got.view(np.uint64), cosine_matrix(x).view(np.uint64))


@pytest.mark.parametrize("dim", tc.COSINE_ADJ_DIM)
def test_cosine_adjacent_against_the_exact_value(dim):
    from mrag_amd.pairwise import cosine_adjacent
    for n in tc.COSINE_ADJ_N:
        x = tc.cosine_vectors(n, dim, 45, zero_rows=(2,) if n >= 5 else ())
        for eps in (1e-9, 0.5):
            got = cosine_adjacent(x, eps)
            assert got.shape == (max(0, n - 1),)
            err = tc.max_error(got, tc.exact_adjacent(x, eps))
            print(f"cosine_adjacent n {n} dim {dim} eps {eps}: max error {err:.3e}, bound {COSINE_BOUND(dim):.3e}")
            assert err <= COSINE_BOUND(dim)
            if n >= 5:
                assert got[1] == 0.0 and got[2] == 0.0                   # 0 / (0 + eps) on both sides of the zero row
        if n >= 2:
            assert (np.abs(cosine_adjacent(x, 0.5)) < np.abs(cosine_adjacent(x, 1e-9)))[[i for i in range(n - 1) if n < 5 or i not in (1, 2)]].all()


def test_semantic_edges_equal_the_exact_edge_list():
    from mrag_amd.pairwise import semantic_edges
    n, dim, threshold = 45, 64, 0.9
    v = tc.clustered_vectors(n, dim, 9)
    m = tc.exact_matrix(v)
    pairs = list(itertools.combinations(range(n), 2))
    assert min(abs(float(m[i][j]) - threshold) for i, j in pairs) >= 1e-9          # ``>=`` cannot flip legitimately
    want = [(i, j) for i, j in pairs if m[i][j] >= threshold]
    edges = semantic_edges(v, threshold)
    assert [(i, j) for i, j, _ in edges] == want and len(want) > 20
    assert tc.max_error([s for _, _, s in edges], [m[i][j] for i, j in want]) <= COSINE_BOUND(dim)
