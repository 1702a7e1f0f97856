"""GPU tests of the fp8 scan copy + exact re-rank (DenseIndex(fp8_scan=True), search(precision="fp8"),
mrag_index_search_fp8): the e4m3fn copy bit for bit against torch's float8_e4m3fn, exact results when the candidate
pool covers the corpus, the fp8 candidate kernels against a host simulation of the fp8 scores (fragment layout of the
block-scaled MFMA), recall on the clustered set in both regimes, exact scores, device use, errors, the unchanged exact
search and the sharded path."""
import os

import numpy as np
import pytest

from oracle import dense_search as ds

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _torch():
    import torch
    return torch


def _index(c16, dtype="f16", id_base=0, fp8=True, **kw):
    from mrag_amd.index import DenseIndex
    ix = DenseIndex(c16.shape[1], dtype=dtype, fp8_scan=fp8, **kw)
    if id_base:
        ix.set_id_base(id_base)
    ix.add(c16, normalize=False)
    return ix


def _ref_fp8(stored):
    """torch's e4m3fn (round to nearest even) of clip(256 x, +-448), as bytes."""
    torch = _torch()
    x = np.clip(np.asarray(stored, dtype=np.float32) * np.float32(256.0), -448.0, 448.0)
    return torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def _fp8_values(b):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(b)).view(torch.float8_e4m3fn).to(torch.float64).numpy()


def _bf16(x):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)


def _round(x, dtype):
    """normalised rows rounded to the storage dtype, as what DenseIndex.add(normalize=False) stores."""
    if dtype == "f16":
        return ds.normalize_round(x)
    return _bf16(ds.l2_normalize(x))


def _f64(rows):
    torch = _torch()
    if hasattr(rows, "dtype") and str(rows.dtype) == "torch.bfloat16":
        return rows.to(torch.float64).numpy()
    return np.asarray(rows, dtype=np.float64)


# ---------------------------------------------------------------------------------------------- 1. quantizer
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("dim", [100, 384, 768])
def test_fp8_copy_bit_for_bit(dtype, dim):
    from mrag_amd.index import DenseIndex
    rng = np.random.default_rng(dim)
    parts = [rng.standard_normal((n, dim)).astype(np.float32) for n in (3, 250, 300, 700)]
    parts[1][[0, 17, 249]] = 0.0                                   # zero rows
    raw = (rng.standard_normal((40, dim)) * 2.5).astype(np.float32)  # not normalised: |256 x| > 448 saturates
    raw[0, :5] = [1e-7, -3e-6, 2 ** -16, -(2 ** -10), 1.75]          # fp8 subnormals / underflow / exact values
    before = DenseIndex(dim, dtype=dtype, fp8_scan=True)
    after = DenseIndex(dim, dtype=dtype)
    for ix in (before, after):
        for p in parts:                                           # several adds across capacity growth (256 -> 384 -> ...)
            ix.add(p if dtype == "f16" else _bf16(p), normalize=True)
        ix.add(raw if dtype == "f16" else _bf16(raw), normalize=False)
    after.enable_fp8()
    n = len(before)
    assert n == len(after) == sum(len(p) for p in parts) + len(raw)
    want = _ref_fp8(before.rows())
    got_b, got_a = before.rows_fp8(), after.rows_fp8()
    assert got_b.shape == (n, dim) and got_b.dtype == np.uint8
    assert np.array_equal(got_b, want), int((got_b != want).sum())
    assert np.array_equal(got_a, got_b)
    assert (got_b[3 + 17] == 0).all()
    assert np.array_equal(before.rows_fp8(5, 7), want[5:12])
    # add_stored_bits goes through add: the copy follows
    bits = before.stored_bits()[:37]
    before.add_stored_bits(bits)
    assert np.array_equal(before.rows_fp8(n, 37), want[:37])
    before.enable_fp8()                                           # idempotent
    assert np.array_equal(before.rows_fp8(0, n), want)
    # reserve keeps the copy
    before.reserve(5000)
    assert np.array_equal(before.rows_fp8(0, n), want)


# ---------------------------------------------------------------------------------------------- 2. pool covers the corpus
@pytest.mark.parametrize("n", [50, 64])
@pytest.mark.parametrize("nq", [5, 40])                      # streaming (<= 16 queries) / batch
@pytest.mark.parametrize("k", [10, 64])                      # n < k = 64: the (-inf, -1) tail
def test_fp8_exact_when_pool_covers_corpus(n, nq, k):
    d = 384
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 100 + n))
    q16 = ds.normalize_round(ds.make_gaussian(nq, d, 200 + nq))
    base = 1000
    ix = _index(c16, id_base=base)
    sc, ids = ix.search(q16, k, normalize=False, precision="fp8", refine=64)
    assert ix.last_fp8() == {"refine": 64, "regime": "stream" if nq <= 16 else "batch"}
    rv, ri = ds.brute_force_topk(q16, c16, k)
    valid = ri >= 0
    assert ((ids >= 0) == valid).all()
    assert np.isneginf(sc[~valid]).all() and (ids[~valid] == -1).all()
    np.testing.assert_allclose(sc[valid], rv[valid], rtol=0, atol=TOL)
    _, bad = ds.gap_aware_id_match(ids - np.where(ids >= 0, base, 0), sc, ri, rv, tol=TOL)
    assert bad == 0


# ---------------------------------------------------------------------------------------------- candidate kernels
def _sim_fp8_scores(q16, rows8):
    """fp64 scores of the quantised queries against the fp8 copy, as the candidate kernels define them."""
    q = np.asarray(q16, dtype=np.float32)
    amax = np.abs(q).max(axis=1)
    _, ex = np.frexp(amax)
    scale = np.where(amax > 0, np.ldexp(1.0, 8 - ex), 1.0).astype(np.float32)
    q8 = _fp8_values(_torch().from_numpy(q * scale[:, None]).to(_torch().float8_e4m3fn).view(_torch().uint8).numpy())
    return q8 @ _fp8_values(rows8).T


@pytest.mark.parametrize("nq", [7, 300])                     # streaming / batch
@pytest.mark.parametrize("d", [256, 200])
def test_fp8_candidates_match_simulated_fp8_ranking(nq, d):
    n, k = 3000, 10
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 7 + d))
    q16 = ds.normalize_round(ds.make_gaussian(nq, d, 8 + d))
    ix = _index(c16)
    _, ids = ix.search(q16, k, normalize=False, precision="fp8", refine=k)   # refine = k: the candidate set itself
    s8 = _sim_fp8_scores(q16, ix.rows_fp8())
    kth = np.sort(s8, axis=1)[:, -k]
    got = np.take_along_axis(s8, ids, axis=1)
    tol = 1e-5 * np.abs(s8).max()
    assert (got >= kth[:, None] - tol).all(), float((kth[:, None] - got).max())
    ref = np.argsort(-s8, axis=1, kind="stable")[:, :k]
    assert ds.recall_at_k(ids, ref) >= 0.99


# ---------------------------------------------------------------------------------------------- 3. recall
@pytest.fixture(scope="module")
def clustered():
    torch = _torch()
    c32, q32 = ds.make_clustered(200_000, 16_385, 768, 7)
    c16, q16 = ds.normalize_round(c32), ds.normalize_round(q32)
    ix = _index(c16)
    return ix, c16, q16, torch.from_numpy(c16).cuda().double()


def _oracle_ids(cd, q16, k):
    """exact fp64 top-k on the GPU (torch), rows ascending among equal scores"""
    torch = _torch()
    out = []
    for lo in range(0, q16.shape[0], 2048):
        s = torch.from_numpy(q16[lo:lo + 2048]).cuda().double() @ cd.T
        out.append(torch.topk(s, k, dim=1, sorted=True).indices.cpu().numpy())
    return np.concatenate(out)


@pytest.mark.parametrize("nq", [1, 16, 17, 1000, 16_385])
def test_fp8_recall_k10(clustered, nq):
    ix, c16, q16, cd = clustered
    q = q16[:nq]
    sc, ids = ix.search(q, 10, normalize=False, precision="fp8")
    assert ix.last_fp8() == {"refine": 40, "regime": "stream" if nq <= 16 else "batch"}
    ref = _oracle_ids(cd, q, 10)
    r = ds.recall_at_k(ids, ref)
    assert r >= 0.995, r


@pytest.mark.parametrize("nq", [8, 1000])
def test_fp8_recall_k64(clustered, nq):
    ix, c16, q16, cd = clustered
    q = q16[-nq:]
    _, ids = ix.search(q, 64, normalize=False, precision="fp8", refine=64)
    r = ds.recall_at_k(ids, _oracle_ids(cd, q, 64))
    assert r >= 0.95, r


# ---------------------------------------------------------------------------------------------- 4. exact scores
@pytest.mark.parametrize("nq", [3, 500])
def test_fp8_scores_are_exact(clustered, nq):
    ix, c16, q16, _ = clustered
    q = q16[100:100 + nq]
    sc, ids = ix.search(q, 10, normalize=False, precision="fp8")
    assert (ids >= 0).all()
    exact = np.einsum("ij,ikj->ik", q.astype(np.float64), c16[ids].astype(np.float64))
    np.testing.assert_allclose(sc, exact, rtol=0, atol=TOL)
    assert (np.diff(sc, axis=1) <= 0).all()
    tie = np.diff(sc, axis=1) == 0
    assert (np.diff(ids, axis=1)[tie] > 0).all()                 # equal scores: rows ascending


# ---------------------------------------------------------------------------------------------- 5. device use
def test_fp8_device_tensors_on_a_side_stream():
    torch = _torch()
    n, d, k = 20_000, 384, 10
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 11))
    q16 = ds.normalize_round(ds.make_gaussian(300, d, 12))
    ix = _index(c16)
    for nq in (4, 300):
        hs, hi = ix.search(q16[:nq], k, normalize=False, precision="fp8")
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            qd = torch.from_numpy(q16[:nq]).cuda()
            out = (torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"))
            ds_, di = ix.search(qd, k, normalize=False, stream=s, out=out, precision="fp8")
        s.synchronize()
        assert ds_ is out[0] and di is out[1]
        assert np.array_equal(di.cpu().numpy(), hi) and np.array_equal(ds_.cpu().numpy(), hs)
        g, t = ix.last_timing_ms()
        assert 0 < g <= t


# ---------------------------------------------------------------------------------------------- 6. errors
def test_fp8_errors():
    from mrag_amd import _native as N
    from mrag_amd.index import DenseIndex
    c16 = ds.normalize_round(ds.make_gaussian(500, 64, 3))
    q16 = c16[:4]
    ip = DenseIndex(64, metric="ip")
    with pytest.raises(N.MragError):
        ip.enable_fp8()
    plain = _index(c16, fp8=False)
    with pytest.raises(N.MragError):
        plain.search(q16, 10, normalize=False, precision="fp8")
    with pytest.raises(N.MragError):
        plain.rows_fp8(0, 1)
    with pytest.raises(N.MragError):
        plain.last_fp8()
    ix = _index(c16)
    with pytest.raises(N.MragError):
        ix.search(q16, 65, normalize=False, precision="fp8")
    with pytest.raises(N.MragError):
        ix.search(q16, 10, normalize=False, precision="fp8", refine=9)
    with pytest.raises(N.MragError):
        ix.search(q16, 10, normalize=False, precision="fp8", refine=65)
    with pytest.raises(ValueError):
        ix.search(q16, 10, normalize=False, precision="fp8", allow=np.ones(500, dtype=bool))


# ---------------------------------------------------------------------------------------------- 7. exact search unchanged
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_exact_search_bit_identical_with_fp8_copy(dtype):
    n, d = 30_000, 384
    c = _round(ds.make_gaussian(n, d, 21), dtype)
    q = _round(ds.make_gaussian(400, d, 22), dtype)
    a, b = _index(c, dtype=dtype, fp8=False), _index(c, dtype=dtype, fp8=True)
    b.search(q, 10, normalize=False, precision="fp8")            # an fp8 search in between must not disturb the next exact one
    for nq, k in ((1, 10), (16, 10), (400, 10), (400, 64), (5, 200)):
        sa, ia = a.search(q[:nq], k, normalize=False)
        sb, ib = b.search(q[:nq], k, normalize=False)
        assert np.array_equal(ia, ib) and np.array_equal(sa, sb), (nq, k)


# ---------------------------------------------------------------------------------------------- 8. sharded
def test_sharded_world1_fp8_matches_local():
    torch = _torch()
    import torch.distributed as dist
    from mrag_amd.sharded import ShardedDenseIndex
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29631")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        n, d, k = 40_000, 256, 10
        c16 = ds.normalize_round(ds.make_gaussian(n, d, 41))
        q16 = ds.normalize_round(ds.make_gaussian(300, d, 42))
        sh = ShardedDenseIndex(d, n, rank=0, world=1, device=0, fp8_scan=True)
        sh.add_local(c16, normalize=False)
        for nq in (3, 300):
            ls, li = sh.index.search(q16[:nq], k, normalize=False, precision="fp8")
            ss, si = sh.search(q16[:nq], k, force_collective=True, normalize=False, precision="fp8")
            ss, si = np.asarray(ss), np.asarray(si)
            assert np.array_equal(si, li) and np.array_equal(ss, ls), nq
            assert sh.index.last_fp8()["regime"] == ("stream" if nq <= 16 else "batch")
    finally:
        if created:
            dist.destroy_process_group()
