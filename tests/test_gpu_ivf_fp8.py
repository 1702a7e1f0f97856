"""GPU tests of the IVF fp8 scan copy + exact re-rank (IVFFlatIndex(fp8_scan=True), search(precision="fp8"),
mrag_ivf_search_fp8): the e4m3fn copy of the regrouped rows bit for bit against torch's float8_e4m3fn, the exact search's
answer when the candidate pool covers the probed rows, the fp8 scan instance against a host simulation of the fp8 scores,
recall against the index's own exact search, exact scores, device use, errors and refusals, the undisturbed exact paths
and the sharded path."""
import os
import subprocess
import sys
import tempfile
import textwrap

import numpy as np
import pytest

from oracle import dense_search as ds

pytestmark = pytest.mark.gpu
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch():
    import torch
    return torch


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _ivf(c, cen, id_base=0, fp8=True, **kw):
    from mrag_amd.index import IVFFlatIndex
    ix = IVFFlatIndex(c.shape[1], cen.shape[0], fp8_scan=fp8, **kw)
    ix.set_centroids(cen, normalize=False)
    if id_base:
        ix.set_id_base(id_base)
    ix.add(c, normalize=False)
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
    """normalised rows rounded to the storage dtype: what add(normalize=False) stores bit for bit"""
    return ds.normalize_round(x) if dtype == "f16" else _bf16(ds.l2_normalize(x))


def _store(x, dtype):
    """rows rounded to the storage dtype WITHOUT normalising"""
    return np.asarray(x, dtype=np.float16) if dtype == "f16" else _bf16(x)


def _f32(rows):
    return rows.float().numpy() if hasattr(rows, "float") else np.asarray(rows, dtype=np.float32)


def _f64(rows):
    return _f32(rows).astype(np.float64)


def _sim_fp8_scores(q16, rows8):
    """fp64 scores of the quantised queries against the fp8 copy, as the scan defines them."""
    q = _f32(q16)
    amax = np.abs(q).max(axis=1)
    _, ex = np.frexp(amax)
    scale = np.where(amax > 0, np.ldexp(1.0, 8 - ex), 1.0).astype(np.float32)
    q8 = _fp8_values(_torch().from_numpy(q * scale[:, None]).to(_torch().float8_e4m3fn).view(_torch().uint8).numpy())
    return q8 @ _fp8_values(rows8).T


# ---------------------------------------------------------------------------------------------- 1. the copy
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("dim", [100, 384, 768])
def test_ivf_fp8_copy_bit_for_bit(dtype, dim):
    from mrag_amd.index import IVFFlatIndex
    rng = np.random.default_rng(dim)
    parts = [rng.standard_normal((n, dim)).astype(np.float32) for n in (3, 250, 300, 700)]
    parts[1][[0, 17, 249]] = 0.0                                   # zero rows
    raw = (rng.standard_normal((40, dim)) * 2.5).astype(np.float32)  # not normalised: |256 x| > 448 saturates
    raw[0, :5] = [1e-7, -3e-6, 2 ** -16, -(2 ** -10), 1.75]          # fp8 subnormals / underflow / exact values
    stored = [_round(p, dtype) for p in parts] + [_store(raw, dtype)]
    more = _round(rng.standard_normal((333, dim)).astype(np.float32), dtype)
    cen = ds.normalize_round(rng.standard_normal((8, dim)).astype(np.float32))
    q = ds.normalize_round(rng.standard_normal((5, dim)).astype(np.float32))
    before = IVFFlatIndex(dim, 8, dtype=dtype, fp8_scan=True)      # enabled at construction
    after = IVFFlatIndex(dim, 8, dtype=dtype)                      # enabled after the adds, before any regroup
    late = IVFFlatIndex(dim, 8, dtype=dtype)                       # enabled after a search has regrouped the rows
    for ix in (before, after, late):
        ix.set_centroids(cen, normalize=False)
        for p in stored:                                           # several adds across capacity growth (256 -> 512 -> ...)
            ix.add(p, normalize=False)
    late.search(q, 3, 2)
    after.enable_fp8()
    late.enable_fp8()
    n = len(before)
    assert n == len(after) == len(late) == sum(len(p) for p in parts) + len(raw)
    want = _ref_fp8(np.concatenate([_f32(p) for p in stored]))
    got = before.rows_fp8()
    assert got.shape == (n, dim) and got.dtype == np.uint8
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(after.rows_fp8(), got) and np.array_equal(late.rows_fp8(), got)
    assert (got[3 + 17] == 0).all()
    assert (want[n - 40:] == 0x7E).any() or (want[n - 40:] == 0xFE).any()      # the set does saturate at +-448
    assert np.array_equal(before.rows_fp8(5, 7), want[5:12])
    # a search, more rows, another search: the copy is current after the regroup
    before.search(q, 3, 2, precision="fp8")
    before.add(more, normalize=False)
    assert np.array_equal(before.rows_fp8(n, len(more)), _ref_fp8(_f32(more)))   # (regroups by itself)
    before.search(q, 3, 2, precision="fp8")
    want2 = np.concatenate([want, _ref_fp8(_f32(more))])
    assert np.array_equal(before.rows_fp8(), want2)
    before.enable_fp8()                                            # idempotent
    before.enable_fp8()
    assert np.array_equal(before.rows_fp8(), want2)


# ---------------------------------------------------------------------------------------------- 2. pool covers the candidates
@pytest.mark.parametrize("n", [50, 64])
@pytest.mark.parametrize("nq", [5, 40])
@pytest.mark.parametrize("k", [10, 64])                      # n < k = 64: the (-inf, -1) tail
def test_ivf_fp8_equals_exact_when_pool_covers_probed_rows(n, nq, k):
    d, nlist, base = 384, 4, 1000
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 100 + n))
    q16 = ds.normalize_round(ds.make_gaussian(nq, d, 200 + nq))
    cen = ds.normalize_round(ds.make_gaussian(nlist, d, 300))
    ix = _ivf(c16, cen, id_base=base)
    sc, ids = ix.search(q16, k, nlist, normalize=False, precision="fp8", refine=64)
    assert ix.last_fp8() == {"refine": 64}
    es, ei = ix.search(q16, k, nlist, normalize=False)
    valid = ei >= 0
    assert valid.sum() == nq * min(n, k)
    assert ((ids >= 0) == valid).all()
    assert np.isneginf(sc[~valid]).all() and (ids[~valid] == -1).all()
    np.testing.assert_allclose(sc[valid], es[valid], rtol=0, atol=TOL)
    _, bad = ds.gap_aware_id_match(ids, sc, ei, es, tol=TOL)
    assert bad == 0
    assert (ids[valid] >= base).all() and (ids[valid] < base + n).all()


# ---------------------------------------------------------------------------------------------- 3. the fp8 scan instance
@pytest.mark.parametrize("nq", [7, 300])
@pytest.mark.parametrize("d", [256, 200])
def test_ivf_fp8_candidates_match_simulated_fp8_ranking(nq, d):
    n, k, nlist = 3000, 10, 16
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 7 + d))
    q16 = ds.normalize_round(ds.make_gaussian(nq, d, 8 + d))
    cen = ds.kmeans_spherical(c16, nlist, 2, seed=5)
    ix = _ivf(c16, cen)
    _, ids = ix.search(q16, k, nlist, normalize=False, precision="fp8", refine=k)   # every list, refine = k: the candidate set itself
    assert (ids >= 0).all()
    s8 = _sim_fp8_scores(q16, ix.rows_fp8())
    kth = np.sort(s8, axis=1)[:, -k]
    got = np.take_along_axis(s8, ids, axis=1)
    tol = 1e-5 * np.abs(s8).max()
    assert (got >= kth[:, None] - tol).all(), float((kth[:, None] - got).max())
    ref = np.argsort(-s8, axis=1, kind="stable")[:, :k]
    assert ds.recall_at_k(ids, ref) >= 0.99


@pytest.mark.parametrize("nq", [7, 300])
@pytest.mark.parametrize("nprobe", [1, 3])
def test_ivf_fp8_returns_rows_of_the_probed_lists_only(nq, nprobe):
    n, d, k, nlist = 3000, 256, 10, 16
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 61))
    q16 = ds.normalize_round(ds.make_gaussian(nq, d, 62))
    cen = ds.kmeans_spherical(c16, nlist, 2, seed=6)
    ix = _ivf(c16, cen)
    sc, ids = ix.search(q16, k, nprobe, normalize=False, precision="fp8")
    assign = ix.assignments().astype(np.int64)
    cs = _f64(q16) @ _f64(cen).T
    nth = -np.sort(-cs, axis=1)[:, nprobe - 1]
    found = ids >= 0
    assert found[:, 0].all()
    lists = assign[np.where(found, ids, 0)]
    reach = np.take_along_axis(cs, lists, axis=1) >= nth[:, None] - TOL
    assert (reach | ~found).all()
    # and it is the exact search over those lists wherever the pool (40) covers them or not: same probes, exact scores
    es, ei = ix.search(q16, k, nprobe, normalize=False)
    assert ((ei >= 0) == found).all()
    exact = np.einsum("ij,ikj->ik", _f64(q16), _f64(c16)[np.where(found, ids, 0)])
    np.testing.assert_allclose(sc[found], exact[found], rtol=0, atol=TOL)


# ---------------------------------------------------------------------------------------------- 4. recall
@pytest.fixture(scope="module")
def clustered():
    n, nlist = 200_000, 1024
    c32, q32 = ds.make_clustered(n, 1000, 768, 7)
    c16, q16 = ds.normalize_round(c32), ds.normalize_round(q32)
    cen = c16[np.random.default_rng(3).choice(n, nlist, replace=False)]
    return _ivf(c16, cen), c16, q16


@pytest.mark.parametrize("nq", [1, 17, 1000])
@pytest.mark.parametrize("nprobe", [1, 8, 32])
def test_ivf_fp8_recall_k10_against_own_exact_search(clustered, nprobe, nq):
    ix, c16, q16 = clustered
    q = q16[:nq]
    _, ids = ix.search(q, 10, nprobe, normalize=False, precision="fp8")
    assert ix.last_fp8() == {"refine": 40}
    _, ref = ix.search(q, 10, nprobe, normalize=False)
    r = ds.recall_at_k(ids, ref)
    print(f"recall@10 nprobe {nprobe} nq {nq}: {r:.5f}")
    assert r >= 0.995, r


@pytest.mark.parametrize("nq", [1, 17, 1000])
@pytest.mark.parametrize("nprobe", [1, 8, 32])
def test_ivf_fp8_recall_k64_against_own_exact_search(clustered, nprobe, nq):
    ix, c16, q16 = clustered
    q = q16[-nq:]
    _, ids = ix.search(q, 64, nprobe, normalize=False, precision="fp8", refine=64)
    assert ix.last_fp8() == {"refine": 64}
    _, ref = ix.search(q, 64, nprobe, normalize=False)
    r = ds.recall_at_k(ids, ref)
    print(f"recall@64 nprobe {nprobe} nq {nq}: {r:.5f}")
    assert r >= 0.95, r


# ---------------------------------------------------------------------------------------------- 5. exact scores
@pytest.mark.parametrize("nq", [3, 500])
def test_ivf_fp8_scores_are_exact(clustered, nq):
    ix, c16, q16 = clustered
    q = q16[100:100 + nq]
    sc, ids = ix.search(q, 10, 8, normalize=False, precision="fp8")
    assert (ids >= 0).all()
    exact = np.einsum("ij,ikj->ik", q.astype(np.float64), c16[ids].astype(np.float64))
    np.testing.assert_allclose(sc, exact, rtol=0, atol=TOL)
    assert (np.diff(sc, axis=1) <= 0).all()
    tie = np.diff(sc, axis=1) == 0
    assert (np.diff(ids, axis=1)[tie] > 0).all()                 # equal scores: rows ascending


# ---------------------------------------------------------------------------------------------- 6. device use
def test_ivf_fp8_device_tensors_on_a_side_stream():
    torch = _torch()
    n, d, k, nlist, nprobe = 20_000, 384, 10, 64, 8
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 11))
    q16 = ds.normalize_round(ds.make_gaussian(300, d, 12))
    ix = _ivf(c16, ds.kmeans_spherical(c16, nlist, 2, seed=2))
    for nq in (4, 300):
        hs, hi = ix.search(q16[:nq], k, nprobe, normalize=False, precision="fp8")
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            qd = torch.from_numpy(q16[:nq]).cuda()
            out = (torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"))
            ds_, di = ix.search(qd, k, nprobe, normalize=False, stream=s, out=out, precision="fp8")
        s.synchronize()
        assert ds_ is out[0] and di is out[1]
        assert np.array_equal(di.cpu().numpy(), hi) and np.array_equal(ds_.cpu().numpy(), hs)
        t = ix.last_timing()
        assert 0 < t["scan_ms"] <= t["total_ms"]


# ---------------------------------------------------------------------------------------------- 7. errors and refusals
def test_ivf_fp8_errors():
    from mrag_amd import _native as N
    from mrag_amd.index import IVFFlatIndex
    c16 = ds.normalize_round(ds.make_gaussian(500, 64, 3))
    cen = ds.normalize_round(ds.make_gaussian(4, 64, 4))
    q16 = c16[:4]
    ip = IVFFlatIndex(64, 4, metric="ip")
    with pytest.raises(N.MragError) as e:
        ip.enable_fp8()
    assert e.value.code == -1
    plain = _ivf(c16, cen, fp8=False)
    with pytest.raises(N.MragError):
        plain.search(q16, 10, 2, normalize=False, precision="fp8")
    with pytest.raises(N.MragError):
        plain.rows_fp8(0, 1)
    with pytest.raises(N.MragError):
        plain.last_fp8()
    ix = _ivf(c16, cen)
    with pytest.raises(N.MragError):
        ix.last_fp8()                                            # no fp8 search yet
    for kw in (dict(k=65), dict(k=10, refine=9), dict(k=10, refine=65)):
        with pytest.raises(N.MragError) as e:
            ix.search(q16, kw.pop("k"), 2, normalize=False, precision="fp8", **kw)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        ix.search(q16, 10, 2, normalize=False, precision="fp8", allow=np.ones(500, dtype=bool))
    with pytest.raises(N.MragError):
        ix.rows_fp8(400, 101)


_CHILD = textwrap.dedent('''
    import sys, numpy as np, torch
    sys.path.insert(0, ".")
    from oracle import dense_search as ds
    from mrag_amd.index import IVFFlatIndex
    from mrag_amd._native import MragError
    c16 = ds.normalize_round(ds.make_gaussian(5000, 128, 31)); q16 = ds.normalize_round(ds.make_gaussian(50, 128, 32))
    cen = ds.kmeans_spherical(c16, 16, 2, seed=4)
    ix = IVFFlatIndex(128, 16, fp8_scan=True); ix.set_centroids(cen, normalize=False); ix.add(c16, normalize=False)
    qd = torch.from_numpy(q16).cuda()
    out = (torch.full((50, 10), 7.0, dtype=torch.float32, device="cuda"), torch.full((50, 10), -7, dtype=torch.int64, device="cuda"))
    s0, i0 = ix.search(q16, 10, 4, normalize=False)              # the exact search still runs (fused regime when the buffer is off)
    try:
        ix.search(qd, 10, 4, normalize=False, precision="fp8", out=out)
        torch.cuda.synchronize()
        np.savez(sys.argv[1], code=0, sc=out[0].cpu().numpy(), ids=out[1].cpu().numpy(), s0=s0, i0=i0)
    except MragError as e:
        torch.cuda.synchronize()
        np.savez(sys.argv[1], code=e.code, msg=str(e), sc=out[0].cpu().numpy(), ids=out[1].cpu().numpy(), s0=s0, i0=i0)
''')


def _run_child(td, name, env):
    path = os.path.join(td, name + ".npz")
    subprocess.run([sys.executable, "-c", _CHILD, path], check=True, env={**os.environ, **env}, cwd=ROOT, timeout=600)
    return np.load(path)


def test_ivf_fp8_refused_with_the_score_buffer_disabled():
    """With MRAG_IVF_SCORES_MB = 0 the search would take the fused regime, which has no fp8 form: MRAG_ERR_UNSUPPORTED,
    and the output buffers keep what they held."""
    with tempfile.TemporaryDirectory() as td:
        on = _run_child(td, "on", {})
        off = _run_child(td, "off", {"MRAG_IVF_SCORES_MB": "0"})
        assert int(on["code"]) == 0 and (on["ids"] >= 0).all()
        np.testing.assert_allclose(on["s0"], off["s0"], rtol=0, atol=TOL)
        assert int(off["code"]) == -5 and "MRAG_ERR_UNSUPPORTED" in str(off["msg"]) and "MRAG_IVF_SCORES_MB" in str(off["msg"])
        assert (off["sc"] == 7.0).all() and (off["ids"] == -7).all()


def test_ivf_fp8_refused_above_256_probed_lists():
    from mrag_amd._native import MragError
    n, d, nlist = 2000, 64, 300
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 51))
    ix = _ivf(c16, c16[:nlist].copy())
    torch = _torch()
    qd = torch.from_numpy(c16[:3]).cuda()
    out = (torch.full((3, 5), 7.0, dtype=torch.float32, device="cuda"), torch.full((3, 5), -7, dtype=torch.int64, device="cuda"))
    with pytest.raises(MragError) as e:
        ix.search(qd, 5, nlist, normalize=False, precision="fp8", out=out)
    torch.cuda.synchronize()
    assert e.value.code == -5
    assert (out[0] == 7.0).all().item() and (out[1] == -7).all().item()
    sc, ids = ix.search(c16[:3], 5, 256, normalize=False, precision="fp8")     # 256 lists: served
    assert (ids[:, 0] == np.arange(3)).all()


# ---------------------------------------------------------------------------------------------- 8. exact paths undisturbed
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_ivf_exact_paths_bit_identical_with_fp8_copy(dtype):
    n, d, nlist, nprobe = 30_000, 384, 64, 8
    c = _round(ds.make_gaussian(n, d, 21), dtype)
    q = _round(ds.make_gaussian(400, d, 22), dtype)
    cen = ds.kmeans_spherical(ds.normalize_round(ds.make_gaussian(n, d, 21)), nlist, 2, seed=9)
    a, b = _ivf(c, cen, dtype=dtype, fp8=False), _ivf(c, cen, dtype=dtype, fp8=True)
    b.search(q, 10, nprobe, normalize=False, precision="fp8")    # an fp8 search in between must not disturb the next exact one
    for nq, k in ((1, 10), (16, 10), (400, 10), (400, 64)):
        sa, ia = a.search(q[:nq], k, nprobe, normalize=False)
        sb, ib = b.search(q[:nq], k, nprobe, normalize=False)
        assert np.array_equal(ia, ib) and np.array_equal(sa, sb), (nq, k)
        b.search(q[:nq], k, nprobe, normalize=False, precision="fp8")
    allow = np.random.default_rng(5).random(n) < 0.3
    for path in ("probe", "exact"):
        ra, rb = (ix.search(q, 10, nprobe, normalize=False, allow=allow, filter_path=path) for ix in (a, b))
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]), path
    b.search(q, 10, nprobe, normalize=False, precision="fp8")
    ra, rb = (ix.range_search(q, 0.1, 20, nprobe, normalize=False) for ix in (a, b))
    for x, y in zip(ra, rb):
        assert np.array_equal(_np(x), _np(y))
    assert (_np(ra[2]) > 0).any()
    b.search(q, 10, nprobe, normalize=False, precision="fp8")
    ja, jb = (ix.self_join(0.1, nprobe, k=16) for ix in (a, b))
    for x, y in zip(ja, jb):
        assert np.array_equal(_np(x), _np(y))
    assert (_np(ja[2]) > 0).any()


# ---------------------------------------------------------------------------------------------- 9. sharded
def test_sharded_world1_ivf_fp8_matches_local():
    import torch.distributed as dist
    from mrag_amd.sharded import ShardedIVFIndex
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29633")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        n, d, k, nlist, nprobe = 40_000, 256, 10, 64, 8
        c16 = ds.normalize_round(ds.make_gaussian(n, d, 41))
        q16 = ds.normalize_round(ds.make_gaussian(300, d, 42))
        sh = ShardedIVFIndex(d, nlist, n, rank=0, world=1, device=0, fp8_scan=True)
        sh.set_centroids(ds.kmeans_spherical(c16, nlist, 2, seed=8), normalize=False)
        sh.add_local(c16, normalize=False)
        for nq in (3, 300):
            ls, li = sh.index.search(q16[:nq], k, nprobe, precision="fp8")
            ss, si = sh.search(q16[:nq], k, nprobe, force_collective=True, precision="fp8")
            ss, si = np.asarray(ss), np.asarray(si)
            assert np.array_equal(si, li) and np.array_equal(ss, ls), nq
            assert sh.index.last_fp8() == {"refine": 40}
    finally:
        if created:
            dist.destroy_process_group()
