"""GPU parity of the filtered IVF search (IVFFlatIndex.search(allow=...), mrag_ivf_search_filtered): path P (filter-aware
probing), path E (filtered brute force) and AUTO, against the numpy restatement in test_ivf_filtered_host.py on the
GPU's own assignments.  Queries whose last probed and first unprobed live list score within 1e-5 (the fp32 centroid
ranking may legally swap them) are left out of the strict comparison."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import dense_search as ds

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_ivf_filtered_host import ivf_filtered_ref  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _round(x, dtype):
    """normalised rows, rounded once to the storage dtype, as fp32 (exactly representable in it)"""
    import torch
    x = ds.l2_normalize(x).astype(np.float32)
    return torch.from_numpy(x).to(torch.bfloat16 if dtype == "bf16" else torch.float16).float().numpy()


def _data(n=20000, nq=200, d=128, seed=7, dtype="f16"):
    rows, qs = ds.make_clustered(n, nq, d, seed, n_centroids=64)
    return _round(rows, dtype), _round(qs, dtype)


def _index(c, cen, dtype="f16", id_base=0):
    from mrag_amd.index import IVFFlatIndex
    ix = IVFFlatIndex(c.shape[1], cen.shape[0], dtype=dtype)
    ix.set_centroids(cen, normalize=False)
    ix.add(c, normalize=False)
    if id_base:
        ix.set_id_base(id_base)
    return ix


def _row_centroids(c, nlist, seed):
    """centroids = distinct corpus rows: every list holds at least its own row (no empty list)"""
    return c[np.random.default_rng(seed).choice(c.shape[0], size=nlist, replace=False)]


def _check(sc, ids, rv, ri, margin, tol=TOL):
    assert sc.shape == rv.shape and ids.dtype == np.int64
    keep = margin >= tol
    assert keep.mean() > 0.9
    sc, ids, rv, ri = sc[keep], ids[keep], rv[keep], ri[keep]
    valid = ri >= 0
    assert ((ids >= 0) == valid).all()
    assert np.isneginf(sc[~valid]).all() and (ids[~valid] == -1).all()
    np.testing.assert_allclose(sc[valid], rv[valid], rtol=0, atol=tol)
    strict, bad = ds.gap_aware_id_match(ids, sc, ri, rv, tol=tol)
    assert bad == 0, (strict, bad)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("nprobe,nlist", [(8, 64), (100, 256)])
def test_probe_path_matches_restatement(dtype, nprobe, nlist):
    c, q = _data(dtype=dtype)
    cen = _round(ds.kmeans_spherical(c, nlist, 2, seed=3, dtype=np.float32), dtype)
    base = 1000
    ix = _index(c, cen, dtype, id_base=base)
    assign = ix.assignments()
    rng = np.random.default_rng(nprobe)
    for sel in (0.5, 0.1, 0.01, 0.001):
        mask = rng.random(c.shape[0]) < sel
        sc, ids = ix.search(q, 10, nprobe, normalize=False, allow=mask, filter_path="probe")
        lf = ix.last_filter()
        assert lf["path"] == "probe" and lf["allowed"] == int(mask.sum())
        assert lf["live_lists"] == int((np.bincount(assign[mask], minlength=nlist) > 0).sum())
        rv, ri, margin = ivf_filtered_ref(q, c, cen, assign, mask, nprobe, 10, base)
        _check(sc, ids, rv, ri, margin)
        counts = ix.allowed_per_list(mask)
        assert np.array_equal(counts, np.bincount(assign[mask], minlength=nlist))
    ix.close()


@pytest.mark.parametrize("nprobe", [8, 100])
def test_all_allowed_is_the_plain_search(nprobe):
    c, q = _data()
    nlist = 256
    cen = _row_centroids(c, nlist, 5)
    ix = _index(c, cen, id_base=77)
    assert (np.bincount(ix.assignments(), minlength=nlist) > 0).all()          # no empty list
    s0, i0 = ix.search(q, 10, nprobe, normalize=False)
    for allow in (np.ones(c.shape[0], dtype=bool), np.arange(c.shape[0])):
        s1, i1 = ix.search(q, 10, nprobe, normalize=False, allow=allow, filter_path="probe")
        assert np.array_equal(s0, s1) and np.array_equal(i0, i1)
    assert ix.last_filter()["live_lists"] == nlist
    ix.close()


def test_empty_lists_are_dead():
    """duplicate centroids: a tie goes to the lowest list id, so the higher copy's list stays empty.  P never probes it
    (the next live list takes its place); the plain search spends a probe on it."""
    c, q = _data()
    base = _row_centroids(c, 200, 5)
    cen = np.concatenate([base, base[:56]])                 # lists 200..255 empty
    ix = _index(c, cen)
    assign = ix.assignments()
    cnt = np.bincount(assign, minlength=256)
    assert (cnt[200:] == 0).all() and (cnt[:200] > 0).all()
    full = np.ones(c.shape[0], dtype=bool)
    sc, ids = ix.search(q, 10, 8, normalize=False, allow=full, filter_path="probe")
    rv, ri, margin = ivf_filtered_ref(q, c, cen, assign, full, 8, 10)
    _check(sc, ids, rv, ri, margin)
    assert ix.last_filter()["live_lists"] == 200
    s0, i0 = ix.search(q, 10, 8, normalize=False)
    pv, pi = ds.ivf_search(q, c, cen, assign.astype(np.int64), 8, 10)     # the plain semantics: empty lists use probes
    np.testing.assert_allclose(s0, pv, rtol=0, atol=TOL)
    assert not np.array_equal(i0, ids)                       # some query probed a duplicate: P found other rows
    assert (sc >= s0 - TOL).all()                            # ... never worse ones
    ix.close()


def test_list_correlated_mask_needs_filter_aware_probing():
    c, q = _data()
    nlist, nprobe, k = 64, 8, 10
    cen = _round(ds.kmeans_spherical(c, nlist, 2, seed=3, dtype=np.float32), "f16")
    ix = _index(c, cen)
    assign = ix.assignments()
    cs = q.astype(np.float64) @ cen.astype(np.float64).T
    far = np.argsort(cs.max(axis=0))[:3]                    # the lists no query is near
    far = far[np.bincount(assign, minlength=nlist)[far] >= k]
    assert far.size
    mask = np.isin(assign, far)
    sp, ip = ix.search(q, k, nprobe, normalize=False, allow=mask, filter_path="probe")
    se, ie = ix.search(q, k, nprobe, normalize=False, allow=mask, filter_path="exact")
    assert (ip >= 0).all()                                   # full k results
    assert np.array_equal(sp, se) and np.array_equal(ip, ie)
    s0, i0 = ix.search(q, k, nprobe, normalize=False)        # post-filtering the plain search
    post = np.where(mask[np.maximum(i0, 0)] & (i0 >= 0), i0, -1)
    assert (post >= 0).mean() < 0.1
    ix.close()


def test_exact_path_is_the_dense_filtered_search():
    from mrag_amd.index import DenseIndex
    c, q = _data()
    nlist = 64
    cen = _round(ds.kmeans_spherical(c, nlist, 2, seed=3, dtype=np.float32), "f16")
    ix = _index(c, cen, id_base=500)
    dx = DenseIndex(c.shape[1])
    dx.add(c, normalize=False)
    dx.set_id_base(500)
    rng = np.random.default_rng(1)
    for sel in (0.3, 0.01):
        mask = rng.random(c.shape[0]) < sel
        se, ie = ix.search(q, 10, 8, normalize=False, allow=mask, filter_path="exact")
        assert ix.last_filter() == {"path": "exact", "allowed": int(mask.sum()), "live_lists": None}
        sd, idd = dx.search(q, 10, normalize=False, allow=mask)
        assert np.array_equal(se, sd) and np.array_equal(ie, idd)
        sa, ia = ix.search(q, 10, nlist, normalize=False, allow=mask, filter_path="probe")   # nprobe == nlist: E
        assert ix.last_filter()["path"] == "exact"
        assert np.array_equal(sa, sd) and np.array_equal(ia, idd)
    ix.close()
    dx.close()


def test_edge_cases():
    c, q = _data()
    nlist = 64
    cen = _round(ds.kmeans_spherical(c, nlist, 2, seed=3, dtype=np.float32), "f16")
    ix = _index(c, cen, id_base=3)
    assign = ix.assignments()
    few = np.zeros(c.shape[0], dtype=bool); few[[5, 900, 17000, 19999]] = True
    none = np.zeros(c.shape[0], dtype=bool)
    lst = int(np.argmax(np.bincount(assign, minlength=nlist)))
    one_list = (assign == lst) & (np.arange(c.shape[0]) % 2 == 0)
    for name, mask in (("few", few), ("none", none), ("one_list", one_list)):
        for path in ("probe", "exact", "auto"):
            sc, ids = ix.search(q, 10, 8, normalize=False, allow=mask, filter_path=path)
            rv, ri, _ = ivf_filtered_ref(q, c, cen, assign, mask, 8, 10, 3, "exact")   # <= nprobe live lists: exact
            _check(sc, ids, rv, ri, np.full(q.shape[0], np.inf))
            if name == "none":
                assert (ids == -1).all() and np.isneginf(sc).all()
            if name == "one_list" and path == "probe":
                assert ix.last_filter()["live_lists"] == 1
    ix.close()


def test_device_form_is_async_and_equal():
    import torch
    c, q = _data()
    nlist = 64
    cen = _round(ds.kmeans_spherical(c, nlist, 2, seed=3, dtype=np.float32), "f16")
    ix = _index(c, cen, id_base=11)
    mask = np.random.default_rng(4).random(c.shape[0]) < 0.05
    qd = torch.from_numpy(q).cuda()
    md = torch.from_numpy(mask).cuda()
    s = torch.cuda.Stream()
    for path in ("probe", "exact", "auto"):
        want_s, want_i = ix.search(q, 10, 8, normalize=False, allow=mask, filter_path=path)
        with torch.cuda.stream(s):
            sc, ids = ix.search(qd, 10, 8, normalize=False, allow=md, filter_path=path, stream=s)
        s.synchronize()
        assert sc.is_cuda and ids.is_cuda
        assert np.array_equal(sc.cpu().numpy(), want_s) and np.array_equal(ids.cpu().numpy(), want_i), path
        assert ix.last_filter()["allowed"] == int(mask.sum())
    counts = ix.allowed_per_list(md, stream=s)
    s.synchronize()
    assert counts.is_cuda and np.array_equal(counts.cpu().numpy(), ix.allowed_per_list(mask))
    # device per-list counts in place of the index's own: the same live lists, the same result
    with torch.cuda.stream(s):
        sc, ids = ix.search(qd, 10, 8, normalize=False, allow=md, filter_path="probe", list_allowed=counts, stream=s)
    s.synchronize()
    want_s, want_i = ix.search(q, 10, 8, normalize=False, allow=mask, filter_path="probe")
    assert np.array_equal(sc.cpu().numpy(), want_s) and np.array_equal(ids.cpu().numpy(), want_i)
    ix.close()


def test_filtered_search_leaves_the_plain_search_alone():
    c, q = _data()
    cen = _round(ds.kmeans_spherical(c, 64, 2, seed=3, dtype=np.float32), "f16")
    ix = _index(c, cen)
    before = {nprobe: ix.search(q, 10, nprobe, normalize=False) for nprobe in (8, 64)}
    for path in ("probe", "exact"):
        ix.search(q, 10, 8, normalize=False, allow=np.random.default_rng(2).random(c.shape[0]) < 0.01, filter_path=path)
        for nprobe, (s0, i0) in before.items():
            s1, i1 = ix.search(q, 10, nprobe, normalize=False)
            assert np.array_equal(s0, s1) and np.array_equal(i0, i1), (path, nprobe)
    ix.close()


FUSED_PROBE_WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["MRAG_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRAG_ROOT"], "tests"))
import numpy as np
from oracle import dense_search as ds
from mrag_amd.index import IVFFlatIndex
from test_ivf_filtered_host import ivf_filtered_ref
# MRAG_IVF_SCORES_MB=4: the probe scores of 200 queries x 5000 lists (5 MB) do not fit, the lists' segments (<= 32 rows
# each, <= 2.6 MB) do -> the probe selection runs the batch (nprobe 8) / streaming (nprobe 100) kernels over the centroids
# with the live-list bitset as their allow-set
n, nq, d, nlist = 20000, 200, 128, 5000
c, q = ds.normalize_round(ds.make_gaussian(n, d, 21)), ds.normalize_round(ds.make_gaussian(nq, d, 22))
cen = c[np.random.default_rng(5).choice(n, size=nlist, replace=False)]
ix = IVFFlatIndex(d, nlist); ix.set_centroids(cen, normalize=False); ix.add(c, normalize=False); ix.set_id_base(9)
assign = ix.assignments()
cnt = np.bincount(assign, minlength=nlist)
assert cnt.min() > 0 and cnt.max() <= 32, (cnt.min(), cnt.max())
rng = np.random.default_rng(1)
for nprobe in (8, 100):
    for sel in (1.0, 0.1, 0.005):
        mask = rng.random(n) < sel
        sc, ids = ix.search(q, 10, nprobe, normalize=False, allow=mask, filter_path="probe")
        assert ix.last_filter()["path"] == "probe"
        rv, ri, margin = ivf_filtered_ref(q, c, cen, assign, mask, nprobe, 10, 9)
        keep = margin >= 1e-5
        assert keep.mean() > 0.9
        np.testing.assert_allclose(sc[keep], rv[keep], rtol=0, atol=1e-5)
        assert ds.gap_aware_id_match(ids[keep], sc[keep], ri[keep], rv[keep], tol=1e-5)[1] == 0, (nprobe, sel)
        if sel == 1.0:
            s0, i0 = ix.search(q, 10, nprobe, normalize=False)
            assert np.array_equal(s0, sc) and np.array_equal(i0, ids)
print("fused probe ok")
"""


def test_fused_probe_selection_regime(tmp_path):
    root = Path(__file__).resolve().parent.parent
    script = tmp_path / "fused_probe.py"
    script.write_text(FUSED_PROBE_WORKER)
    env = dict(os.environ, MRAG_ROOT=str(root), MRAG_IVF_SCORES_MB="4")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "fused probe ok" in r.stdout


SHARDED_WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["MRAG_ROOT"])
import numpy as np, torch, torch.distributed as dist
from mrag_amd.sharded import ShardedIVFIndex, shard_bounds
from mrag_amd.index import IVFFlatIndex
from oracle import dense_search as ds
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
torch.cuda.set_device(0)
n, nq, d, k, nlist, nprobe = 30_001, 200, 128, 10, 128, 4
rows, qs = ds.make_clustered(n, nq, d, 11, n_centroids=64)
c16, q16 = ds.normalize_round(rows), ds.normalize_round(qs)
cen = ds.kmeans_spherical(c16, nlist, 2, seed=3)
lo, hi = shard_bounds(n, world, rank)
sh = ShardedIVFIndex(d, nlist, n, rank, world, device=0)
sh.set_centroids(cen, normalize=False)
sh.add_local(torch.from_numpy(c16[lo:hi]).cuda(), normalize=False)
one = IVFFlatIndex(d, nlist); one.set_centroids(cen, normalize=False); one.add(c16, normalize=False)
assign = one.assignments()
q = torch.from_numpy(q16).cuda()
owner = np.searchsorted([shard_bounds(n, world, r)[1] for r in range(world)], np.arange(n), side="right")
rng = np.random.default_rng(7)
masks = {"random": rng.random(n) < 0.02,
         "first_only": np.isin(np.arange(n), np.arange(100, 400)),     # ranks 1 and 2 have no allowed row
         "per_rank_lists": (assign % world) == owner}                   # every list's allowed rows on one rank only
for name, mask in masks.items():
    for path in ("probe", "exact", "auto"):
        rs_, ri_ = one.search(q, k, nprobe, normalize=False, allow=mask, filter_path=path); torch.cuda.synchronize()
        rs_, ri_ = rs_.cpu().numpy(), ri_.cpu().numpy()
        for mode in ("device", "host"):
            s_, i_ = sh.search(q, k, nprobe, merge=mode, allow=mask, filter_path=path)
            s_ = s_.cpu().numpy() if torch.is_tensor(s_) else s_
            i_ = i_.cpu().numpy() if torch.is_tensor(i_) else i_
            assert (i_ == ri_).all() and np.array_equal(s_, rs_), (name, path, mode, "sharded filtered IVF != one index")
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_three_ranks_filtered_ivf_on_one_gpu(tmp_path):
    root = Path(__file__).resolve().parent.parent
    script = tmp_path / "ranks_ivf_filtered.py"
    script.write_text(SHARDED_WORKER)
    env = dict(os.environ, MRAG_ROOT=str(root), MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3",
                        "--master-addr", "127.0.0.1", "--master-port", "29663", str(script)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 3
