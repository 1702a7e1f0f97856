"""CPU tests of the filtered IVF search's host side: the numpy restatement of its semantics (used by the GPU tests too),
allow-set validation, AUTO's rule (mrag_ivf_choose_filter_path, pure arithmetic) and the sharded exchange with a global
allow-set (gloo, injected numpy searcher and per-list counts)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest


def ivf_filtered_ref(q, c, cen, assign, mask, nprobe, k, id_base=0, path="probe", list_allowed=None):
    """Restatement of mrag_ivf_search_filtered (include/mrag.h) in fp64.  A list is live when it holds an allowed row
    (or, with ``list_allowed``, when that count is > 0); path "probe": every query probes its ``nprobe`` best live lists by
    (centroid score desc, list id asc) and returns the top-k of the allowed rows there; path "exact" (or nprobe >= nlist):
    the top-k over all allowed rows.  Order (score desc, row asc), ids = row + id_base, empty slots (-inf, -1).
    -> (scores [nq,k], ids [nq,k], margin [nq]): margin = gap between the last probed and the first unprobed live list's
    centroid score (inf when every live list is probed) -- below ~1e-5 the device's fp32 ranking may pick the other one."""
    q64, c64 = np.asarray(q, dtype=np.float64), np.asarray(c, dtype=np.float64)
    assign = np.asarray(assign, dtype=np.int64)
    mask = np.asarray(mask, dtype=bool)
    nlist, nq = cen.shape[0], q64.shape[0]
    counts = np.bincount(assign[mask], minlength=nlist) if list_allowed is None else np.asarray(list_allowed)
    live = np.flatnonzero(counts > 0)
    cs = q64 @ np.asarray(cen, dtype=np.float64).T
    out_v = np.full((nq, k), -np.inf)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    margin = np.full(nq, np.inf)
    exact = path == "exact" or nprobe >= nlist
    allowed = np.flatnonzero(mask)
    for i in range(nq):
        if exact:
            rows = allowed
        else:
            s = cs[i, live]
            order = np.lexsort((live, -s))
            pick = live[order[:nprobe]]
            if live.size > nprobe:
                margin[i] = s[order[nprobe - 1]] - s[order[nprobe]]
            rows = allowed[np.isin(assign[allowed], pick)]
        if rows.size:
            sc = c64[rows] @ q64[i]
            o = np.lexsort((rows, -sc))[:k]
            out_v[i, :o.size] = sc[o]
            out_i[i, :o.size] = rows[o] + id_base
    return out_v, out_i, margin


def test_restatement_basics():
    rng = np.random.default_rng(0)
    c = rng.standard_normal((40, 8)); q = rng.standard_normal((3, 8)); cen = rng.standard_normal((4, 8))
    assign = np.argmax(c @ cen.T, axis=1)
    full = np.ones(40, dtype=bool)
    v_e, i_e, _ = ivf_filtered_ref(q, c, cen, assign, full, 4, 5, path="exact")
    v_p, i_p, m = ivf_filtered_ref(q, c, cen, assign, full, 4, 5)       # nprobe == nlist: exact
    assert np.array_equal(i_e, i_p) and np.isinf(m).all()
    none = np.zeros(40, dtype=bool)
    v, i, _ = ivf_filtered_ref(q, c, cen, assign, none, 2, 5, id_base=7)
    assert (i == -1).all() and np.isneginf(v).all()
    one = np.zeros(40, dtype=bool); one[np.flatnonzero(assign == assign[0])[:2]] = True
    v, i, _ = ivf_filtered_ref(q, c, cen, assign, one, 1, 5, id_base=100)
    assert ((i >= 0).sum(axis=1) == 2).all() and set(i[i >= 0] - 100) <= set(np.flatnonzero(one))


def test_allow_validation_raises():
    from mrag_amd.sharded import ShardedIVFIndex, local_allow_mask
    n = 100
    with pytest.raises(ValueError):
        local_allow_mask(np.ones(99, dtype=bool), n, 0, 50)               # wrong length
    with pytest.raises(ValueError):
        local_allow_mask(np.array([0, 100]), n, 0, 50)                    # position out of range
    with pytest.raises(ValueError):
        local_allow_mask(np.ones((10, 10), dtype=bool), n, 0, 50)         # not 1-D
    with pytest.raises(ValueError):
        local_allow_mask(np.ones(n, dtype=np.float32), n, 0, 50)          # not a mask or positions
    got = local_allow_mask(np.array([3, 60, 70]), n, 50, 100)
    assert got.shape == (50,) and np.flatnonzero(got).tolist() == [10, 20]
    calls = []
    sh = ShardedIVFIndex(8, 4, n, 0, 1, local_search=lambda *a, **kw: calls.append(kw),
                         local_list_counts=lambda m: np.zeros(4, dtype=np.int32))
    with pytest.raises(ValueError):
        sh.search(np.zeros((2, 8), dtype=np.float32), 5, 2, allow=np.ones(n, dtype=bool), filter_path="mask")
    with pytest.raises(ValueError):
        sh.search(np.zeros((2, 8), dtype=np.float32), 5, 2, allow=np.ones(n + 1, dtype=bool))
    assert not calls


def test_choose_filter_path_rule():
    from mrag_amd.index import ivf_choose_filter_path
    for nq in (1, 16, 17, 10_000):
        for nprobe, nlist in ((8, 256), (32, 4096), (100, 512)):
            n = 625_000
            paths = [ivf_choose_filter_path(nq, 10, nprobe, nlist, n, m, 768) for m in
                     (0, 1, 10, 100, 1000, 10_000, 100_000, n)]
            assert set(paths) <= {"probe", "exact"}
            # monotonic in m: exact for few allowed rows, probe from some m on, never back
            first_probe = paths.index("probe") if "probe" in paths else len(paths)
            assert all(p == "exact" for p in paths[:first_probe]) and all(p == "probe" for p in paths[first_probe:])
            assert paths[0] == "exact"
            if (nprobe, nlist) == (32, 4096):                          # the measured shape: all-allowed probes
                assert paths[-1] == "probe"
            for m in (0, 1000, n):                                      # exhaustive probing is filtered brute force
                assert ivf_choose_filter_path(nq, 10, nlist, nlist, n, m, 768) == "exact"
                assert ivf_choose_filter_path(nq, 10, nlist + 5, nlist, n, m, 768) == "exact"
    from mrag_amd import _native as N
    with pytest.raises(N.MragError):
        ivf_choose_filter_path(10, 10, 8, 256, 100, 101, 768)          # more allowed rows than rows


WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["MRAG_ROOT"]); sys.path.insert(0, os.path.join(os.environ["MRAG_ROOT"], "tests"))
import numpy as np, torch.distributed as dist
from mrag_amd.sharded import ShardedIVFIndex, shard_bounds
from oracle import dense_search as ds
from test_ivf_filtered_host import ivf_filtered_ref
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
n, nq, d, k, nlist, nprobe = 3001, 40, 32, 10, 24, 3
c16 = ds.normalize_round(ds.make_gaussian(n, d, 1234)); q16 = ds.normalize_round(ds.make_gaussian(nq, d, 5678))
cen = ds.kmeans_spherical(c16, nlist, 2, seed=1)
assign = ds.ivf_assign(c16, cen).astype(np.int64)
lo, hi = shard_bounds(n, world, rank)
seen = {}

def counts(local_mask):
    assert local_mask.shape == (hi - lo,)
    return np.bincount(assign[lo:hi][local_mask], minlength=nlist).astype(np.int32)

def local(queries, kk, npr, allow=None, filter_path=None, list_allowed=None):
    assert allow is not None and filter_path in ("probe", "exact") and list_allowed.shape == (nlist,)
    seen["path"] = filter_path
    v, i, _ = ivf_filtered_ref(np.asarray(queries), c16[lo:hi], cen, assign[lo:hi], allow, npr, kk, lo, filter_path, list_allowed)
    return v.astype(np.float32), i

sh = ShardedIVFIndex(d, nlist, n, rank, world, local_search=local, local_list_counts=counts)
rng = np.random.default_rng(3)
owner = np.searchsorted([shard_bounds(n, world, r)[1] for r in range(world)], np.arange(n), side="right")
masks = {"random": rng.random(n) < 0.05,
         "first_only": np.isin(np.arange(n), np.arange(10, 40)),
         "per_rank_lists": (assign % world) == owner,          # each list's allowed rows sit on one rank only
         "none": np.zeros(n, dtype=bool)}
for name, mask in masks.items():
    for path in ("probe", "exact", "auto"):
        want_path = path
        if path == "auto":
            from mrag_amd.index import ivf_choose_filter_path
            want_path = ivf_choose_filter_path(nq, k, nprobe, nlist, n, int(mask.sum()), d)
        want_s, want_i, margin = ivf_filtered_ref(q16, c16, cen, assign, mask, nprobe, k, 0, want_path)
        for allow in (mask, np.flatnonzero(mask)):
            s_, i_ = sh.search(q16, k, nprobe, allow=allow, filter_path=path)
            assert seen["path"] == want_path, (name, path)
            assert (i_ == want_i).all(), (name, path, "ids")
            np.testing.assert_allclose(s_, want_s, rtol=0, atol=1e-6)
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_ivf_filtered_on_gloo(world, tmp_path):
    root = Path(__file__).resolve().parent.parent
    script = tmp_path / "ivf_filtered_ranks.py"
    script.write_text(WORKER)
    env = dict(os.environ, MRAG_ROOT=str(root), MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                        "--master-addr", "127.0.0.1", "--master-port", str(29580 + world), str(script)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == world
