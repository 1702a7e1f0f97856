"""CPU tests: the C-ABI library loads and exports every symbol include/mrag.h declares; compute
entry points fail loudly without a GPU; host merge; the N>1 exchange path on gloo (world 2)."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_library_exports_every_declared_symbol():
    from mrag_amd import _native as N
    header = (ROOT / "include" / "mrag.h").read_text()
    declared = set(re.findall(r"\b(mrag_[a-z0-9_]+)\s*\(", header))
    declared -= {"mrag_handle"}
    assert declared == set(N.SIGNATURES), declared ^ set(N.SIGNATURES)
    lib = N.load()
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.mrag_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.lib_path())], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(mrag_[a-z0-9_]+)$", out, flags=re.M))
    assert declared <= exported


def test_no_silent_cpu_fallback():
    if _has_gpu():
        pytest.skip("GPU present")
    from mrag_amd import _native as N
    from mrag_amd.index import DenseIndex, cosine_f64
    assert N.device_count() == 0
    with pytest.raises(N.MragError) as e:
        DenseIndex(64)
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)
    with pytest.raises(N.MragError):
        cosine_f64(np.ones(4), np.ones((2, 4)))


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from mrag_amd import _native as N
    monkeypatch.setattr(N, "_LIB", None)
    monkeypatch.setenv("MRAG_HIP_LIB", str(tmp_path / "nope.so"))
    with pytest.raises(N.MragLibraryMissing):
        N.load()
    monkeypatch.delenv("MRAG_HIP_LIB")
    monkeypatch.setattr(N, "_LIB", None)
    N.load()


def test_host_merge_matches_oracle():
    from mrag_amd.index import topk_merge
    from oracle import dense_search as ds
    rng = np.random.default_rng(0)
    nparts, nq, k = 8, 700, 10
    sc = rng.integers(0, 50, size=(nparts, nq, k)).astype(np.float32) / 7     # many exact ties
    sc = -np.sort(-sc, axis=2)
    ids = rng.permutation(nparts * nq * k).reshape(nparts, nq, k).astype(np.int64)
    ids[3, :, 7:] = -1                                                       # empty slots
    sc[3, :, 7:] = -np.inf
    v, i = topk_merge(sc, ids)
    ov, oi = ds.merge_topk([sc[p] for p in range(nparts)], [ids[p] for p in range(nparts)], k)
    assert (i == oi).all() and (v == ov.astype(np.float32)).all()
    v1, i1 = topk_merge(sc, ids, nthreads=1)
    assert (i1 == i).all()
    vs, is_ = topk_merge(sc[:1, :, :3] * 0 - np.inf, ids[:1, :, :3] * 0 - 1)
    assert (is_ == -1).all() and np.isneginf(vs).all()


WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["MRAG_ROOT"])
import numpy as np, torch, torch.distributed as dist
from mrag_amd.sharded import ShardedDenseIndex, shard_bounds
from oracle import dense_search as ds
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
n, nq, d, k = 3001, 37, 48, 10
c16 = ds.normalize_round(ds.make_gaussian(n, d, 1234)); q16 = ds.normalize_round(ds.make_gaussian(nq, d, 5678))
lo, hi = shard_bounds(n, world, rank)
def local(q, k):                       # the oracle plays the per-GPU kernel in this CPU test
    v, i = ds.brute_force_topk(q, c16[lo:hi], k)
    return v.astype(np.float32), np.where(i >= 0, i + lo, i)
sh = ShardedDenseIndex(d, n, rank, world, local_search=local)
assert (sh.lo, sh.hi) == (lo, hi)
for _ in range(2):                     # second call reuses the gather buffers
    v, i = sh.search(q16, k)
rv, ri = ds.brute_force_topk(q16, c16, k)
assert (i == ri).all(), "sharded ids differ from unsharded"
assert np.array_equal(v, rv.astype(np.float32))
assert set(sh.last_phases) >= {"local_ms", "pack_ms", "gather_ms", "merge_ms"}, sh.last_phases
# two-half pipeline (all-gather of half A in flight under the local search of half B): exactly the one-shot result
vp, ip = sh.search(q16, k, pipeline=True)
assert np.array_equal(ip, i) and np.array_equal(vp, v)
assert set(sh.last_phases) >= {"local_ms", "pack_ms", "gather_ms", "merge_ms"}, sh.last_phases
vp1, ip1 = sh.search(q16[:1], k, pipeline=True)      # a single query cannot be cut: falls back to one shot
assert np.array_equal(ip1, i[:1])
# changing batch sizes and k, one shot and pipeline in turn, on the SAME index: every answer is the unsharded one ...
turn = 0
for k2 in (10, 3):
    for nq2 in (37, 5, 2, 36, 19):
        v2, i2 = sh.search(q16[:nq2], k2, pipeline=bool(turn & 1)); turn += 1
        rv2, ri2 = ds.brute_force_topk(q16[:nq2], c16, k2)
        assert (i2 == ri2).all() and np.array_equal(v2, rv2.astype(np.float32)), (k2, nq2)
# ... and the exchange keeps gather buffers for the last call's shape only (here: 19 rows cut 9 + 10), not one set per batch size
assert [tuple(g.shape) for g in sh._exchange.gather] == [(world, 9, 3), (world, 10, 3)], [g.shape for g in sh._exchange.gather]
# ADVICE r2: one caller-kept `bufs` reused with ANOTHER n_total (same world / q / k) must not reuse stale bases
from mrag_amd.sharded import gather_and_merge
bufs = {}
for n2 in (n, 2000):
    lo2, hi2 = shard_bounds(n2, world, rank)
    v2, i2 = ds.brute_force_topk(q16, c16[lo2:hi2], k)
    i2 = np.where(i2 >= 0, i2 + lo2, i2)
    gv, gi = gather_and_merge(torch.from_numpy(v2.astype(np.float32)), torch.from_numpy(i2), bufs=bufs,
                              id_bases=[shard_bounds(n2, world, r)[0] for r in range(world)])
    rv2, ri2 = ds.brute_force_topk(q16, c16[:n2], k)
    assert (gi == ri2).all(), f"stale id bases after n_total changed to {n2}"
# ... and ids that do not fit the 32-bit shard-local slot raise on every rank, they never wrap
bad_ids = torch.from_numpy(i2).clone(); bad_ids[0, 0] = lo2 - 1 if lo2 > 0 else lo2 + 2**32
try:
    gather_and_merge(torch.from_numpy(v2.astype(np.float32)), bad_ids, bufs=bufs,
                     id_bases=[shard_bounds(n2, world, r)[0] for r in range(world)])
    raise SystemExit("out-of-range id was packed silently")
except ValueError as e:
    assert "outside" in str(e)
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_exchange_on_gloo(world, tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MRAG_ROOT=str(ROOT), MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                        "--master-addr", "127.0.0.1", "--master-port", str(29500 + world), str(script)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("ok") == world


IVF_WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["MRAG_ROOT"])
import numpy as np, torch, torch.distributed as dist
from mrag_amd.sharded import ShardedIVFIndex, shard_bounds
from oracle import dense_search as ds
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
n, nq, d, k, nlist, nprobe = 4003, 41, 32, 10, 16, 5
rows, qs = ds.make_clustered(n, nq, d, 3, n_centroids=16)
c16, q16 = ds.normalize_round(rows), ds.normalize_round(qs)
cen = ds.kmeans_spherical(c16, nlist, 3, seed=1)       # replicated centroids (trained once)
assign = ds.ivf_assign(c16, cen)
lo, hi = shard_bounds(n, world, rank)
def local(q, k, nprobe):               # the oracle plays the per-GPU IVF kernel: this rank's rows of EVERY list
    v, i = ds.ivf_search(q, c16[lo:hi], cen, assign[lo:hi], nprobe, k)
    return v.astype(np.float32), np.where(i >= 0, i + lo, i)
sh = ShardedIVFIndex(d, nlist, n, rank, world, local_search=local)
for _ in range(2):
    v, i = sh.search(q16, k, nprobe)
rv, ri = ds.ivf_search(q16, c16, cen, assign, nprobe, k)
assert (i == ri).all(), "sharded IVF ids differ from the unsharded IVF result"
assert np.array_equal(v, rv.astype(np.float32))
# few rows per (shard, probe set): empty slots (-1, -inf) cross the packed exchange intact
v2, i2 = sh.search(q16[:3], 64, 1)
rv2, ri2 = ds.ivf_search(q16[:3], c16, cen, assign, 1, 64)
assert (i2 == ri2).all() and np.array_equal(v2, rv2.astype(np.float32))
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_sharded_ivf_exchange_on_gloo(tmp_path):
    world = 2
    script = tmp_path / "ivf_worker.py"
    script.write_text(IVF_WORKER)
    env = dict(os.environ, MRAG_ROOT=str(ROOT), MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                        "--master-addr", "127.0.0.1", "--master-port", "29511", str(script)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("ok") == world


def test_packed_partial_roundtrip():
    """one all-gather of 8-byte (score, int32 shard-local id) words."""
    import torch
    from mrag_amd.sharded import pack_partial, unpack_partial
    sc = torch.tensor([[1.5, -0.0, float("-inf")], [3.0e-39, -2.25, float("-inf")]], dtype=torch.float32)
    ids = torch.tensor([[7_000_000_123, 7_000_000_000, -1], [7_000_000_000 + 2**31 + 5, 7_000_000_001, -1]], dtype=torch.int64)
    w = pack_partial(sc, ids, 7_000_000_000)
    assert w.dtype == torch.int64 and w.shape == sc.shape
    s2, i2 = unpack_partial(w.view(1, 2, 3), torch.tensor([7_000_000_000]).view(1, 1, 1))
    assert torch.equal(i2[0], ids) and torch.equal(s2[0].view(torch.int32), sc.view(torch.int32))


def test_shard_bounds_cover_everything():
    from mrag_amd.sharded import shard_bounds
    for n in (0, 1, 7, 1_000_000):
        for w in (1, 2, 3, 8):
            b = [shard_bounds(n, w, r) for r in range(w)]
            assert b[0][0] == 0 and b[-1][1] == n and all(b[i][1] == b[i + 1][0] for i in range(w - 1))


def test_bench_self_launches_ranks_and_reports_missing_devices():
    """`python bench.py --gpus N` must launch its own ranks (child torchrun, never exec) and a box
    with fewer devices must say so -- not die on "launch with torch.distributed.run"."""
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"))
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two devices present: the launch itself is exercised by the driver")
    assert r.returncode != 0
    assert "needs 2 visible MI355X devices" in (r.stdout + r.stderr)
