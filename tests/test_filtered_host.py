"""CPU tests of the filtered search's host side: allow-set packing and validation, the loud failure without a GPU,
the sharded exchange with a global allow-set (gloo, injected oracle searcher) and the backend's filter resolution."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest


def _ref_words(mask):
    n = mask.shape[0]
    w = np.zeros((n + 31) // 32, dtype=np.uint32)
    for r in np.flatnonzero(mask):
        w[r // 32] |= np.uint32(1) << np.uint32(r % 32)
    return w


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000, 4097])
def test_allow_packing_equivalence(n):
    from mrag_amd.index import allow_bits
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.3
    want = _ref_words(mask)
    for a in (mask, mask.astype(np.uint8), mask.astype(np.uint8) * 7, np.flatnonzero(mask),
              np.flatnonzero(mask).astype(np.int32)):
        got = allow_bits(a, n)
        assert got.dtype == np.uint32 and got.shape == want.shape
        assert np.array_equal(got, want)
    import torch
    assert np.array_equal(allow_bits(torch.from_numpy(mask), n), want)
    assert np.array_equal(allow_bits(np.array([], dtype=np.int64), n), np.zeros_like(want))


def test_allow_validation_raises():
    from mrag_amd.index import allow_bits
    with pytest.raises(ValueError):
        allow_bits(np.ones(9, dtype=bool), 10)               # wrong length
    with pytest.raises(ValueError):
        allow_bits(np.ones(11, dtype=np.uint8), 10)
    with pytest.raises(ValueError):
        allow_bits(np.array([0, -1]), 10)                    # negative position
    with pytest.raises(ValueError):
        allow_bits(np.array([3, 10]), 10)                    # out of range
    with pytest.raises(ValueError):
        allow_bits(np.ones((2, 5), dtype=bool), 10)          # not 1-D
    with pytest.raises(ValueError):
        allow_bits(np.ones(10, dtype=np.float32), 10)        # neither mask nor positions


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_filtered_search_without_gpu_is_loud():
    if _has_gpu():
        pytest.skip("GPU present")
    import ctypes as C
    from mrag_amd import _native as N
    from mrag_amd.index import DenseIndex
    with pytest.raises(N.MragError) as e:
        DenseIndex(64)
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)
    # an index object without a live handle: the filtered search reaches the library and fails there
    ix = DenseIndex.__new__(DenseIndex)
    ix._lib, ix.dim, ix.metric, ix.device, ix._h = N.load(), 64, "cosine", 0, C.c_uint64(0)
    with pytest.raises(N.MragError):
        ix.search(np.ones((1, 64), dtype=np.float32), 5, allow=np.ones(10, dtype=bool))
    with pytest.raises(N.MragError):
        ix.last_filter()
    lib = N.load()
    sc, ids = np.zeros(5, np.float32), np.zeros(5, np.int64)
    q, allow = np.ones(64, np.float32), np.ones(1, np.uint32)
    st = lib.mrag_index_search_filtered(0, q.ctypes.data, 1, N.MRAG_F32, 0, 0, 5, allow.ctypes.data, 10, N.ALLOW_BITS32, 0,
                                        N.FILTER_AUTO, sc.ctypes.data, ids.ctypes.data, 0, None)
    assert st == -1


WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["MRAG_ROOT"])
import numpy as np, torch.distributed as dist
from mrag_amd.sharded import ShardedDenseIndex, shard_bounds
from mrag_amd.index import allow_bits
from oracle import dense_search as ds
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
n, nq, d, k = 3001, 20, 32, 10
c16 = ds.normalize_round(ds.make_gaussian(n, d, 1)); q16 = ds.normalize_round(ds.make_gaussian(nq, d, 2))
lo, hi = shard_bounds(n, world, rank)

def oracle_filtered(q, cc, mask, kk, base):
    rows = np.flatnonzero(mask)
    if rows.size == 0:
        return np.full((q.shape[0], kk), -np.inf, np.float32), np.full((q.shape[0], kk), -1, np.int64)
    v, i = ds.brute_force_topk(q, cc[rows], kk)
    return v.astype(np.float32), np.where(i >= 0, rows[np.maximum(i, 0)] + base, -1)

def local(queries, kk, allow=None, **kw):
    mask = np.ones(hi - lo, dtype=bool) if allow is None else allow
    assert mask.shape == (hi - lo,)
    return oracle_filtered(np.asarray(queries), c16[lo:hi], mask, kk, lo)

sh = ShardedDenseIndex(d, n, rank, world, local_search=local)
rng = np.random.default_rng(3)
mask = rng.random(n) < 0.05
first_only = np.zeros(n, dtype=bool); first_only[10:40] = True
for allow in (mask, np.flatnonzero(mask), first_only, mask.astype(np.uint8)):
    m = allow.astype(bool) if allow.dtype in (np.bool_, np.uint8) else np.isin(np.arange(n), allow)
    want_s, want_i = oracle_filtered(q16, c16, m, k, 0)
    for pipe in (False, True):
        s_, i_ = sh.search(q16, k, pipeline=pipe, allow=allow)
        assert (i_ == want_i).all(), (pipe, "ids")
        np.testing.assert_allclose(s_, want_s, rtol=0, atol=1e-6)
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_filtered_on_gloo(world, tmp_path):
    root = Path(__file__).resolve().parent.parent
    script = tmp_path / "filtered_ranks.py"
    script.write_text(WORKER)
    env = dict(os.environ, MRAG_ROOT=str(root), MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                        "--master-addr", "127.0.0.1", "--master-port", str(29560 + world), str(script)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == world


def keep_even_rows(req, rows):
    return np.arange(len(rows)) % 2 == 0


def test_dense_row_filter_resolution():
    from mrag_amd.backend import DenseRetrievalBackend
    b = DenseRetrievalBackend(router=None, dense_row_filter="test_filtered_host:keep_even_rows")
    assert b.dense_row_filter is keep_even_rows or b.dense_row_filter.__name__ == "keep_even_rows"
    assert b.dense_row_filter(None, [0, 1, 2]).tolist() == [True, False, True]
    assert DenseRetrievalBackend(router=None).dense_row_filter is None
    f = lambda req, rows: None          # noqa: E731
    assert DenseRetrievalBackend(router=None, dense_row_filter=f).dense_row_filter is f
    with pytest.raises(TypeError):
        DenseRetrievalBackend(router=None, dense_row_filter=42)
    with pytest.raises((ImportError, AttributeError, ValueError)):
        DenseRetrievalBackend(router=None, dense_row_filter="no_such_module_here:f")
