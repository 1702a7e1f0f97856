"""Host-side pieces of the IVF fp8 scan: the new symbols in the C ABI (header, binding, library), the Python argument
checks of IVFFlatIndex.search(precision=..., refine=...) raised before any native call, the keyword defaults, and the
pass-through of precision / refine from ShardedIVFIndex.search to the local search (gloo, injected numpy searcher)."""
import ctypes
import inspect
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NEW = {"mrag_ivf_enable_fp8": 1, "mrag_ivf_get_rows_fp8": 6, "mrag_ivf_search_fp8": 13, "mrag_ivf_last_fp8": 2}


class _NoNative:
    """stands in for the library: any native call fails the test"""
    def __getattr__(self, name):
        raise AssertionError(f"native call {name} reached")


def _fake_ivf():
    from mrag_amd.index import IVFFlatIndex
    ix = IVFFlatIndex.__new__(IVFFlatIndex)
    ix._lib = _NoNative()
    ix._h = None
    ix.dim, ix.nlist, ix.metric, ix.dtype, ix.device, ix.id_base = 8, 16, "cosine", "f16", 0, 0
    return ix


def test_abi_declares_binds_and_exports_ivf_fp8_entry_points():
    from mrag_amd import _native as N
    hdr = (ROOT / "include" / "mrag.h").read_text()
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(mrag_\w+)\(([^;]*)\);", hdr, flags=re.M | re.S)}
    for name, nargs in NEW.items():
        assert name in declared, name
        assert len(declared[name].split(",")) == nargs, name
        assert len(N.SIGNATURES[name]) == nargs, name
    lib = ctypes.CDLL(str(N.lib_path()))
    for name in NEW:
        assert hasattr(lib, name), name
    assert len(declared) + 1 == len(N.SIGNATURES) == 64            # (+ const char* mrag_last_error)
    assert "64 entry points" in (ROOT / "README.md").read_text()


def test_ivf_fp8_argument_checks_before_native():
    ix = _fake_ivf()
    q = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError, match="precision must be one of"):
        ix.search(q, 10, 4, precision="fp16")
    with pytest.raises(ValueError, match="refine applies to precision='fp8' only"):
        ix.search(q, 10, 4, refine=40)
    with pytest.raises(ValueError, match="refine must be positive"):
        ix.search(q, 10, 4, precision="fp8", refine=-1)
    with pytest.raises(ValueError, match="does not combine with allow"):
        ix.search(q, 10, 4, precision="fp8", allow=np.ones(5, dtype=bool))


def test_sharded_ivf_fp8_argument_checks_before_the_local_search():
    from mrag_amd.sharded import ShardedIVFIndex
    calls = []
    sh = ShardedIVFIndex(8, 4, 50, 0, 1, local_search=lambda *a, **kw: calls.append(kw),
                         local_list_counts=lambda m: calls.append("counts"))
    q = np.zeros((2, 8), np.float32)
    with pytest.raises(ValueError, match="does not combine with allow"):
        sh.search(q, 10, 2, precision="fp8", allow=np.ones(50, dtype=bool))
    with pytest.raises(ValueError, match="precision must be one of"):
        sh.search(q, 10, 2, precision="int8")
    with pytest.raises(ValueError, match="refine applies"):
        sh.search(q, 10, 2, refine=20)
    assert calls == []


def test_fp8_keyword_defaults():
    from mrag_amd.index import IVFFlatIndex
    from mrag_amd.sharded import ShardedIVFIndex
    for cls in (IVFFlatIndex, ShardedIVFIndex):
        assert inspect.signature(cls.__init__).parameters["fp8_scan"].default is False
        p = inspect.signature(cls.search).parameters
        assert p["precision"].default == "exact" and p["refine"].default is None
    for name in ("enable_fp8", "rows_fp8", "last_fp8"):
        assert callable(getattr(IVFFlatIndex, name))


WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["MRAG_ROOT"])
import numpy as np, torch.distributed as dist
from mrag_amd.sharded import ShardedIVFIndex, shard_bounds
from oracle import dense_search as ds
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
n, nq, d, k, nlist = 2001, 30, 32, 10, 8
c16 = ds.normalize_round(ds.make_gaussian(n, d, 12)); q16 = ds.normalize_round(ds.make_gaussian(nq, d, 34))
lo, hi = shard_bounds(n, world, rank)
seen = []

def local(queries, kk, npr, **kw):
    seen.append(dict(kw, nprobe=npr))
    v, i = ds.brute_force_topk(np.asarray(queries), c16[lo:hi], kk)
    return v.astype(np.float32), np.where(i >= 0, i + lo, -1)

sh = ShardedIVFIndex(d, nlist, n, rank, world, local_search=local)
want_s, want_i = ds.brute_force_topk(q16, c16, k)
for kw in ({"precision": "fp8", "refine": 33}, {"precision": "fp8"}, {}):
    s_, i_ = sh.search(q16, k, 3, **kw)
    assert (i_ == want_i).all()
    np.testing.assert_allclose(s_, want_s, rtol=0, atol=1e-6)
assert seen == [{"precision": "fp8", "refine": 33, "nprobe": 3}, {"precision": "fp8", "refine": None, "nprobe": 3},
                {"nprobe": 3}], seen                     # (the plain search: exactly the call made before fp8 existed)
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_sharded_ivf_passes_precision_and_refine_through_on_gloo(tmp_path):
    world = 2
    script = tmp_path / "ivf_fp8_ranks.py"
    script.write_text(WORKER)
    env = dict(os.environ, MRAG_ROOT=str(ROOT), MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                        "--master-addr", "127.0.0.1", "--master-port", "29597", str(script)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == world
