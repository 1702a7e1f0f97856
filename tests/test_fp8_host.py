"""CPU tests of the fp8 scan's host side: the new C entry points are declared, bound and exported, the default refine
pool is computed without a GPU, and DenseIndex.search rejects bad precision / refine / allow combinations before any
library call."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
FP8_SYMBOLS = {"mrag_index_enable_fp8", "mrag_index_get_rows_fp8", "mrag_index_fp8_default_refine",
               "mrag_index_search_fp8", "mrag_index_last_fp8"}


def test_fp8_symbols_declared_bound_exported():
    from mrag_amd import _native as N
    header = (ROOT / "include" / "mrag.h").read_text()
    declared = set(re.findall(r"\bint\s+(mrag_\w+)\s*\(", header))
    assert FP8_SYMBOLS <= declared
    assert FP8_SYMBOLS <= set(N.SIGNATURES)
    lib = N.load()
    for name in FP8_SYMBOLS:
        assert getattr(lib, name) is not None
    assert "MRAG_FP8_BATCH = 0" in header and "MRAG_FP8_STREAM = 1" in header
    assert (N.FP8_BATCH, N.FP8_STREAM) == (0, 1)


@pytest.mark.parametrize("k,want", [(1, 40), (10, 40), (11, 44), (15, 60), (16, 64), (64, 64)])
def test_fp8_default_refine(k, want):
    from mrag_amd.index import fp8_default_refine
    assert fp8_default_refine(k) == want


@pytest.mark.parametrize("k", [0, 65, -1])
def test_fp8_default_refine_rejects(k):
    from mrag_amd import _native as N
    from mrag_amd.index import fp8_default_refine
    with pytest.raises(N.MragError) as e:
        fp8_default_refine(k)
    assert e.value.code == -1                     # MRAG_ERR_INVALID


def _unbound_index():
    """A DenseIndex with no library handle: the argument checks below must fire before any library call."""
    from mrag_amd.index import DenseIndex
    ix = DenseIndex.__new__(DenseIndex)
    ix.dim, ix.metric, ix.dtype, ix.device = 8, "cosine", "f16", 0
    ix._h = None
    return ix


def test_search_precision_checks_raise_value_error():
    ix = _unbound_index()
    q = np.ones((2, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="precision"):
        ix.search(q, 4, precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        ix.search(q, 4, precision=None)
    with pytest.raises(ValueError, match="allow"):
        ix.search(q, 4, precision="fp8", allow=np.ones(10, dtype=bool))
    with pytest.raises(ValueError, match="refine"):
        ix.search(q, 4, refine=40)                # refine without precision="fp8"
    with pytest.raises(ValueError, match="refine"):
        ix.search(q, 4, precision="fp8", refine=-3)


def test_sharded_forwards_fp8_scan():
    import inspect
    from mrag_amd.sharded import ShardedDenseIndex
    from mrag_amd.index import DenseIndex
    assert inspect.signature(ShardedDenseIndex.__init__).parameters["fp8_scan"].default is False
    assert inspect.signature(DenseIndex.__init__).parameters["fp8_scan"].default is False
    p = inspect.signature(DenseIndex.search).parameters
    assert p["precision"].default == "exact" and p["refine"].default is None
