"""Host-side pieces of the IVF range search: the Python argument checks of IVFFlatIndex.range_search / self_join (raised
before any native call), the new symbols in the C ABI, and the nprobe pass-through of semantic_edges_index."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


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


def test_ivf_range_search_argument_checks_before_native():
    ix = _fake_ivf()
    q = np.zeros((2, 8), np.float32)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            ix.range_search(q, bad, 10, 4)
    for bad in ("0.5", None, True):
        with pytest.raises(ValueError, match="real number"):
            ix.range_search(q, bad, 10, 4)
    for k in (0, -3, 257, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            ix.range_search(q, 0.5, k, 4)
    for nprobe in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="nprobe"):
            ix.range_search(q, 0.5, 10, nprobe)
    with pytest.raises(ValueError, match="exclude"):
        ix.range_search(q, 0.5, 10, 4, exclude=np.zeros((2, 1), dtype=np.int64))     # 2-D
    with pytest.raises(ValueError, match="exclude"):
        ix.range_search(q, 0.5, 10, 4, exclude=np.zeros(3, dtype=np.int64))          # one row per query
    with pytest.raises(ValueError, match="exclude"):
        ix.range_search(q, 0.5, 10, 4, exclude=np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="exclude"):
        ix.range_search(q, 0.5, 10, 4, exclude=np.array([0, -2]))
    with pytest.raises(TypeError):
        ix.range_search(q, 0.5, 10, 4, allow=np.ones(4, dtype=bool))                  # no allow-set form


def test_ivf_self_join_argument_checks_before_native():
    ix = _fake_ivf()
    with pytest.raises(ValueError, match="finite"):
        ix.self_join(float("nan"), 4)
    with pytest.raises(ValueError, match="real number"):
        ix.self_join("0.9", 4)
    for k in (0, 257, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            ix.self_join(0.9, 4, k=k)
    with pytest.raises(ValueError, match="nprobe"):
        ix.self_join(0.9, 0)
    for batch in (0, -5, 1.5, True):
        with pytest.raises(ValueError, match="batch"):
            ix.self_join(0.9, 4, k=8, batch=batch)


def test_abi_declares_and_binds_ivf_range_entry_points():
    from mrag_amd import _native as N
    hdr = (ROOT / "include" / "mrag.h").read_text()
    assert re.search(r"\bint mrag_ivf_search_range\(", hdr) and re.search(r"\bint mrag_ivf_self_join\(", hdr)
    assert len(N.SIGNATURES["mrag_ivf_search_range"]) == 16
    assert len(N.SIGNATURES["mrag_ivf_self_join"]) == 10
    # every declaration of the header is bound and the other way round
    declared = set(re.findall(r"^(?:int|const char\*)\s+(mrag_\w+)\(", hdr, flags=re.M))
    assert {"mrag_ivf_search_range", "mrag_ivf_self_join"} <= declared
    assert declared == set(N.SIGNATURES)
    assert "edge_builder.py:146-169" in hdr[hdr.index("mrag_ivf_search_range") - 2500:hdr.index("mrag_ivf_self_join")]


class _StubJoin:
    def __init__(self):
        self.calls, self.id_base = [], 5

    def self_join(self, *args, **kw):
        self.calls.append((args, kw))
        sc = np.array([[0.95, -np.inf], [0.95, -np.inf], [-np.inf, -np.inf]], dtype=np.float32)
        ids = np.array([[6, -1], [5, -1], [-1, -1]], dtype=np.int64)
        cnt = np.array([1, 3, 0], dtype=np.int64)

        class _T:
            def __init__(self, a):
                self.a = a

            def cpu(self):
                return self

            def numpy(self):
                return self.a
        return _T(sc), _T(ids), _T(cnt)


def test_semantic_edges_index_passes_nprobe_through():
    from mrag_amd.pairwise import semantic_edges_index
    ivf = _StubJoin()
    edges, trunc = semantic_edges_index(ivf, 0.9, k=2, batch=100, nprobe=7)
    assert ivf.calls == [((0.9, 7), {"k": 2, "batch": 100})]
    assert [(i, j) for i, j, _ in edges] == [(0, 1)] and trunc.tolist() == [1]
    dense = _StubJoin()
    edges, trunc = semantic_edges_index(dense, 0.9, k=2, batch=100)
    assert dense.calls == [((0.9,), {"k": 2, "batch": 100})]          # exactly the call made before nprobe existed
    assert [(i, j) for i, j, _ in edges] == [(0, 1)] and trunc.tolist() == [1]
