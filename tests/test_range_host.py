"""Host-side pieces of the range search: the neighbour-list -> edge step of semantic_edges_index, the Python argument
checks of DenseIndex.range_search / self_join (raised before any native call), the fp32 floor rounding, and the new
symbol in the C ABI."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_neighbor_lists_to_edges_union_max_order():
    from mrag_amd.pairwise import neighbor_lists_to_edges
    # row 0 lists 2 and 1; row 1 lists 0 (higher score); row 2 lists nothing; row 3 lists 1 and itself
    ids = np.array([[12, 11, -1], [10, -1, -1], [-1, -1, -1], [11, 13, -1]], dtype=np.int64)
    sc = np.array([[0.95, 0.91, -np.inf], [0.93, -np.inf, -np.inf], [-np.inf] * 3, [0.97, 1.0, -np.inf]], dtype=np.float32)
    edges = neighbor_lists_to_edges(sc, ids, id_base=10)
    assert [(i, j) for i, j, _ in edges] == [(0, 1), (0, 2), (1, 3)]
    sims = {(i, j): v for i, j, v in edges}
    assert sims[(0, 1)] == pytest.approx(float(np.float32(0.93)))   # the larger direction
    assert sims[(0, 2)] == pytest.approx(float(np.float32(0.95)))
    assert sims[(1, 3)] == pytest.approx(float(np.float32(0.97)))
    assert all(isinstance(i, int) and isinstance(j, int) and isinstance(v, float) for i, j, v in edges)


def test_neighbor_lists_to_edges_matches_dense_rule():
    from mrag_amd.pairwise import neighbor_lists_to_edges
    rng = np.random.default_rng(3)
    n, k = 40, 6
    S = rng.random((n, n)).astype(np.float32)
    np.fill_diagonal(S, -np.inf)
    ids = np.argsort(-S, axis=1, kind="stable")[:, :k]
    sc = np.take_along_axis(S, ids, axis=1)
    edges = neighbor_lists_to_edges(sc, ids)
    want = {}
    for r in range(n):
        for c, v in zip(ids[r], sc[r]):
            key = (min(r, c), max(r, c))
            want[key] = max(want.get(key, -np.inf), float(v))
    assert [(i, j) for i, j, _ in edges] == sorted(want)
    assert all(v == want[(i, j)] for i, j, v in edges)
    assert neighbor_lists_to_edges(np.full((3, 2), -np.inf, np.float32), np.full((3, 2), -1)) == []
    with pytest.raises(ValueError):
        neighbor_lists_to_edges(np.zeros((3, 2)), np.zeros((3, 3), dtype=np.int64))


def test_range_floor_rounding():
    from mrag_amd.index import range_floor
    f = range_floor(0.9)
    assert f.dtype == np.float32 and float(f) >= 0.9 and float(np.nextafter(f, np.float32(-np.inf))) < 0.9
    assert range_floor(0.5) == np.float32(0.5) and range_floor(-2) == np.float32(-2.0)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39, "0.5", None, True):
        with pytest.raises(ValueError):
            range_floor(bad)


class _NoNative:
    """stands in for the library: any native call fails the test"""
    def __getattr__(self, name):
        if name == "mrag_index_max_k":
            def max_k(nq, out):
                out._obj.value = 256
                return 0
            return max_k
        raise AssertionError(f"native call {name} reached")


def _fake_index():
    from mrag_amd.index import DenseIndex
    ix = DenseIndex.__new__(DenseIndex)
    ix._lib = _NoNative()
    ix._h = None
    ix.dim, ix.metric, ix.dtype, ix.device, ix.id_base = 8, "cosine", "f16", 0, 0
    return ix


def test_range_search_argument_checks_before_native():
    ix = _fake_index()
    q = np.zeros((2, 8), np.float32)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            ix.range_search(q, bad, 10)
    for k in (0, -3, 257, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            ix.range_search(q, 0.5, k)
    with pytest.raises(ValueError, match="fp8"):
        ix.range_search(q, 0.5, 10, precision="fp8")
    with pytest.raises(ValueError):
        ix.range_search(q, 0.5, 10, precision="fp4")
    with pytest.raises(ValueError, match="filter_path"):
        ix.range_search(q, 0.5, 10, filter_path="nope")
    with pytest.raises(ValueError, match="finite"):
        ix.self_join(float("nan"))
    with pytest.raises(ValueError, match="k must be"):
        ix.self_join(0.9, k=256)
    with pytest.raises(ValueError, match="batch"):
        ix.self_join(0.9, k=8, batch=0)


def test_abi_declares_and_binds_search_range():
    from mrag_amd import _native as N
    hdr = (ROOT / "include" / "mrag.h").read_text()
    assert re.search(r"\bint mrag_index_search_range\(", hdr)
    assert "mrag_index_search_range" in N.SIGNATURES
    assert len(N.SIGNATURES["mrag_index_search_range"]) == 18
