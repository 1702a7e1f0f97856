"""The host side of the dense search over per-question allow-sets, and what its GPU tests can see -- no kernel runs here.
The two new C entry points are declared, bound and exported and refuse a dead handle; ``pack_sets`` turns masks and row
positions into the same CSR; the case builders of tests/filter_sets_cases.py hold what tests/test_gpu_filter_sets.py
relies on (fp64 oracle ``oracle.dense_search.brute_force_topk`` over ``c16[set]``); and the backend's new switch is off
unless asked for."""
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import filter_sets_cases as fs
from mrag_amd.backend import DenseRetrievalBackend
from mrag_amd.index import DenseIndex, pack_sets
from oracle import dense_search as ds

ROOT = Path(__file__).resolve().parents[1]
NEW = {"mrag_index_search_sets": 13, "mrag_index_last_sets": 4}


# ------------------------------------------------------------------------------------------------ ABI and binding
def test_abi_declares_binds_and_exports_the_sets_search():
    from mrag_amd import _native as N
    hdr = (ROOT / "include" / "mrag_filter_batch.h").read_text()
    assert '#include "mrag_filter_batch.h"' in (ROOT / "include" / "mrag.h").read_text()
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(mrag_\w+)\(([^;]*)\);", hdr, flags=re.M | re.S)}
    assert set(declared) == set(NEW) == set(N.FILTER_BATCH_SIGNATURES)
    for name, nargs in NEW.items():
        assert len(declared[name].split(",")) == nargs and len(N.FILTER_BATCH_SIGNATURES[name]) == nargs
    # the earlier tables are as they were, and the new names are in none of them
    assert (len(N.SIGNATURES), len(N.EXTENSION_SIGNATURES), len(N.FUSE_BATCH_SIGNATURES), len(N.RERANK_BATCH_SIGNATURES)) == (64, 2, 1, 1)
    assert not set(NEW) & (set(N.SIGNATURES) | set(N.EXTENSION_SIGNATURES) | set(N.FUSE_BATCH_SIGNATURES) | set(N.RERANK_BATCH_SIGNATURES))
    assert "MRAG_ABI_VERSION 1" in (ROOT / "include" / "mrag.h").read_text()
    assert N.lib_path().exists(), "libmrag_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.lib_path())], capture_output=True, text=True).stdout
    assert set(NEW) <= set(re.findall(r"\b(mrag_[a-z0-9_]+)$", out, flags=re.M))
    lib = N.load()
    assert all(getattr(lib, name).argtypes == N.FILTER_BATCH_SIGNATURES[name] for name in NEW)


def test_a_dead_handle_fails_with_a_status_and_a_message():
    from mrag_amd import _native as N
    lib = N.load()
    q, ptr, rows, of = np.ones((1, 8), np.float32), np.asarray([0, 2], np.int64), np.asarray([0, 1], np.int64), np.zeros(1, np.int32)
    sc, ids = np.full((1, 2), 7.0, np.float32), np.full((1, 2), 7, np.int64)
    st = lib.mrag_index_search_sets(0xdead, q.ctypes.data, 1, N.MRAG_F32, 1, 2, 1, ptr.ctypes.data, rows.ctypes.data, of.ctypes.data,
                                    sc.ctypes.data, ids.ctypes.data, None)
    assert st == -1 and b"invalid handle" in lib.mrag_last_error() and (sc == 7.0).all() and (ids == 7).all()
    assert lib.mrag_index_last_sets(0xdead, None, None, None) == -1 and b"invalid handle" in lib.mrag_last_error()


# ------------------------------------------------------------------------------------------------ pack_sets
def test_pack_sets_masks_and_positions_give_the_same_csr():
    n = 100
    masks = [np.arange(n) % 7 == 0, np.zeros(n, dtype=bool), np.arange(n) == n - 1, np.ones(n, dtype=np.uint8)]
    ptr_m, rows_m = pack_sets(masks, n)
    ptr_p, rows_p = pack_sets([np.flatnonzero(m) for m in masks], n)
    assert ptr_m.tolist() == ptr_p.tolist() == [0, 15, 15, 16, 116] and rows_m.tolist() == rows_p.tolist()
    assert ptr_m.dtype == rows_m.dtype == ptr_p.dtype == rows_p.dtype == np.int64
    assert rows_m[:15].tolist() == list(range(0, n, 7)) and rows_m[15] == n - 1


def test_pack_sets_sorts_deduplicates_and_takes_empty_sets():
    ptr, rows = pack_sets([[5, 3, 3, 9, 5], [], np.asarray([], dtype=np.int32), (2,), np.asarray([7, 0], dtype=np.int16)], 10)
    assert ptr.tolist() == [0, 3, 3, 3, 4, 6] and rows.tolist() == [3, 5, 9, 2, 0, 7]
    ptr, rows = pack_sets([], 10)
    assert ptr.tolist() == [0] and rows.shape == (0,) and rows.dtype == np.int64
    ptr, rows = pack_sets([[]], 0)
    assert ptr.tolist() == [0, 0] and rows.shape == (0,)


@pytest.mark.parametrize("bad", [[[10]], [[-1]], [[0, 1], [3, 99]], [np.zeros(9, dtype=bool)], [np.zeros((2, 5), dtype=bool)], [[0.5]]])
def test_pack_sets_refuses_what_is_not_a_set_of_rows(bad):
    with pytest.raises(ValueError):
        pack_sets(bad, 10)


# ------------------------------------------------------------------------------------------------ what the cases hold
def test_the_grid_holds_every_size_sharing_and_edge():
    sets, set_of = fs.grid_layout()
    n = fs.N_GRID
    assert n <= 20000 and n % 256 and len(set_of) < 1000
    assert set(fs.SET_SIZES) <= {len(s) for s in sets}
    per_set = np.bincount(set_of, minlength=len(sets))
    assert set(fs.QUESTIONS_PER_SET) <= set(per_set.tolist()) and (per_set > 0).all()
    assert any(len(s) > 128 and c > 128 for s, c in zip(sets, per_set))          # several row chunks x several question groups
    assert all((np.diff(s) > 0).all() and (len(s) == 0 or (0 <= s[0] and s[-1] < n)) for s in sets)
    assert any(s.tolist() == [0] for s in sets) and any(s.tolist() == [n - 1] for s in sets) and any(s.tolist() == [0, n - 1] for s in sets)
    assert sum(len(s) and s[0] >= n - n % 256 and len(s) > 1 for s in sets) >= 2  # only rows of the partial last tile
    # shared and per-question sets are interleaved in the call, not sorted by set
    assert (np.diff(set_of) < 0).sum() > 100
    # every (size, k) with fewer rows than k is in the grid
    assert {(m, k) for m, k in fs.k_above_m_cases()} >= {(0, 1), (1, 10), (9, 10), (9, 64), (129, 200), (129, 256), (128, 256)}
    assert all(m < k for m, k in fs.k_above_m_cases())


@pytest.mark.parametrize("k", [1, 10, 200])
def test_the_grid_oracle_is_brute_force_over_the_set(k):
    sets, set_of = fs.grid_layout()
    c, q = fs.gaussian_rows(fs.N_GRID, 64, 1), fs.gaussian_rows(len(set_of), 64, 2)
    rv, ri = fs.oracle(q, c, sets, set_of, k, id_base=1000)
    for g in (0, 17, 400, len(set_of) - 1):
        rows = sets[set_of[g]]
        if len(rows) == 0:
            assert np.isneginf(rv[g]).all() and (ri[g] == -1).all()
            continue
        v, i = ds.brute_force_topk(q[g:g + 1], c[rows], k)
        m = min(k, len(rows))
        assert rv[g, :m].tolist() == v[0, :m].tolist() and ri[g, :m].tolist() == (rows[i[0, :m]] + 1000).tolist()
        assert np.isneginf(rv[g, m:]).all() and (ri[g, m:] == -1).all() and (m == k or len(rows) < k)


def test_the_tie_cases_tie_more_than_1024_times_on_the_kth_score():
    c, q, sets, set_of = fs.identical_rows_case()
    assert len(sets[0]) == 2000 and (c[sets[0]] == c[sets[0][0]]).all()
    for k in (1, 10, 256):
        assert (fs.ties_on_kth(q, c, sets[0], k) == 2000).all()
        rv, ri = fs.oracle(q, c, sets, set_of, k)
        assert (ri == sets[0][:k]).all()                                          # ids ascending: the first k of the set
    c, q, sets, set_of = fs.integer_rows_case()
    assert (c == np.round(c)).all() and len(sets[0]) == 4000
    for k in (10, 200, 256):
        t = fs.ties_on_kth(q, c, sets[0], k)
        assert (t > 1024).all() and (t < len(sets[0])).all()                      # the tie is cut by k, and it is not the whole set
        rv, ri = fs.oracle(q, c, sets, set_of, k)
        first = sets[0][sets[0] % 3 == 0][:k]
        assert (ri == first).all() and (rv[0] == 6).all() and (rv[1] == 2).all()


def test_the_position_probe_differs_from_its_neighbours():
    c, pq, pset, fq, fsets, fof = fs.position_case()
    assert len(fq) == fs.B_POS - 1 and len(pset) == 300
    want = fs.oracle(pq, c, [pset], [0], 10)[1][0].tolist()
    for at in (0, fs.B_POS // 2, fs.B_POS - 1):
        q, sets, set_of = fs.place(pq, pset, fq, fsets, fof, at)
        assert len(q) == fs.B_POS and (q[at] == pq[0]).all() and set_of[at] == len(sets) - 1
        rv, ri = fs.oracle(q, c, sets, set_of, 10)
        assert ri[at].tolist() == want
        for nb in (at - 1, at + 1):
            if 0 <= nb < fs.B_POS:
                assert ri[nb].tolist() != want and set_of[nb] != set_of[at]
    # the fillers mix sets of their own with shared ones
    assert len(set(fof.tolist())) > 90 and np.bincount(fof).max() > 60


def test_exact_rows_score_exactly_in_fp32():
    for rows in (fs.pm1_rows(500, 96, 1), fs.small_int_rows(500, 64, 2)):
        s = rows.astype(np.float64) @ rows[:7].astype(np.float64).T
        assert (s == np.round(s)).all() and np.abs(s).max() < 2 ** 20             # integers far below 2^24: exact in any order


def test_the_backend_filter_of_the_tests_returns_three_sets_and_none():
    from mrag_amd.dto import RetrievalIn
    rows = fs.doc_rows()
    got = [fs.three_sets_or_none(RetrievalIn(query=q, graph_id="", top_k=5, trace_id="t"), rows) for q in fs.doc_queries()]
    assert sum(g is None for g in got) >= 3
    packed = {pack_sets([g], len(rows))[1].tobytes() for g in got if g is not None}
    assert len(packed) == 3 and sorted(len(p) // 8 for p in packed) == [200, 300, 400]


# ------------------------------------------------------------------------------------------------ the public interface
def test_the_switch_is_off_by_default_and_the_methods_exist():
    sig = inspect.signature(DenseRetrievalBackend.__init__)
    assert sig.parameters["dense_filter_batch"].default is False

    class R:
        def embed(self, **kw):
            raise AssertionError("not called")
    assert DenseRetrievalBackend(R(), index_path="nowhere.jsonl").dense_filter_batch is False
    assert DenseRetrievalBackend(R(), index_path="nowhere.jsonl", dense_filter_batch=True).dense_filter_batch is True
    assert list(inspect.signature(DenseIndex.search_sets).parameters) == ["self", "queries", "k", "sets", "set_of", "normalize"]
    assert callable(DenseIndex.last_sets)
