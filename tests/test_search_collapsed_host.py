"""The host side of the collapsed dense search, and what its GPU tests can see -- no kernel runs here.  The three new C entry
points are declared, bound and exported and refuse a dead handle; the exactness argument behind
``mrag_index_search_collapsed`` -- the rounds of ``search_collapsed_cases.collapse_rounds`` over an exact top-``scan_k``
give the fp64 brute force over all rows, ties included, in at most k + 1 rounds -- is checked by brute force;
``row_keys_of`` and ``collapse_scan_k`` hold their edge values; the case builders hold what
tests/test_gpu_search_collapsed.py relies on; and the backend's new argument is off unless asked for."""
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import search_collapsed_cases as sc
from mrag_amd.backend import DenseRetrievalBackend
from mrag_amd.index import DenseIndex, collapse_scan_k, row_keys_of

ROOT = Path(__file__).resolve().parents[1]
NEW = {"mrag_index_set_row_keys": 4, "mrag_index_search_collapsed": 13, "mrag_index_last_collapsed": 6}


# ------------------------------------------------------------------------------------------------ ABI and binding
def test_abi_declares_binds_and_exports_the_collapsed_search():
    from mrag_amd import _native as N
    hdr = (ROOT / "include" / "mrag_search_collapsed.h").read_text()
    assert '#include "mrag_search_collapsed.h"' in (ROOT / "include" / "mrag.h").read_text()
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(mrag_\w+)\(([^;]*)\);", hdr, flags=re.M | re.S)}
    assert set(declared) == set(NEW) == set(N.SEARCH_COLLAPSED_SIGNATURES)
    for name, nargs in NEW.items():
        assert len(declared[name].split(",")) == nargs and len(N.SEARCH_COLLAPSED_SIGNATURES[name]) == nargs
    assert "synchronises `stream` at least once" in hdr                       # stated where the call is declared
    # the earlier tables are as they were, and the new names are in none of them
    earlier = (N.SIGNATURES, N.EXTENSION_SIGNATURES, N.FUSE_BATCH_SIGNATURES, N.RERANK_BATCH_SIGNATURES, N.FILTER_BATCH_SIGNATURES,
               N.SEARCH_GROUPS_SIGNATURES)
    assert tuple(len(t) for t in earlier) == (64, 2, 1, 1, 2, 2)
    assert not any(set(NEW) & set(t) for t in earlier)
    assert "MRAG_ABI_VERSION 1" in (ROOT / "include" / "mrag.h").read_text()
    assert N.lib_path().exists(), "libmrag_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.lib_path())], capture_output=True, text=True).stdout
    assert set(NEW) <= set(re.findall(r"\b(mrag_[a-z0-9_]+)$", out, flags=re.M))
    lib = N.load()
    assert all(getattr(lib, name).argtypes == N.SEARCH_COLLAPSED_SIGNATURES[name] for name in NEW)


def test_a_dead_handle_fails_with_a_status_and_a_message():
    from mrag_amd import _native as N
    lib = N.load()
    q, keys = np.ones((2, 8), np.float32), np.zeros(2, np.int32)
    s, i, k = np.full((2, 2), 7.0, np.float32), np.full((2, 2), 7, np.int64), np.full((2, 2), 7, np.int32)
    st = lib.mrag_index_search_collapsed(0xdead, q.ctypes.data, 2, N.MRAG_F32, 1, 0, 2, 0, s.ctypes.data, i.ctypes.data,
                                         k.ctypes.data, 0, None)
    assert st == -1 and b"invalid handle" in lib.mrag_last_error()
    assert (s == 7.0).all() and (i == 7).all() and (k == 7).all()
    assert lib.mrag_index_set_row_keys(0xdead, keys.ctypes.data, 2, 0) == -1 and b"invalid handle" in lib.mrag_last_error()
    assert lib.mrag_index_last_collapsed(0xdead, None, None, None, None, None) == -1 and b"invalid handle" in lib.mrag_last_error()


# ------------------------------------------------------------------------------------------------ the host helpers
def test_row_keys_of_numbers_the_values_in_order_of_first_appearance():
    keys, n_keys, m = row_keys_of(["b", "a", "b", ("t", 1), "a", "b"])
    assert keys.tolist() == [0, 1, 0, 2, 1, 0] and keys.dtype == np.int32 and (n_keys, m) == (3, 3)
    keys, n_keys, m = row_keys_of([])
    assert keys.shape == (0,) and keys.dtype == np.int32 and (n_keys, m) == (0, 0)
    keys, n_keys, m = row_keys_of(range(5))
    assert keys.tolist() == [0, 1, 2, 3, 4] and (n_keys, m) == (5, 1)
    keys, n_keys, m = row_keys_of([None] * 4)                                  # a missing field is one key
    assert keys.tolist() == [0] * 4 and (n_keys, m) == (1, 4)
    titles = [f"Title {i // 4}" for i in range(800)]
    keys, n_keys, m = row_keys_of(titles)
    assert (keys == np.arange(800) // 4).all() and (n_keys, m) == (200, 4)


def test_collapse_scan_k_edge_values():
    assert collapse_scan_k(10, 1, 5000) == 10                                  # m = 1: the plain search's depth
    assert collapse_scan_k(1, 300, 5000) == 1                                  # one key wanted: its best row leads
    assert collapse_scan_k(10, 3, 5000) == 28                                  # (k - 1) m + 1
    assert collapse_scan_k(10, 4, 5000) == 37
    assert collapse_scan_k(10, 29, 5000) == 256 == collapse_scan_k(200, 4, 5000) == collapse_scan_k(256, 1, 5000)   # the cap
    assert collapse_scan_k(10, 28, 5000) == 253
    assert collapse_scan_k(10, 4, 30) == 30                                    # cap at n
    assert collapse_scan_k(10, 4, 10) == 10
    assert collapse_scan_k(10, 4, 3) == 10 == collapse_scan_k(10, 0, 0)        # never below k
    for k in (0, 257, True, 2.0):
        with pytest.raises(ValueError):
            collapse_scan_k(k, 1, 100)


# ------------------------------------------------------------------------------------------------ the exactness argument
def test_collapse_rounds_on_a_case_worked_by_hand():
    #        row:  0    1    2    3    4    5    6
    s = np.asarray([[9.0, 9.0, 8.0, 8.0, 7.0, 7.0, 1.0]], dtype=np.float32)
    keys = np.asarray([4, 4, 4, 2, 4, 9, 2], dtype=np.int32)
    got = sc.collapse_rounds(sc.exact_search_fn(s, 3), 1, keys, 3, 3)
    # round 0 sees rows 0 1 2 (key 4 only); round 1 sees rows 3 5 6 (keys 2 9 2): complete
    assert got[1].tolist() == [[0, 3, 5]] and got[0].tolist() == [[9.0, 8.0, 7.0]] and got[2].tolist() == [[4, 2, 9]]
    assert got[3].tolist() == [2]
    assert got[0].dtype == np.float32 and got[1].dtype == np.int64 and got[2].dtype == np.int32
    # three keys, k = 5: tails.  A list of 8 shows that all 7 rows were seen; a FULL list of 7 does not, and the redo finds nothing
    for scan_k, rounds in ((8, 1), (7, 2)):
        got = sc.collapse_rounds(sc.exact_search_fn(s, scan_k, id_base=100), 1, keys, 5, scan_k, id_base=100)
        assert got[1].tolist() == [[100, 103, 105, -1, -1]] and got[2].tolist() == [[4, 2, 9, -1, -1]] and got[3].tolist() == [rounds]
        assert np.isneginf(got[0][0, 3:]).all()
    got = sc.collapse_rounds(sc.exact_search_fn(s, 2), 1, keys, 2, 2)          # a redo that meets its key at once
    assert got[1].tolist() == [[0, 3]] and got[3].tolist() == [2]


FAMILIES = {"distinct": sc.LAYOUTS["distinct"], "one_key": sc.LAYOUTS["one_key"], "runs2": sc.runs(2), "runs5": sc.runs(5),
            "interleaved3": sc.interleaved(3), "interleaved7": sc.interleaved(7), "big_values": sc.LAYOUTS["big_values"]}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_rounds_give_the_brute_force_over_all_rows_in_at_most_k_plus_1_rounds(family):
    """the exactness argument, by brute force: small integer scores (many ties), every 1 <= k <= scan_k <= k + 9"""
    n, nq, dim = 37, 4, 2
    c, q = sc.small_int_rows(n, dim, 11), sc.small_int_rows(nq, dim, 12)
    s = q.astype(np.float64) @ c.astype(np.float64).T
    assert all(len(np.unique(row)) < n / 2 for row in s)                      # many ties under every query
    keys = FAMILIES[family](n)
    most = 0
    for k in range(1, n + 3):
        want = sc.oracle_collapsed(q, c, keys, k, id_base=50)
        for scan_k in range(k, k + 10):
            got = sc.collapse_rounds(sc.exact_search_fn(s, scan_k, id_base=50), nq, keys, k, scan_k, id_base=50)
            assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist(), (family, k, scan_k)
            assert got[0].tobytes() == want[0].astype(np.float32).tobytes()
            assert got[3].min() >= 1 and got[3].max() <= k + 1, (family, k, scan_k, got[3].tolist())
            most = max(most, int(got[3].max()))
            if scan_k >= (k - 1) * row_keys_of(keys.tolist())[2] + 1:
                assert got[3].max() == 1                                       # the depth behind the default never needs a redo
    assert (most > 1) == (family not in ("distinct",))


def test_the_oracle_is_brute_force_over_the_best_row_of_every_key():
    c, q = sc.gaussian_rows(500, 64, 1), sc.gaussian_rows(3, 64, 2)
    keys = sc.interleaved(40)(500)
    rv, ri, rk = sc.oracle_collapsed(q, c, keys, 45, id_base=50)
    s = q.astype(np.float64) @ c.astype(np.float64).T
    for g in range(3):
        best = {}
        for r in range(500):
            if keys[r] not in best or s[g, r] > s[g, best[keys[r]]]:
                best[int(keys[r])] = r
        order = sorted(best.values(), key=lambda r: (-s[g, r], r))
        assert ri[g, :40].tolist() == [r + 50 for r in order] and rk[g, :40].tolist() == [int(keys[r]) for r in order]
        assert rv[g, :40].tolist() == [s[g, r] for r in order]
        assert (ri[g, 40:] == -1).all() and (rk[g, 40:] == -1).all() and np.isneginf(rv[g, 40:]).all()
    rv, ri, rk = sc.oracle_collapsed(q, c[:0], keys[:0], 3)
    assert (ri == -1).all() and (rk == -1).all() and np.isneginf(rv).all()


# ------------------------------------------------------------------------------------------------ what the cases hold
def test_the_layouts_cross_tile_and_wave_boundaries():
    n = sc.N_EXACT
    assert n == 7 * 256 + 211
    for name, fn in sc.LAYOUTS.items():
        keys = fn(n)
        assert keys.dtype == np.int32 and keys.shape == (n,) and keys.min() >= 0, name
    assert len(np.unique(sc.LAYOUTS["distinct"](n))) == n and len(np.unique(sc.LAYOUTS["one_key"](n))) == 1
    for m in (3, 7, 300):                                                      # a run that holds rows of two 256-row tiles
        keys = sc.runs(m)(n)
        assert any(keys[t * 256 - 1] == keys[t * 256] for t in range(1, 8)), m
        assert np.bincount(keys).max() == m
    assert len(np.unique(sc.interleaved(257)(n))) == 257 > 256 and sc.interleaved(257)(n)[257] == 0
    big = sc.LAYOUTS["big_values"](n)
    assert big.max() == 2 ** 31 - 1 and np.bincount(row_keys_of(big.tolist())[0]).max() == 3 and np.diff(np.unique(big)).min() > 10 ** 6
    # the lists end before, at and behind entry 63 / 64, the last entry a 64-bit ballot's first wave holds
    scans = {s for _, s in sc.K_SCAN}
    assert {63, 64, 65} <= scans and {1, 255, 256} <= scans and any(k == s for k, s in sc.K_SCAN) and max(k for k, _ in sc.K_SCAN) == 256
    assert set(sc.NQS) == {8, 16, 17, 44}


def test_exact_rows_score_exactly_and_heads_stand_behind_entry_63():
    from filter_sets_cases import round_bf16
    for dim in sc.DIMS:
        c, q = sc.exact_case(dim, 8)
        s = q.astype(np.float64) @ c.astype(np.float64).T
        assert (s == np.round(s)).all() and np.abs(s).max() < 2 ** 20
        assert (round_bf16(c.astype(np.float32)) == c.astype(np.float32)).all()
    # under runs of 7 a list of 255 entries holds heads in every one of its four waves, and duplicates of keys met in an
    # EARLIER wave: what a 32-bit ballot or a test that looks only inside the own wave would get wrong
    c, q = sc.exact_case(96, 8)
    s = (q.astype(np.float64) @ c.astype(np.float64).T).astype(np.float32)
    keys = sc.runs(7)(sc.N_EXACT)
    lists = sc.exact_search_fn(s, 255)(list(range(8)), None)[1]
    for row in lists:
        kk = keys[row]
        first = np.asarray([kk[e] not in kk[:e] for e in range(255)])
        assert all(first[w * 64:(w + 1) * 64].any() for w in range(4)) and first[32:64].any()
        assert any((not first[e]) and kk[e] in kk[:64] for e in range(64, 255))


def test_the_redo_case_forces_a_redo_for_every_probe_and_none_for_the_fillers():
    c, keys, probes, fill = sc.redo_case()
    assert (c[600:900] == c[700]).all() and (keys[600:900] == sc.REDO_KEY).all() and (probes == c[700]).all()
    rest = np.delete(keys, np.arange(600, 900))
    assert sc.REDO_KEY not in rest and np.bincount(rest).max() == 3
    q = np.concatenate([probes, fill])
    s = (q.astype(np.float64) @ c.astype(np.float64).T).astype(np.float32)
    assert (s[:3, 600:900] == 64).all() and (np.delete(s[:3], np.arange(600, 900), axis=1) < 64).all()
    assert (s[3:, 700] <= 0).all()
    for k, scan_k in sc.REDO_K_SCAN:
        got = sc.collapse_rounds(sc.exact_search_fn(s, scan_k), len(q), keys, k, scan_k)
        assert (got[3][:3] >= 2).all() and (got[3][3:] == 1).all(), (k, scan_k, got[3].tolist())
        want = sc.oracle_collapsed(q, c, keys, k)
        assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
        assert (got[2][:3, 0] == sc.REDO_KEY).all() and (got[1][:3, 0] == 600).all()
    assert sc.place(probes[:1], fill, 5).shape == (len(fill) + 1, 64) and (sc.place(probes[:1], fill, 5)[5] == probes[0]).all()


def test_the_gaussian_cases_need_exactly_one_round():
    for dim in sc.DIMS:
        c, keys, q = sc.gaussian_case(dim, nq=6)
        scan_k = collapse_scan_k(sc.GAUSS_K, sc.GAUSS_M, len(c))
        assert scan_k == 28 and np.bincount(keys).max() == sc.GAUSS_M
        s = (q.astype(np.float64) @ c.astype(np.float64).T).astype(np.float32)
        got = sc.collapse_rounds(sc.exact_search_fn(s, scan_k), len(q), keys, sc.GAUSS_K, scan_k)
        assert (got[3] == 1).all() and (got[1] >= 0).all()


# ------------------------------------------------------------------------------------------------ the public interface
class _NoRouter:
    def embed(self, **kw):
        raise AssertionError("not called")


def test_the_new_argument_is_off_by_default_and_the_methods_exist():
    sig = inspect.signature(DenseRetrievalBackend.__init__)
    assert sig.parameters["dense_collapse"].default is None
    kw = dict(index_path="nowhere.jsonl")
    assert DenseRetrievalBackend(_NoRouter(), **kw).dense_collapse is None
    assert DenseRetrievalBackend(_NoRouter(), dense_collapse="title", **kw).dense_collapse == "title"
    assert DenseRetrievalBackend(_NoRouter(), dense_collapse=sc.title_of, **kw).dense_collapse is sc.title_of
    assert DenseRetrievalBackend(_NoRouter(), dense_collapse="search_collapsed_cases:title_of", **kw).dense_collapse is sc.title_of
    with pytest.raises(TypeError):
        DenseRetrievalBackend(_NoRouter(), dense_collapse=3, **kw)
    for bad in (dict(dense_mode="rerank"), dict(dense_row_filter=lambda req, rows: None),
                dict(query_expander=lambda **k: [], dense_expanded=True)):
        with pytest.raises(ValueError):
            DenseRetrievalBackend(_NoRouter(), dense_collapse="title", **kw, **bad)
    DenseRetrievalBackend(_NoRouter(), dense_collapse="title", query_expander=lambda **k: [], **kw)   # the text channel's expander is fine
    assert list(inspect.signature(DenseIndex.search_collapsed).parameters) == [
        "self", "queries", "k", "scan_k", "normalize", "stream", "out", "return_keys"]
    assert callable(DenseIndex.set_row_keys) and callable(DenseIndex.last_collapsed)


def test_run_without_dense_collapse_is_unchanged():
    """no corpus file: the dense channel degrades, the text channel is an injected searcher"""
    from mrag_amd.dto import RetrievalIn

    def text_search(*, queries, top_k):
        return [{"id": f"d{len(q)}", "score": float(len(q)), "meta": {"text": q}} for q in queries]
    req = RetrievalIn(query="alpha beta gamma", graph_id="", top_k=3, trace_id="t")
    plain = DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", text_search=text_search).run(req)
    off = DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", text_search=text_search, dense_collapse=None).run(req)
    assert off == plain and "dense_collapse" not in plain["diagnostics"]
    on = DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", text_search=text_search, dense_collapse="title")
    for got in (on.run(req), on.run_batch([req])[0]):                         # no rows: nothing to collapse, the text hits stand
        assert got["hits"] == plain["hits"] and "dense_collapse" not in got["diagnostics"]
