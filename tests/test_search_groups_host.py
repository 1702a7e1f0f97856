"""The host side of the grouped dense search, and what its GPU tests can see -- no kernel runs here.  The two new C entry
points are declared, bound and exported and refuse a dead handle; ``group_ptr_of`` turns sizes into ``group_ptr``; the
exactness argument behind ``mrag_index_search_groups`` -- the union of the per-query top-k lists holds the top-k of the
row-wise maximum, ties included -- is checked by brute force through the host restatement
``search_groups_cases.merge_groups``; the case builders hold what tests/test_gpu_search_groups.py relies on; and the
backend's new arguments are off unless asked for."""
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import search_groups_cases as sg
from mrag_amd.backend import DenseRetrievalBackend
from mrag_amd.index import DenseIndex, group_ptr_of

ROOT = Path(__file__).resolve().parents[1]
NEW = {"mrag_index_search_groups": 17, "mrag_index_last_groups": 4}


# ------------------------------------------------------------------------------------------------ ABI and binding
def test_abi_declares_binds_and_exports_the_grouped_search():
    from mrag_amd import _native as N
    hdr = (ROOT / "include" / "mrag_search_groups.h").read_text()
    assert '#include "mrag_search_groups.h"' in (ROOT / "include" / "mrag.h").read_text()
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(mrag_\w+)\(([^;]*)\);", hdr, flags=re.M | re.S)}
    assert set(declared) == set(NEW) == set(N.SEARCH_GROUPS_SIGNATURES)
    for name, nargs in NEW.items():
        assert len(declared[name].split(",")) == nargs and len(N.SEARCH_GROUPS_SIGNATURES[name]) == nargs
    # the earlier tables are as they were, and the new names are in none of them
    earlier = (N.SIGNATURES, N.EXTENSION_SIGNATURES, N.FUSE_BATCH_SIGNATURES, N.RERANK_BATCH_SIGNATURES, N.FILTER_BATCH_SIGNATURES)
    assert tuple(len(t) for t in earlier) == (64, 2, 1, 1, 2)
    assert not any(set(NEW) & set(t) for t in earlier)
    assert "MRAG_ABI_VERSION 1" in (ROOT / "include" / "mrag.h").read_text()
    assert N.lib_path().exists(), "libmrag_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.lib_path())], capture_output=True, text=True).stdout
    assert set(NEW) <= set(re.findall(r"\b(mrag_[a-z0-9_]+)$", out, flags=re.M))
    lib = N.load()
    assert all(getattr(lib, name).argtypes == N.SEARCH_GROUPS_SIGNATURES[name] for name in NEW)


def test_a_dead_handle_fails_with_a_status_and_a_message():
    from mrag_amd import _native as N
    lib = N.load()
    q, ptr = np.ones((2, 8), np.float32), np.asarray([0, 2], np.int64)
    sc, ids, wh = np.full((1, 2), 7.0, np.float32), np.full((1, 2), 7, np.int64), np.full((1, 2), 7, np.int32)
    st = lib.mrag_index_search_groups(0xdead, q.ctypes.data, 2, N.MRAG_F32, 1, 0, 2, 1, ptr.ctypes.data, None, 0, 0,
                                      sc.ctypes.data, ids.ctypes.data, wh.ctypes.data, 0, None)
    assert st == -1 and b"invalid handle" in lib.mrag_last_error()
    assert (sc == 7.0).all() and (ids == 7).all() and (wh == 7).all()
    assert lib.mrag_index_last_groups(0xdead, None, None, None) == -1 and b"invalid handle" in lib.mrag_last_error()


# ------------------------------------------------------------------------------------------------ group_ptr_of
def test_sizes_become_group_ptr():
    assert group_ptr_of(None, [2, 0, 5, 1], 8).tolist() == [0, 2, 2, 7, 8]
    assert group_ptr_of(None, np.asarray([3], dtype=np.int32), 3).tolist() == [0, 3]
    assert group_ptr_of(None, [], 0).tolist() == [0]
    assert group_ptr_of(None, [0, 0], 0).tolist() == [0, 0, 0]
    p = group_ptr_of([0, 2, 2, 7], None, 7)
    assert p.tolist() == [0, 2, 2, 7] and p.dtype == np.int64 and p.flags.c_contiguous
    assert group_ptr_of(None, [2, 5], 7).dtype == np.int64
    assert sg.ptr_of([2, 0, 5, 1]).tolist() == [0, 2, 2, 7, 8]


@pytest.mark.parametrize("gp,sizes,nq", [(None, None, 3), ([0, 3], [3], 3), ([1, 3], None, 3), ([0, 2, 1, 3], None, 3), ([0, 2], None, 3),
                                         (None, [2, 2], 3), (None, [4, -1], 3), ([], None, 0), ([[0, 3]], None, 3), ([0.0, 3.0], None, 3),
                                         (None, [True, True], 2)])
def test_group_ptr_of_refuses_what_is_not_a_partition_of_the_queries(gp, sizes, nq):
    with pytest.raises(ValueError):
        group_ptr_of(gp, sizes, nq)


# ------------------------------------------------------------------------------------------------ the restatement
def test_merge_groups_on_a_case_worked_by_hand():
    inf = np.inf
    #            query 0                    query 1                      query 2 (another question)
    sc = [[5.0, 3.0, 3.0, -inf], [7.0, 5.0, 3.0, 1.0], [2.0, -inf, -inf, -inf]]
    ids = [[4, 2, 9, -1], [9, 4, 1, 8], [6, -1, -1, -1]]
    s, i, w = sg.merge_groups(sc, ids, [0, 2, 2, 3], 4)
    assert i.tolist() == [[9, 4, 1, 2], [-1] * 4, [6, -1, -1, -1]]
    assert s[0].tolist() == [7.0, 5.0, 3.0, 3.0] and np.isneginf(s[1]).all() and s[2, 0] == 2.0 and np.isneginf(s[2, 1:]).all()
    assert w.tolist() == [[1, 0, 1, 0], [-1] * 4, [0, -1, -1, -1]]           # id 4 ties at 5.0: the lower query position
    assert s.dtype == np.float32 and i.dtype == np.int64 and w.dtype == np.int32
    s, i, w = sg.merge_groups(sc, ids, [0, 2, 2, 3], 6)                      # five distinct ids in question 0
    assert i[0].tolist() == [9, 4, 1, 2, 8, -1] and w[0].tolist() == [1, 0, 1, 0, 1, -1]


def test_merge_groups_compares_signed_zeros_as_floats():
    nz, pz = np.float32(-0.0), np.float32(0.0)
    for first, second in ((nz, pz), (pz, nz)):
        s, i, w = sg.merge_groups([[first, -1.0], [second, -1.0]], [[3, 5], [3, 5]], [0, 2], 2)
        assert i.tolist() == [[3, 5]] and w.tolist() == [[0, 0]]
        assert np.signbit(s[0, 0]) == np.signbit(first)                       # the first one met stays, with its own bits
    # zeros of either sign tie: id ascending decides
    s, i, w = sg.merge_groups([[pz], [nz]], [[8], [2]], [0, 2], 2)
    assert i.tolist() == [[2, 8]] and w.tolist() == [[1, 0]] and np.signbit(s[0, 0]) and not np.signbit(s[0, 1])


@pytest.mark.parametrize("seed", range(6))
def test_the_union_of_the_per_query_lists_holds_the_merged_top_k(seed):
    """the exactness argument, by brute force: small integer scores (many ties), every k"""
    rng = np.random.default_rng(seed)
    q, n = int(rng.integers(1, 7)), int(rng.integers(1, 40))
    s = rng.integers(-2, 3, size=(q, n)).astype(np.float32)
    if seed % 2:
        s[s == 0] = np.where(rng.random(int((s == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    for k in range(1, n + 3):
        got = sg.merge_groups(*sg.topk_lists(s, k), [0, q], k)
        m, order, which = sg.rowwise_max_topk(s, k)
        c = len(order)
        assert got[1][0, :c].tolist() == order.tolist() and (got[1][0, c:] == -1).all(), (seed, k)
        assert (got[0][0, :c] == m).all() and np.isneginf(got[0][0, c:]).all()
        assert got[2][0, :c].tolist() == which.tolist() and (got[2][0, c:] == -1).all()
        assert c == min(k, n)


# ------------------------------------------------------------------------------------------------ what the cases hold
def test_the_layouts_hold_every_group_size_and_both_sides_of_the_kernel_boundary():
    totals = {name: int(np.sum(s)) for name, s in sg.LAYOUTS.items()}
    assert totals["below16"] < 16 == totals["at16"] < totals["above16"] < totals["mixed"]
    sizes = {int(x) for s in sg.LAYOUTS.values() for x in s}
    assert {0, 1, 2, 5, 16} <= sizes
    mixed = sg.LAYOUTS["mixed"]
    assert mixed[0] == 0 and mixed[-1] == 0 and 0 in mixed[1:-1] and 1 in mixed
    assert max(sizes) * max(sg.KS) == sg.MAX_ENTRIES                          # 16 queries at k = 256: exactly the limit
    assert sg.N_EXACT % 256 and 2000 <= sg.N_EXACT <= 20000


def test_exact_rows_score_exactly_in_fp32_and_in_both_storage_types():
    from filter_sets_cases import round_bf16
    for dim in sg.DIMS:
        c, q, _ = sg.exact_case(dim, "mixed")
        s = q.astype(np.float64) @ c.astype(np.float64).T
        assert (s == np.round(s)).all() and np.abs(s).max() < 2 ** 20
        assert (round_bf16(c.astype(np.float32)) == c.astype(np.float32)).all()
    c, q, sizes = sg.duplicates_case()
    assert (c[100:200] == q[0]).all() and (q[:4] == q[0]).all() and (q[4] == q[6]).all() and (q[4] != q[5]).any() and sizes == [4, 3]
    s = q.astype(np.float64) @ c.astype(np.float64).T
    m, order, which = sg.rowwise_max_topk(s[:4], 10)
    assert order.tolist() == list(range(100, 110)) and (m == 96).all() and (which == 0).all()
    m, order, which = sg.rowwise_max_topk(s[4:], 10)
    assert order.tolist() == list(range(50, 55)) + list(range(300, 305)) and which.tolist() == [1] * 5 + [0] * 5


def test_the_signed_zero_case_underflows_with_both_signs():
    c, q, sizes = sg.signed_zero_case()
    p = c[:10, 0] * q[:, :1]                                                  # fp32 products
    assert (p == 0).all() and np.signbit(p[0]).all() and not np.signbit(p[1]).any()
    from filter_sets_cases import round_bf16
    assert (round_bf16(c) == c).all() and (round_bf16(q) == q).all()


def test_the_position_probe_stands_among_other_group_sizes():
    c, pq, fq, fsizes = sg.position_case()
    assert len(fsizes) == sg.B_POS - 1 == 129 and len(pq) == 3 and set(fsizes) == set(range(7))
    for at in (0, sg.B_POS // 2, sg.B_POS - 1):
        q, sizes = sg.place(pq, fq, fsizes, at)
        ptr = sg.ptr_of(sizes)
        assert len(sizes) == sg.B_POS and sizes[at] == 3 and (q[ptr[at]:ptr[at + 1]] == pq).all() and len(q) == len(fq) + 3
        assert [s for g, s in enumerate(sizes) if g != at] == list(fsizes)


def test_the_oracle_is_brute_force_over_the_row_wise_max():
    c, q = sg.gaussian_rows(500, 64, 1), sg.gaussian_rows(6, 64, 2)
    rv, ri = sg.oracle_groups(q, c, [3, 0, 1, 2], 10, id_base=50)
    s = q.astype(np.float64) @ c.astype(np.float64).T
    for g, (a, b) in enumerate(((0, 3), (3, 3), (3, 4), (4, 6))):
        if a == b:
            assert np.isneginf(rv[g]).all() and (ri[g] == -1).all()
            continue
        m = s[a:b].max(axis=0)
        order = np.lexsort((np.arange(500), -m))[:10]
        assert ri[g].tolist() == (order + 50).tolist() and rv[g].tolist() == m[order].tolist()


def test_the_expanders_of_the_backend_tests():
    got = sg.expander(query="alpha beta gamma", trace_id="t")
    assert got == ["gamma beta alpha", "beta gamma alpha", "king of the river city"]
    assert len(sg.long_expander(query="alpha", trace_id="t")) * 200 + 200 > sg.MAX_ENTRIES
    with pytest.raises(RuntimeError):
        sg.failing_expander(query="alpha", trace_id="t")


# ------------------------------------------------------------------------------------------------ the public interface
class _NoRouter:
    def embed(self, **kw):
        raise AssertionError("not called")


def test_the_new_arguments_are_off_by_default_and_the_methods_exist():
    sig = inspect.signature(DenseRetrievalBackend.__init__)
    assert sig.parameters["query_expander"].default is None and sig.parameters["dense_expanded"].default is False
    b = DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl")
    assert b.query_expander is None and b.dense_expanded is False
    b = DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", query_expander=sg.expander, dense_expanded=True)
    assert b.query_expander is sg.expander and b.dense_expanded is True
    assert DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl",
                                 query_expander="search_groups_cases:expander").query_expander is sg.expander
    with pytest.raises(TypeError):
        DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", query_expander=3)
    with pytest.raises(ValueError):
        DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", dense_mode="rerank", dense_expanded=True)
    assert list(inspect.signature(DenseIndex.search_groups).parameters) == [
        "self", "queries", "k", "group_ptr", "sizes", "allow", "normalize", "stream", "out", "return_which"]
    assert callable(DenseIndex.last_groups)


def test_run_without_an_expander_is_unchanged_and_with_one_feeds_the_text_channel():
    """no corpus file: the dense channel degrades, the text channel is an injected searcher that records its queries"""
    from mrag_amd.dto import RetrievalIn
    seen = []

    def text_search(*, queries, top_k):
        seen.append(list(queries))
        return [{"id": f"d{len(q)}", "score": float(len(q)), "meta": {"text": q}} for q in queries]
    req = RetrievalIn(query="alpha beta gamma", graph_id="", top_k=3, trace_id="t")
    plain = DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", text_search=text_search).run(req)
    assert seen == [["alpha beta gamma"]] and plain["diagnostics"]["queries"] == ["alpha beta gamma"]
    assert "expand_error" not in plain["diagnostics"]
    off = DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", text_search=text_search, query_expander=None,
                                dense_expanded=False).run(req)
    assert off == plain
    want = ["alpha beta gamma"] + sg.expander(query="alpha beta gamma", trace_id="t")
    for run in (lambda b: b.run(req), lambda b: b.run_batch([req])[0]):
        del seen[:]
        got = run(DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", text_search=text_search, query_expander=sg.expander))
        assert seen == [want] and got["diagnostics"]["queries"] == want and "expand_error" not in got["diagnostics"]
        assert len(got["hits"]) >= len(plain["hits"])
        del seen[:]
        got = run(DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", text_search=text_search,
                                        query_expander=sg.failing_expander))
        assert seen == [["alpha beta gamma"]] and got["diagnostics"]["queries"] == ["alpha beta gamma"]
        assert "the expander is down" in got["diagnostics"]["expand_error"]
        assert got["hits"] == plain["hits"]
