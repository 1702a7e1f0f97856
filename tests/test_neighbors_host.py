"""The host side of the neighbour expansion (the device graph channel), and what its GPU tests can see -- no kernel runs
here.  The two new C entry points are declared, bound and exported and refuse a dead handle; the restatement
``neighbors_cases.expand`` equals the reference's ``expand_qmatch_neighbors`` on the F11 fixture as a mapping row ->
(score, distance); ``reference_decay`` holds its edge values; the restatement's order is strict and does not depend on
seed-row padding; the case builders hold what tests/test_gpu_neighbors.py relies on; the backend's new arguments are off
unless asked for and refuse what they must; and ``fusion.batch_entries`` without graph arrays is what it was."""
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import neighbors_cases as nc
from mrag_amd import fusion
from mrag_amd.backend import DenseRetrievalBackend
from mrag_amd.index import DenseIndex, reference_decay

ROOT = Path(__file__).resolve().parents[1]
NEW = {"mrag_index_expand_neighbors": 14, "mrag_index_last_neighbors": 4}


# ------------------------------------------------------------------------------------------------ ABI and binding
def test_abi_declares_binds_and_exports_the_neighbour_expansion():
    from mrag_amd import _native as N
    hdr = (ROOT / "include" / "mrag_neighbors.h").read_text()
    assert '#include "mrag_neighbors.h"' in (ROOT / "include" / "mrag.h").read_text()
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(mrag_\w+)\(([^;]*)\);", hdr, flags=re.M | re.S)}
    assert set(declared) == set(NEW) == set(N.NEIGHBORS_SIGNATURES)
    for name, nargs in NEW.items():
        assert len(declared[name].split(",")) == nargs and len(N.NEIGHBORS_SIGNATURES[name]) == nargs
    assert "Stream contract" in hdr and "no synchronisation" in hdr             # stated where the call is declared
    earlier = (N.SIGNATURES, N.EXTENSION_SIGNATURES, N.FUSE_BATCH_SIGNATURES, N.RERANK_BATCH_SIGNATURES, N.FILTER_BATCH_SIGNATURES,
               N.SEARCH_GROUPS_SIGNATURES, N.SEARCH_COLLAPSED_SIGNATURES)
    assert tuple(len(t) for t in earlier) == (64, 2, 1, 1, 2, 2, 3)
    assert sum(len(t) for t in earlier) + len(N.NEIGHBORS_SIGNATURES) == 77
    assert not any(set(NEW) & set(t) for t in earlier)
    assert "MRAG_ABI_VERSION 1" in (ROOT / "include" / "mrag.h").read_text()
    assert N.lib_path().exists(), "libmrag_hip.so is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.lib_path())], capture_output=True, text=True).stdout
    assert set(NEW) <= set(re.findall(r"\b(mrag_[a-z0-9_]+)$", out, flags=re.M))
    lib = N.load()
    assert all(getattr(lib, name).argtypes == N.NEIGHBORS_SIGNATURES[name] for name in NEW)


def test_a_dead_handle_fails_with_a_status_and_a_message():
    from mrag_amd import _native as N
    lib = N.load()
    seeds, decay = np.zeros((2, 3), np.int64), np.asarray([1.0, 0.5], np.float32)
    s, i = np.full((2, 4), 7.0, np.float32), np.full((2, 4), 7, np.int64)
    d, p = np.full((2, 4), 7, np.int32), np.full((2, 4), 7, np.int32)
    st = lib.mrag_index_expand_neighbors(0xdead, seeds.ctypes.data, 2, 3, 0, 1, decay.ctypes.data, 4, s.ctypes.data, i.ctypes.data,
                                         d.ctypes.data, p.ctypes.data, 0, None)
    assert st == -1 and b"invalid handle" in lib.mrag_last_error()
    assert (s == 7.0).all() and (i == 7).all() and (d == 7).all() and (p == 7).all()
    assert lib.mrag_index_last_neighbors(0xdead, None, None, None) == -1 and b"invalid handle" in lib.mrag_last_error()


# ------------------------------------------------------------------------------------------------ the reference
def test_the_restatement_equals_the_reference_on_f11_as_a_mapping():
    cases = nc.golden_cases()
    assert len(cases) >= 100 and nc.GOLDEN.stat().st_size < 64 * 1024
    assert {w for _, _, w, _ in cases} == set(range(9))
    lens_seen, docs_seen = set(), set()
    for keys, seeds, window, want in cases:
        lens_seen |= set(np.bincount(keys).tolist())
        docs_seen.add(int(keys.max()) + 1)
        assert len(set(seeds[0].tolist())) < seeds.shape[1]                     # a duplicate seed in every case
        sc, ids, dist, seed = nc.expand(seeds, keys, window)
        valid = ids[0] >= 0
        decay = reference_decay(window)
        got = {int(r): (float(decay[d]), int(d)) for r, d in zip(ids[0][valid], dist[0][valid])}
        assert got == want, (keys.tolist(), seeds.tolist(), window)             # fp64 decay values: equal, not close
        assert (sc[0][valid] == decay.astype(np.float32)[dist[0][valid]]).all()
        assert np.isneginf(sc[0][~valid]).all() and (dist[0][~valid] == -1).all() and (seed[0][~valid] == -1).all()
        for r, j in zip(ids[0][valid], seed[0][valid]):                          # the named seed attains the distance
            assert abs(int(seeds[0, j]) - int(r)) == got[int(r)][1] and keys[seeds[0, j]] == keys[r]
    assert lens_seen >= set(range(1, 8)) and docs_seen >= set(range(1, 8))


def test_reference_decay_edge_values():
    assert reference_decay(0).tolist() == [1.0] and reference_decay(0).dtype == np.float64
    d = reference_decay(16)
    assert d.shape == (17,) and d[:3].tolist() == [1.0, 0.7, 0.5]
    assert d[3] == 0.5 - 0.1 * 1 and d[4] == 0.5 - 0.1 * 2
    assert d[5] == 0.5 - 0.1 * 3 == 0.19999999999999996 and d[5] != 0.2          # as the reference computes it
    assert 0.5 - 0.1 * 4 < 0.1 and d[6] == 0.1 and (d[6:] == 0.1).all()          # the floor
    assert (np.diff(d) <= 0).all() and (np.diff(d.astype(np.float32)) <= 0).all()
    assert reference_decay(2).tolist() == d[:3].tolist()
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError):
            reference_decay(bad)


# ------------------------------------------------------------------------------------------------ the declared order
def test_the_order_is_strict_and_independent_of_padding():
    keys = nc.runs_1_to_7(400)
    for window in nc.WINDOWS:
        seeds = nc.random_seeds(400, 12, 9, 40 + window)
        sc, ids, dist, seed = nc.expand(seeds, keys, window)
        for q in range(len(seeds)):
            v = ids[q] >= 0
            order = list(zip(dist[q][v].tolist(), seed[q][v].tolist(), ids[q][v].tolist()))
            assert all(a < b for a, b in zip(order, order[1:]))                 # strictly increasing: no two rows compare equal
            assert len(set(ids[q][v].tolist())) == int(v.sum())
            assert (np.diff(sc[q][v]) <= 0).all()                               # by distance = by score, stable
            assert not v[int(v.sum()):].any()                                   # the valid slots lead
        padded = np.concatenate([seeds, np.full((len(seeds), 7), -1, dtype=np.int64)], axis=1)
        for a, b in zip(nc.expand(padded, keys, window, m=ids.shape[1]), (sc, ids, dist, seed)):
            assert a.tobytes() == b.tobytes()
        for m in (1, 5, ids.shape[1] + 3):                                       # any m is a prefix, then padding
            cut = nc.expand(seeds, keys, window, m=m)
            c = min(m, ids.shape[1])
            assert (cut[1][:, :c] == ids[:, :c]).all() and (cut[1][:, c:] == -1).all()


def test_a_case_worked_by_hand():
    #    row:  0  1  2  3  4  5  6  7  8  9
    keys = np.asarray([5, 5, 5, 5, 9, 9, 5, 5, 5, 2], dtype=np.int32)
    sc, ids, dist, seed = nc.expand(np.asarray([[3, 1, 6, -1, 3, 99]]), keys, 2, id_base=0)
    # seed 0 (row 3) reaches 1..3, seed 1 (row 1) 0..3, seed 2 (row 6, a second run of key 5) 6..8; position 4 duplicates 0
    assert ids[0, :7].tolist() == [3, 1, 6, 2, 0, 7, 8] and (ids[0, 7:] == -1).all()
    assert dist[0, :7].tolist() == [0, 0, 0, 1, 1, 1, 2] and seed[0, :7].tolist() == [0, 1, 2, 0, 1, 2, 2]
    assert sc[0, :7].tolist() == [1.0, 1.0, 1.0, np.float32(0.7), np.float32(0.7), np.float32(0.7), 0.5]
    sc, ids, dist, seed = nc.expand(np.asarray([[103]]), keys, 5, id_base=100, decay=[4, 3, 3, 2, 2, 1])
    assert ids[0].tolist()[:4] == [103, 102, 101, 100] and dist[0].tolist()[:4] == [0, 1, 2, 3] and sc[0].tolist()[:4] == [4, 3, 3, 2]


# ------------------------------------------------------------------------------------------------ what the cases hold
def test_the_case_builders_hold_what_the_gpu_tests_rely_on():
    n = nc.N_ROWS
    assert n % 256 != 0 and n <= 2000
    for name, fn in nc.LAYOUTS.items():
        keys = fn(n)
        assert keys.dtype == np.int32 and keys.shape == (n,) and keys.min() >= 0, name
    lo, hi = nc.run_bounds(nc.one_run(n))
    assert (lo == 0).all() and (hi == n - 1).all()
    lo, hi = nc.run_bounds(nc.own_runs(n))
    assert (lo == np.arange(n)).all() and (hi == lo).all()
    lo, hi = nc.run_bounds(nc.runs_1_to_7(n))
    assert set((hi - lo + 1).tolist()) == set(range(1, 8))
    rec = nc.recurring(n)
    lo, hi = nc.run_bounds(rec)
    assert len(np.unique(rec)) == 3 and (hi - lo + 1).max() == 3                # the key recurs, its runs do not link
    got = nc.reached([4], rec, 16)
    assert sorted(got) == [3, 4, 5] and rec[4] == rec[13] != rec[6]
    for name, fn in nc.LAYOUTS.items():
        keys = fn(n)
        rows = nc.edge_seeds(keys).tolist()
        lo, hi = nc.run_bounds(keys)
        assert 0 in rows and n - 1 in rows and any(r == lo[r] for r in rows) and any(r == hi[r] for r in rows), name
    short = nc.edge_seeds(nc.runs_1_to_7(n))
    lo, hi = nc.run_bounds(nc.runs_1_to_7(n))
    assert {1, 2} <= set((hi - lo + 1)[short].tolist())                          # runs shorter than the window
    seeds = nc.random_seeds(n, 40, 9, 1, id_base=1000)
    assert (seeds == -1).any() and ((seeds < 1000) & (seeds != -1)).any() and (seeds >= 1000 + n).any()
    assert all(len(set(r)) < len(r) for r in seeds.tolist())                     # duplicates
    over = [len(nc.reached(r, nc.one_run(n), 5, 1000)) < 11 * sum(1000 <= x < 1000 + n for x in r) for r in seeds.tolist()]
    assert any(over)                                                            # reaches overlap
    assert {63, 64, 65, 2047, 2050, 4095} == set(nc.ENTRY_SHAPES)
    for entries, (s, w) in nc.ENTRY_SHAPES.items():
        assert s * (2 * w + 1) == entries and s <= 256 and w <= 16
    s, w = nc.ENTRIES_REFUSED
    assert s * (2 * w + 1) == 4097 and s <= 256 and w <= 16
    # no shape inside the limits has 2048, 2049 or 4096 entries
    counts = {s * (2 * w + 1) for s in range(257) for w in range(17)}
    assert not counts & {2048, 2049, 4096} and max(c for c in counts if c <= 4096) == 4095


# ------------------------------------------------------------------------------------------------ the public interface
class _NoRouter:
    def embed(self, **kw):
        raise AssertionError("not called")


def test_the_new_arguments_are_off_by_default_and_refuse_what_they_must():
    sig = inspect.signature(DenseRetrievalBackend.__init__)
    assert sig.parameters["graph_channel"].default is None and sig.parameters["graph_window"].default == 2
    assert sig.parameters["graph_seed_k"].default is None and sig.parameters["graph_doc"].default == "title"
    kw = dict(index_path="nowhere.jsonl")
    b = DenseRetrievalBackend(_NoRouter(), **kw)
    assert b.graph_channel is None and b.graph_window == 2 and b.graph_seed_k is None and b.graph_doc == "title"
    b = DenseRetrievalBackend(_NoRouter(), graph_channel="neighbors", graph_window=3, graph_seed_k=7, graph_doc=nc.title_of, **kw)
    assert (b.graph_channel, b.graph_window, b.graph_seed_k) == ("neighbors", 3, 7) and b.graph_doc is nc.title_of
    assert DenseRetrievalBackend(_NoRouter(), graph_channel="neighbors", graph_doc="neighbors_cases:title_of", **kw).graph_doc is nc.title_of
    for bad in (dict(graph_channel="bfs"), dict(graph_channel="neighbors", graph_expand=lambda **k: []),
                dict(graph_channel="neighbors", dense_mode="rerank"),
                dict(graph_channel="neighbors", dense_collapse="doc_id"),
                dict(graph_channel="neighbors", dense_collapse=nc.title_of),       # "title" and a callable: not the same keys
                dict(graph_window=-1), dict(graph_window=1.5), dict(graph_seed_k=0)):
        with pytest.raises(ValueError):
            DenseRetrievalBackend(_NoRouter(), **kw, **bad)
    with pytest.raises(TypeError):
        DenseRetrievalBackend(_NoRouter(), graph_channel="neighbors", graph_doc=3, **kw)
    DenseRetrievalBackend(_NoRouter(), graph_channel="neighbors", dense_collapse="title", **kw)
    DenseRetrievalBackend(_NoRouter(), graph_channel="neighbors", graph_doc=nc.title_of, dense_collapse=nc.title_of, **kw)
    DenseRetrievalBackend(_NoRouter(), dense_collapse="doc_id", **kw)               # without the channel graph_doc is not looked at
    # the request's own integer window wins; the seeds are capped by the call's limits
    b = DenseRetrievalBackend(_NoRouter(), graph_channel="neighbors", **kw)

    class Req:
        graph_window = 5
    assert b._graph_window_of(Req()) == 5 and b._graph_window_of(object()) == 2
    Req.graph_window = "7"
    assert b._graph_window_of(Req()) == 2
    Req.graph_window = -3
    assert b._graph_window_of(Req()) == 0
    assert b._graph_seeds_of(20, 2) == 20 and b._graph_seeds_of(300, 2) == 256 and b._graph_seeds_of(300, 16) == 4096 // 33
    assert DenseRetrievalBackend(_NoRouter(), graph_channel="neighbors", graph_seed_k=5, **kw)._graph_seeds_of(20, 2) == 5
    assert list(inspect.signature(DenseIndex.expand_neighbors).parameters) == [
        "self", "seeds", "window", "m", "decay", "return_from", "stream", "out"]
    assert callable(DenseIndex.last_neighbors)


def test_run_without_the_graph_channel_is_unchanged_and_a_missing_corpus_degrades():
    from mrag_amd.dto import RetrievalIn

    def text_search(*, queries, top_k):
        return [{"id": f"d{len(q)}", "score": float(len(q)), "meta": {"text": q}} for q in queries]
    req = RetrievalIn(query="alpha beta gamma", graph_id="", top_k=3, trace_id="t")
    plain = DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", text_search=text_search).run(req)
    off = DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", text_search=text_search, graph_channel=None).run(req)
    assert off == plain and not any(k.startswith("graph_") and k != "graph_candidates" for k in plain["diagnostics"])
    on = DenseRetrievalBackend(_NoRouter(), index_path="nowhere.jsonl", text_search=text_search, graph_channel="neighbors")
    for got in (on.run(req), on.run_batch([req])[0]):                           # no rows: no seeds, the text hits stand
        assert got["hits"] == plain["hits"] and got["diagnostics"]["graph_candidates"] == 0
        assert got["diagnostics"]["graph_window_used"] == 2 and "graph_error" not in got["diagnostics"]
        assert got["diagnostics"]["graph_channel"] == {"seeds": 0, "window": 2, "max_entries": 0}


# ------------------------------------------------------------------------------------------------ batch_entries
def _batch_entries_before(text_docs, text_scores, text_n, dense_ids, dense_scores, norm_keys, pool=None):
    """``fusion.batch_entries`` as it was before it took graph arrays, restated with one loop per question"""
    B = len(text_docs)
    ptr, keys, scores, payload = [0], [], [], []
    for g in range(B):
        lim = 2 ** 31 - 1 if pool is None else int(pool[g])
        for j in range(min(int(text_n[g]), lim, len(text_docs[g]))):
            keys.append(norm_keys[text_docs[g][j]]); scores.append(float(text_scores[g][j])); payload.append(text_docs[g][j])
        ptr += [len(keys), len(keys)]
        for j in range(min(lim, len(dense_ids[g]))):
            if dense_ids[g][j] >= 0:
                keys.append(norm_keys[dense_ids[g][j]]); scores.append(float(dense_scores[g][j])); payload.append(dense_ids[g][j])
        ptr.append(len(keys))
    return (np.asarray(ptr, np.int32), np.asarray(keys, np.int32), np.asarray(scores, np.float64), np.asarray(payload, np.int32))


def test_batch_entries_without_graph_arrays_is_byte_identical_and_with_them_fills_the_graph_range():
    rng = np.random.default_rng(5)
    B, n = 6, 50
    norm_keys = rng.permutation(n).astype(np.int32)
    t_docs, t_sc, t_n = rng.integers(0, n, (B, 7)), rng.random((B, 7)), rng.integers(0, 8, B)
    d_ids, d_sc = rng.integers(-1, n, (B, 9)), rng.random((B, 9)).astype(np.float32)
    g_rows, g_sc, g_n = rng.integers(0, n, (B, 5)), rng.random((B, 5)), rng.integers(0, 6, B)
    for pool in (None, [3, 9, 1, 20, 4, 5]):
        want = _batch_entries_before(t_docs, t_sc, t_n, d_ids, d_sc, norm_keys, pool)
        got = fusion.batch_entries(t_docs, t_sc, t_n, d_ids, d_sc, norm_keys, pool=pool)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        assert (got[0][1::3] == got[0][2::3]).all()                              # no graph entries
        cp, keys, scores, payload = fusion.batch_entries(t_docs, t_sc, t_n, d_ids, d_sc, norm_keys, pool=pool, graph_rows=g_rows,
                                                         graph_scores=g_sc, graph_n=g_n)
        for g in range(B):
            lim = 2 ** 31 - 1 if pool is None else pool[g]
            c = min(int(g_n[g]), lim)
            a, b = cp[3 * g + 1], cp[3 * g + 2]
            assert b - a == c and payload[a:b].tolist() == g_rows[g, :c].tolist() and scores[a:b].tolist() == g_sc[g, :c].tolist()
            assert keys[a:b].tolist() == norm_keys[g_rows[g, :c]].tolist()
            t0, t1 = want[0][3 * g], want[0][3 * g + 1]                           # the text and dense ranges are the old ones
            assert keys[cp[3 * g]:a].tolist() == want[1][t0:t1].tolist()
            d0, d1 = want[0][3 * g + 2], want[0][3 * g + 3]
            assert payload[b:cp[3 * g + 3]].tolist() == want[3][d0:d1].tolist()
    with pytest.raises(ValueError):
        fusion.batch_entries(t_docs, t_sc, t_n, d_ids, d_sc, norm_keys, graph_rows=g_rows)
