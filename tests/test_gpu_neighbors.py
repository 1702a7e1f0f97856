"""GPU tests of the neighbour expansion (``DenseIndex.expand_neighbors``, ``mrag_index_expand_neighbors``) and of the
backend's device graph channel (``DenseRetrievalBackend(graph_channel="neighbors")``).  Every comparison of the call is
bit for bit against the host restatement ``neighbors_cases.expand`` -- scores, ids, dist and seed -- which
tests/test_neighbors_host.py holds against the reference's own expansion; what the cases hold is established there too.

Entry counts: 2048, 2049 and 4096 entries cannot be had inside the call's limits (``neighbors_cases.ENTRY_SHAPES``), so
2047 / 2050 stand on the two sides of the padded size 2048, 4095 is the largest count served and 4097 the smallest refused."""
from typing import Optional

import numpy as np
import pytest

import neighbors_cases as nc

pytestmark = pytest.mark.gpu
UNTOUCHED = 7777
NAMES = ("scores", "ids", "dist", "seed")


def _index(n=nc.N_ROWS, keys=None, id_base=0, seed=7):
    from mrag_amd.index import DenseIndex
    ix = DenseIndex(nc.DIM)
    if id_base:
        ix.set_id_base(id_base)
    if n:
        ix.add(nc.pm1_rows(n, nc.DIM, seed), normalize=False)
    if keys is not None:
        ix.set_row_keys(keys)
    return ix


def _same(got, want, what=None):
    assert len(got) == len(want)
    for a, b, name in zip(got, want, NAMES):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (what, name, np.argwhere(a != b)[:5].tolist())


def _check(ix, seeds, keys, window, m=None, decay=None, id_base=0, what=None):
    got = ix.expand_neighbors(seeds, window, m=m, decay=decay, return_from=True)
    want = nc.expand(seeds, keys, window, m=m, decay=decay, id_base=id_base)
    _same(got, want, what)
    two = ix.expand_neighbors(seeds, window, m=m, decay=decay)                  # dist / seed omitted
    assert len(two) == 2
    _same(two, want[:2], what)
    return got


@pytest.fixture(scope="module")
def shared_index():
    ix = _index()
    yield ix
    ix.close()


def _padded(row, s):
    out = np.full((1, s), -1, dtype=np.int64)
    out[0, :len(row)] = row
    return out


# ------------------------------------------------------------------------------------------------ 1. layouts x windows
@pytest.mark.parametrize("layout", sorted(nc.LAYOUTS))
def test_every_layout_and_window_equals_the_restatement_bit_for_bit(shared_index, layout):
    ix, n = shared_index, nc.N_ROWS
    keys = nc.LAYOUTS[layout](n)
    ix.set_row_keys(keys)
    seeds = np.concatenate([_padded(nc.edge_seeds(keys), 9), nc.random_seeds(n, 40, 9, 11)])
    for window in nc.WINDOWS:
        got = _check(ix, seeds, keys, window, what=(layout, window))
        assert ix.last_neighbors() == {"questions": len(seeds), "max_entries": 9 * (2 * window + 1), "window": window}
        found = (got[1] >= 0).sum(axis=1)
        if layout == "own_runs":                                                # no neighbours at all: the valid distinct seeds
            assert (got[2][got[1] >= 0] == 0).all()
        if layout == "one_run" and window:
            assert found.max() > 9                                              # neighbours were reached
        if layout == "recurring":
            assert found.max() <= 9 * 3                                         # a key that recurs does not link its runs


def test_a_non_zero_id_base_and_seeds_outside_the_index(shared_index):
    n, base = 700, 123_456_789_012
    keys = nc.runs_1_to_7(n)
    ix = _index(n, keys, id_base=base)
    seeds = np.concatenate([_padded(nc.edge_seeds(keys, base), 12), nc.random_seeds(n, 30, 12, 21, id_base=base)])
    assert (seeds == -1).any() and ((seeds < base) & (seeds != -1)).any() and (seeds >= base + n).any()
    for window in (0, 2, 16):
        got = _check(ix, seeds, keys, window, id_base=base, what=window)
        assert got[1][got[1] >= 0].min() >= base and got[1].max() < base + n
    # the same rows through local ids on an index without a base: everything but the ids is equal
    ix0 = _index(n, keys)
    local = np.where((seeds >= base) & (seeds < base + n), seeds - base, -1)
    a, b = ix0.expand_neighbors(local, 2, return_from=True), ix.expand_neighbors(seeds, 2, return_from=True)
    assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
    assert (b[1] == np.where(a[1] >= 0, a[1] + base, -1)).all()
    only_invalid = np.asarray([[-1, -1, -1], [base - 1, base + n, -1], [5, n + 3, -7]], dtype=np.int64)   # local ids: outside too
    got = _check(ix, only_invalid, keys, 2, id_base=base)
    assert (got[1] == -1).all() and np.isneginf(got[0]).all() and (got[2] == -1).all() and (got[3] == -1).all()
    ix.close(); ix0.close()


# ------------------------------------------------------------------------------------------------ 2. shapes
def test_seed_strides_0_1_and_256(shared_index):
    ix, n = shared_index, nc.N_ROWS
    keys = nc.runs_1_to_7(n)
    ix.set_row_keys(keys)
    none = np.zeros((3, 0), dtype=np.int64)
    for window in (0, 2):
        got = ix.expand_neighbors(none, window, m=5, return_from=True)
        _same(got, nc.expand(none, keys, window, m=5))
        assert (got[1] == -1).all() and got[1].shape == (3, 5)
        assert ix.expand_neighbors(none, window)[1].shape == (3, 1)              # the default m is never below 1
    for window in nc.WINDOWS:
        _check(ix, nc.random_seeds(n, 7, 1, 31, invalid=False), keys, window, what=("stride 1", window))
    for window in (0, 2, 7):                                                    # 256, 1280 and 3840 entries
        _check(ix, nc.random_seeds(n, 3, 256, 32 + window), keys, window, what=("stride 256", window))
    ix.set_row_keys(nc.one_run(n))
    _check(ix, nc.random_seeds(n, 2, 256, 33), nc.one_run(n), 7, what="stride 256, one run")


@pytest.mark.parametrize("entries", sorted(nc.ENTRY_SHAPES))
def test_entry_counts_around_a_wave_the_padded_size_and_the_limit(shared_index, entries):
    ix, n = shared_index, nc.N_ROWS
    s, window = nc.ENTRY_SHAPES[entries]
    for layout in ("one_run", "runs_1_to_7"):
        keys = nc.LAYOUTS[layout](n)
        ix.set_row_keys(keys)
        spread = np.random.default_rng(entries).permutation(n)[:3 * s].reshape(3, s).astype(np.int64)   # few overlaps: many rows
        for seeds in (nc.random_seeds(n, 3, s, entries), spread):
            got = _check(ix, seeds, keys, window, what=(entries, layout))
            assert ix.last_neighbors()["max_entries"] == entries
        if layout == "one_run":
            assert (got[1] >= 0).sum(axis=1).max() > min(entries, n) // 3       # spread seeds: many distinct rows


def test_m_below_at_and_above_the_distinct_rows(shared_index):
    ix, n = shared_index, nc.N_ROWS
    keys = nc.runs_1_to_7(n)
    ix.set_row_keys(keys)
    seeds = nc.random_seeds(n, 6, 9, 41)
    full = nc.expand(seeds, keys, 2)
    found = (full[1] >= 0).sum(axis=1)
    assert found.min() >= 2
    for m in sorted({1, int(found.min()) - 1, int(found.min()), int(found.max()), int(found.max()) + 1, 45, 46, 300, 4096}):
        got = _check(ix, seeds, keys, 2, m=m, what=m)
        c = min(m, 45)
        assert got[1].shape == (6, m) and (got[1][:, :c] == full[1][:, :c]).all() and (got[1][:, 45:] == -1).all()


def test_a_custom_decay_with_ties_and_the_default(shared_index):
    from mrag_amd.index import reference_decay
    ix, n = shared_index, nc.N_ROWS
    keys = nc.one_run(n)
    ix.set_row_keys(keys)
    seeds = nc.random_seeds(n, 5, 6, 51)
    decay = np.asarray([3.5, 3.5, 1.0, 1.0, 1.0, -2.0], dtype=np.float32)        # ties: the order stays (dist, seed, row)
    got = _check(ix, seeds, keys, 5, decay=decay)
    v = got[1] >= 0
    assert (got[0][v] == decay[got[2][v]]).all() and set(got[0][v].tolist()) == {3.5, 1.0, -2.0}
    got = _check(ix, seeds, keys, 16)
    v = got[1] >= 0
    assert (got[0][v] == reference_decay(16).astype(np.float32)[got[2][v]]).all() and got[2].max() == 16


# ------------------------------------------------------------------------------------------------ 3. position, buffers
def test_a_question_does_not_depend_on_its_place_among_130(shared_index):
    ix, n = shared_index, nc.N_ROWS
    keys = nc.runs_1_to_7(n)
    ix.set_row_keys(keys)
    fill = nc.random_seeds(n, 129, 9, 61)
    probe = nc.random_seeds(n, 1, 9, 62)
    for window in (2, 16):
        first = None
        for at in (0, 1, 63, 64, 65, 129):
            seeds = np.concatenate([fill[:at], probe, fill[at:]])
            assert len(seeds) == 130
            got = ix.expand_neighbors(seeds, window, return_from=True)
            if first is None:
                first = [x[at].copy() for x in got]
                _same([x[None] for x in first], nc.expand(probe, keys, window))
            _same([x[at] for x in got], first, (window, at))


def test_device_seeds_and_outputs_on_a_side_stream(shared_index):
    import torch
    ix, n = shared_index, nc.N_ROWS
    keys = nc.runs_1_to_7(n)
    ix.set_row_keys(keys)
    seeds = nc.random_seeds(n, 33, 20, 71)
    side = torch.cuda.Stream()
    for window, m in ((2, None), (5, 17), (0, 300)):
        want = nc.expand(seeds, keys, window, m=m)
        mm = want[0].shape[1]
        with torch.cuda.stream(side):
            ds = torch.from_numpy(seeds).cuda()
            side.synchronize()
        dev = ix.expand_neighbors(ds, window, m=m, return_from=True, stream=side)
        assert all(t.is_cuda for t in dev)
        side.synchronize()
        _same([t.cpu().numpy() for t in dev], want, (window, m))
        out = (torch.full((33, mm), 5.0, device="cuda"), torch.full((33, mm), 5, dtype=torch.int64, device="cuda"),
               torch.full((33, mm), 5, dtype=torch.int32, device="cuda"), torch.full((33, mm), 5, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        back = ix.expand_neighbors(ds, window, m=m, return_from=True, stream=side, out=out)
        assert all(a is b for a, b in zip(back, out))
        side.synchronize()
        _same([t.cpu().numpy() for t in out], want, (window, m))
        two = ix.expand_neighbors(ds, window, m=m, stream=side)                   # no dist / seed buffers at all
        side.synchronize()
        assert len(two) == 2
        _same([t.cpu().numpy() for t in two], want[:2], (window, m))
        assert ix.last_neighbors() == {"questions": 33, "max_entries": 20 * (2 * window + 1), "window": window}


def test_seeds_taken_straight_from_search_of_the_same_index(shared_index):
    import torch
    ix, n = shared_index, nc.N_ROWS
    keys = nc.runs_1_to_7(n)
    ix.set_row_keys(keys)
    q = nc.pm1_rows(19, nc.DIM, 81)
    _, ids = ix.search(q, 10, normalize=False)
    _check(ix, ids, keys, 2)
    dq = torch.from_numpy(q).cuda()
    _, dids = ix.search(dq, 10, normalize=False)                                # stays on the device: nothing is read back
    dev = ix.expand_neighbors(dids[:, :7], 2, return_from=True)                  # a non-contiguous view of the leading columns
    torch.cuda.synchronize()
    _same([t.cpu().numpy() for t in dev], nc.expand(ids[:, :7], keys, 2))
    _, big = ix.search(q[:2], 256, normalize=False)                             # the widest list as seeds
    _check(ix, big, keys, 7)


# ------------------------------------------------------------------------------------------------ 4. refusals
def _raw(ix, seeds, window, m, decay=None, nq=None, stride=None, h=None, null=()):
    """the C call itself on output buffers pre-filled with UNTOUCHED -> (status, message, scores, ids, dist, seed)"""
    from mrag_amd import _native as N
    lib = N.load()
    seeds = np.ascontiguousarray(seeds, dtype=np.int64)
    dk = np.ascontiguousarray(nc.reference_decay(max(window, 0)) if decay is None else decay, dtype=np.float32)
    shape = (max(len(seeds), 1), min(max(m, 1), 5000))
    s = np.full(shape, float(UNTOUCHED), dtype=np.float32)
    ids = np.full(shape, UNTOUCHED, dtype=np.int64)
    dist, seed = np.full(shape, UNTOUCHED, dtype=np.int32), np.full(shape, UNTOUCHED, dtype=np.int32)
    bufs = {"seeds": seeds.ctypes.data, "decay": dk.ctypes.data, "sc": s.ctypes.data, "ids": ids.ctypes.data, "dist": dist.ctypes.data,
            "seed": seed.ctypes.data}
    for name in null:
        bufs[name] = None
    st = lib.mrag_index_expand_neighbors(ix._h if h is None else h, bufs["seeds"], seeds.shape[0] if nq is None else nq,
                                         seeds.shape[1] if stride is None else stride, 0, window, bufs["decay"], m, bufs["sc"],
                                         bufs["ids"], bufs["dist"], bufs["seed"], 0, None)
    return st, (lib.mrag_last_error() or b"").decode(), s, ids, dist, seed


def _untouched(*out):
    return all((x == UNTOUCHED).all() for x in out)


def test_refusals_leave_the_outputs_untouched_and_name_the_cause():
    from mrag_amd._native import MragError
    n = 500
    keys = nc.runs_1_to_7(n)
    ix = _index(n)
    seeds = nc.random_seeds(n, 4, 6, 91)
    INVALID, UNSUPPORTED = -1, -5
    with pytest.raises(MragError):                                             # nothing completed yet
        ix.last_neighbors()
    st, msg, *out = _raw(ix, seeds, 2, 10)                                     # no keys set
    assert st == INVALID and "no row keys" in msg and _untouched(*out)
    ix.set_row_keys(keys)
    st, _, s, ids, dist, seed = _raw(ix, seeds, 2, 10)
    assert st == 0
    _same((s, ids, dist, seed), nc.expand(seeds, keys, 2, m=10))
    st, _, s2, ids2, dist2, seed2 = _raw(ix, seeds, 2, 10, null=("dist", "seed"))    # either may be NULL
    assert st == 0 and _untouched(dist2, seed2)
    _same((s2, ids2), (s, ids))
    st, _, s2, ids2, dist2, seed2 = _raw(ix, seeds, 2, 10, null=("seed",))
    assert st == 0 and _untouched(seed2)
    _same((s2, ids2, dist2), (s, ids, dist))
    wide = np.zeros((2, nc.ENTRIES_REFUSED[0]), dtype=np.int64)
    cases = [
        (dict(nq=-1), INVALID, "nq"), (dict(stride=-1), INVALID, "seed_stride"),
        (dict(m=0), INVALID, "m"), (dict(m=-4), INVALID, "m"), (dict(window=-1), INVALID, "window"),
        (dict(null=("seeds",)), INVALID, "NULL"), (dict(null=("decay",)), INVALID, "NULL"), (dict(null=("sc",)), INVALID, "NULL"),
        (dict(null=("ids",)), INVALID, "NULL"),
        (dict(decay=[1.0, np.nan, 0.5]), INVALID, "finite"), (dict(decay=[np.inf, 1.0, 0.5]), INVALID, "finite"),
        (dict(decay=[1.0, 0.5, -np.inf]), INVALID, "finite"), (dict(decay=[1.0, 0.5, 0.6]), INVALID, "increases"),
        (dict(h=0xdead), INVALID, "handle"),
        (dict(window=17, decay=np.ones(18)), UNSUPPORTED, "17"),
        (dict(seeds=np.zeros((2, 257), dtype=np.int64), window=0), UNSUPPORTED, "257"),
        (dict(seeds=wide, window=nc.ENTRIES_REFUSED[1]), UNSUPPORTED, "4097"),
        (dict(m=4097), UNSUPPORTED, "4097"),
    ]
    for kw, want, word in cases:
        args = dict(seeds=seeds, window=2, m=10)
        args.update(kw)
        st, msg, *out = _raw(ix, args.pop("seeds"), args.pop("window"), args.pop("m"), **args)
        assert st == want and word in msg, (kw, st, msg)
        assert _untouched(*out), kw
    assert ix.last_neighbors() == {"questions": 4, "max_entries": 30, "window": 2}   # the refused calls left the record alone
    st, _, *out = _raw(ix, seeds[:0], 2, 10)                                   # no questions: nothing to do, nothing written
    assert st == 0 and _untouched(*out)
    st, _, s, ids, dist, seed = _raw(ix, np.zeros((3, 0), dtype=np.int64), 2, 4, null=("seeds",))   # no seeds: padding only
    assert st == 0 and np.isneginf(s[:3, :4]).all() and (ids[:3, :4] == -1).all() and (dist[:3, :4] == -1).all() and (seed[:3, :4] == -1).all()
    # rows added after set_row_keys: refused until the keys are set again for all rows
    ix.add(nc.pm1_rows(10, nc.DIM, 92), normalize=False)
    st, msg, *out = _raw(ix, seeds, 2, 10)
    assert st == INVALID and "500" in msg and "510" in msg and _untouched(*out)
    with pytest.raises(MragError):
        ix.expand_neighbors(seeds, 2)
    keys2 = nc.runs_1_to_7(510)
    ix.set_row_keys(keys2)
    _check(ix, seeds, keys2, 2)
    # the Python method refuses before the library is called
    for kw in (dict(window=17), dict(window=-1), dict(window=1.5), dict(window=2, m=0), dict(window=2, m=4097),
               dict(window=2, decay=[1.0, 0.5]), dict(window=2, decay=[1.0, 0.5, 0.6]), dict(window=2, decay=[1.0, np.nan, 0.5]),
               dict(window=2, out=(s, ids, dist)), dict(window=2, return_from=True, out=(s, ids))):
        with pytest.raises(ValueError):
            ix.expand_neighbors(seeds, **kw)
    for bad in (np.zeros(5, dtype=np.int64), np.zeros((2, 3)), np.zeros((2, 257), dtype=np.int64)):
        with pytest.raises(ValueError):
            ix.expand_neighbors(bad, 0)
    with pytest.raises(ValueError):
        ix.expand_neighbors(wide, nc.ENTRIES_REFUSED[1])
    ix.close()
    empty = _index(0)                                                          # no rows at all: no keys needed, padding only
    got = empty.expand_neighbors(seeds, 2, return_from=True)
    assert np.isneginf(got[0]).all() and (got[1] == -1).all() and (got[2] == -1).all() and (got[3] == -1).all()
    empty.close()


# ------------------------------------------------------------------------------------------------ 5. the other searches
def test_the_other_searches_are_left_alone():
    n = nc.N_ROWS
    keys = nc.runs_1_to_7(n)
    ix = _index(n, keys)
    q = nc.pm1_rows(9, nc.DIM, 101)
    seeds = nc.random_seeds(n, 50, 64, 102)

    def others(k):
        return (ix.search(q, k, normalize=False), ix.search_groups(q, k, sizes=[4, 5], normalize=False, return_which=True),
                ix.search_collapsed(q, min(k, 100), normalize=False), ix.search_collapsed(q, 10, scan_k=12, normalize=False))
    for k in (10, 200):
        before = others(k)
        host = ix.expand_neighbors(seeds, 5, return_from=True)
        after = others(k)
        for a, b in zip(before, after):
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes(), k
        _same(ix.expand_neighbors(seeds, 5, return_from=True), host)            # ... and they left the expansion alone
    _same(host, nc.expand(seeds, keys, 5))
    ix.close()


# ------------------------------------------------------------------------------------------------ 6. the backend
class _Router:
    def embed(self, *, model_hint, texts, require=None):
        import filter_sets_cases as fs
        return {"vectors": [fs.pm1_vec(t) for t in texts]}


@pytest.fixture()
def docs(tmp_path):
    import filter_sets_cases as fs
    from mrag_amd import corpus
    path = tmp_path / "docs.jsonl"
    corpus.write_docs_jsonl(path, fs.doc_rows())
    corpus.drop_shared("dense-index|"); corpus.drop_shared("bm25-index|")
    yield str(path)
    corpus.drop_shared("dense-index|"); corpus.drop_shared("bm25-index|")


def _requests(n=None):
    import filter_sets_cases as fs
    from mrag_amd.dto import RetrievalIn

    class Req(RetrievalIn):
        graph_window: Optional[int] = None
    windows = (None, None, 0, 5, None, 16, 1)
    return [Req(query=t, graph_id="", top_k=(1, 15, 300)[g % 3], trace_id=f"t{g}", graph_window=windows[g % 7])
            for g, t in enumerate(fs.doc_queries()[:n])]


def _expected_run(b, req, state):
    """what ``run`` must return: ``fuse_channels`` of the request's text hits, the graph hits the restatement builds from its
    dense list, and its dense scores"""
    import filter_sets_cases as fs
    from mrag_amd import fusion
    from mrag_amd.index import row_keys_of
    ix, rows = state["index"], state["rows"]
    top_k = req.top_k
    pool = max(top_k, b.dense_pool_k)
    window = req.graph_window if isinstance(req.graph_window, int) else b.graph_window
    t_hits = list(b.text_search(queries=[req.query], top_k=pool)) if b.text_search is not None else []
    sc, ids = ix.search(np.asarray([fs.pm1_vec(req.query)], dtype=np.float32), min(pool, len(rows), 256))
    dense_norm = fusion.dedupe_by_norm_id(b._dense_hits(rows, sc[0], ids[0]))
    keys = row_keys_of([r["title"] for r in rows])[0]
    seed_k = top_k if b.graph_seed_k is None else b.graph_seed_k
    g_hits = nc.graph_hits(rows, ids[0].tolist(), keys, window, seed_k, pool)
    fused = fusion.fuse_channels(t_hits, g_hits, {nid: h["score"] for nid, h in dense_norm.items()}, alpha_text=b.alpha_text,
                                 alpha_graph=b.alpha_graph, alpha_dense=b.alpha_dense, top_k=10 ** 9)
    for h in fused:
        if not h["meta"].get("text") and h["id"] in dense_norm:
            meta = dict(dense_norm[h["id"]]["meta"])
            meta.update({k: v for k, v in h["meta"].items() if k.startswith("score_")})
            h["meta"] = meta
    return fused[:top_k], g_hits


@pytest.mark.parametrize("variant", ["dense-only", "bm25", "bm25-seed5"])
def test_run_equals_fuse_channels_of_the_three_hit_lists(docs, variant):
    from mrag_amd.backend import DenseRetrievalBackend, resolve_embed_model
    kw = dict(index_path=docs, dense_pool_k=100, graph_channel="neighbors")
    if variant != "dense-only":
        kw["text_channel"] = "bm25"
    if variant == "bm25-seed5":
        kw["graph_seed_k"] = 5
    b = DenseRetrievalBackend(_Router(), **kw)
    plain = DenseRetrievalBackend(_Router(), **{k: v for k, v in kw.items() if not k.startswith("graph_")})
    state = b._get_state(resolve_embed_model(b.router), "t")
    with_graph = 0
    for r in _requests(14):
        got = b.run(r)
        if b.text_search is None and variant != "dense-only":
            pytest.fail("the BM25 channel did not come up")
        want, g_hits = _expected_run(b, r, state)
        assert got["hits"] == want, (variant, r.query)
        d = got["diagnostics"]
        window = r.graph_window if r.graph_window is not None else 2
        seeds = min(5 if variant == "bm25-seed5" else r.top_k, 256, 4096 // (2 * window + 1), max(r.top_k, 100))
        assert d["graph_candidates"] == len(g_hits) > 0 and d["graph_window_used"] == window and "graph_error" not in d
        assert d["graph_channel"] == {"seeds": seeds, "window": window, "max_entries": seeds * (2 * window + 1)}
        with_graph += sum(1 for h in got["hits"] if h["meta"]["score_graph_norm"] > 0)
        assert all("distance" in h["meta"] for h in got["hits"] if h["meta"].get("source") == "graph")
        off = plain.run(r)                                                      # without the channel: as before, no graph keys
        assert off["diagnostics"]["graph_candidates"] == 0 and "graph_channel" not in off["diagnostics"]
        assert all(h["meta"]["score_graph_norm"] == 0.0 for h in off["hits"])
    assert with_graph > 0


@pytest.mark.parametrize("variant", ["dense-only", "bm25", "bm25-collapse", "bm25-device-fuse"])
def test_run_batch_gives_every_request_the_hits_of_run(docs, variant):
    from mrag_amd.backend import DenseRetrievalBackend
    kw = dict(index_path=docs, dense_pool_k=100, graph_channel="neighbors")
    if variant != "dense-only":
        kw["text_channel"] = "bm25"
    if variant == "bm25-collapse":
        kw["dense_collapse"] = "title"
    if variant == "bm25-device-fuse":
        kw["fuse_on_device"] = True
    b = DenseRetrievalBackend(_Router(), **kw)
    reqs = _requests()
    got = b.run_batch(reqs)
    with_graph = 0
    for g, r in enumerate(reqs):
        want = b.run(r)
        assert want["diagnostics"]["dense_error"] is None and want["hits"], (g, r.query)
        assert got[g]["hits"] == want["hits"], (variant, g, r.query)             # ids, scores, meta with distance and the norms
        diag, wdiag = dict(got[g]["diagnostics"]), dict(want["diagnostics"])
        diag.pop("dense_collapse", None); wdiag.pop("dense_collapse", None)
        assert diag.pop("batch_size") == len(reqs) and diag == wdiag, (variant, g)
        assert diag["graph_candidates"] > 0 and "graph_error" not in diag
        with_graph += sum(1 for h in want["hits"] if h["meta"]["score_graph_norm"] > 0 and "distance" in h["meta"])
    assert with_graph > 0                                                       # the graph channel moved fused scores
    assert b._state["index"].last_neighbors()["window"] in {0, 1, 2, 5, 16}


def _fails_for_war(req, rows):
    if "war" in req.query:
        raise RuntimeError("no filter for this request")
    return None


def test_a_request_whose_dense_channel_fails_gets_graph_error_and_still_returns(docs):
    from mrag_amd.backend import DenseRetrievalBackend
    b = DenseRetrievalBackend(_Router(), index_path=docs, dense_pool_k=100, text_channel="bm25", graph_channel="neighbors",
                              dense_row_filter=_fails_for_war)
    reqs = _requests(12)
    bad = [g for g, r in enumerate(reqs) if "war" in r.query]
    assert bad and len(bad) < len(reqs)
    got = b.run_batch(reqs)
    for g, r in enumerate(reqs):
        one = b.run(r)
        assert got[g]["hits"] == one["hits"] and one["hits"], g
        for d in (got[g]["diagnostics"], one["diagnostics"]):
            if g in bad:
                assert d["dense_error"] and "dense channel failed" in d["graph_error"] and d["graph_candidates"] == 0
                assert "graph_channel" not in d
            else:
                assert d["dense_error"] is None and "graph_error" not in d and d["graph_candidates"] > 0
    # a window beyond the call's limit degrades the same way: the expansion refuses, the other channels stand
    good = [r for g, r in enumerate(reqs) if g not in bad]

    class Wide:
        query, graph_id, top_k, trace_id, graph_window = good[0].query, "", 15, "t", 17
    one = b.run(Wide())
    assert one["hits"] and "window" in one["diagnostics"]["graph_error"] and one["diagnostics"]["graph_candidates"] == 0
    assert b.run_batch([Wide(), reqs[1]])[0]["hits"] == one["hits"]
