"""GPU tests of the collapsed dense search (``DenseIndex.search_collapsed``, ``mrag_index_search_collapsed``): bit for bit
against the host restatement ``search_collapsed_cases.collapse_rounds`` over the same build's ``search`` /
``search(allow=)`` (scores, ids and keys) and against the fp64 brute force ``oracle_collapsed`` on exactly summing rows;
the case in which every probe must be redone; Gaussian rows against the fp64 oracle with the yardstick of
tests/test_gpu_search_groups.py (atol 1e-5, ``gap_aware_id_match`` with 0 bad); the layout properties; a query's bits
wherever it stands in the call; device buffers; the other searches left alone; the refusals; and
``DenseRetrievalBackend(dense_collapse=...)``.  What the cases hold is established on the CPU in
tests/test_search_collapsed_host.py."""
import numpy as np
import pytest

import search_collapsed_cases as sc
from oracle import dense_search as ds

pytestmark = pytest.mark.gpu
UNTOUCHED = 7777


def _index(c, keys=None, id_base=0, **kw):
    from mrag_amd.index import DenseIndex
    ix = DenseIndex(c.shape[1], **kw)
    if id_base:
        ix.set_id_base(id_base)
    if len(c):
        ix.add(c, normalize=False)
    if keys is not None:
        ix.set_row_keys(keys)
    return ix


def _same(got, want, what=None):
    for a, b, name in zip(got, want, ("scores", "ids", "keys")):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (what, name, np.argwhere(a != b)[:5].tolist())


def _check_oracle(sc_, ids, rv, ri, tol=sc.TOL):
    """the yardstick of tests/test_gpu_search_groups.py::_check_oracle"""
    assert sc_.shape == rv.shape and sc_.dtype == np.float32 and ids.dtype == np.int64
    valid = ri >= 0
    assert ((ids >= 0) == valid).all()
    assert np.isneginf(sc_[~valid]).all() and (ids[~valid] == -1).all()
    np.testing.assert_allclose(sc_[valid], rv[valid], rtol=0, atol=tol)
    with np.errstate(invalid="ignore"):
        assert (np.diff(sc_, axis=1)[valid[:, 1:]] <= 0).all()
    strict, bad = ds.gap_aware_id_match(ids, sc_, ri, rv, tol=tol)
    assert bad == 0, (strict, bad)


def _oracle32(q, c, keys, k, id_base=0):
    """oracle_collapsed with its scores as the fp32 the index returns (exactly summing rows: the same numbers)"""
    rv, ri, rk = sc.oracle_collapsed(q, c, keys, k, id_base=id_base)
    return rv.astype(np.float32), ri, rk


def _vs_restatement(ix, q, keys, k, scan_k, id_base=0, what=None):
    """search_collapsed against collapse_rounds over the same build's search / search(allow=), bit for bit, and
    last_collapsed against the restatement's rounds -> (the three outputs, rounds per query)"""
    got = ix.search_collapsed(q, k, scan_k=scan_k, normalize=False)
    lc = ix.last_collapsed()
    depth = lc["scan_k"] if scan_k is None else scan_k
    want = sc.collapse_rounds(sc.index_search_fn(ix, q, depth), len(q), keys, k, depth, id_base=id_base)
    _same(got, want[:3], what)
    rounds = want[3]
    assert lc["scan_k"] == depth and lc["redone_queries"] == int((rounds > 1).sum()) and lc["redo_rounds"] == int((rounds - 1).sum()), (what, lc)
    two = ix.search_collapsed(q, k, scan_k=scan_k, normalize=False, return_keys=False)
    assert len(two) == 2
    _same(two, want[:2], what)
    return got, rounds


# ------------------------------------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("layout", sorted(sc.LAYOUTS))
@pytest.mark.parametrize("dim,dtype", [(d, t) for d in sc.DIMS for t in ("f16", "bf16")])
def test_exact_rows_equal_the_restatement_and_the_brute_force_bit_for_bit(dim, dtype, layout):
    keys = sc.LAYOUTS[layout](sc.N_EXACT)
    k_max = max(k for k, _ in sc.K_SCAN)
    redone = 0
    for nq in sc.NQS:
        c, q = sc.exact_case(dim, nq)
        ix = _index(c, keys, dtype=dtype)
        oracle = _oracle32(q, c, keys, k_max)                                 # exact answers are prefixes of one another
        for k, scan_k in sc.K_SCAN:
            got, rounds = _vs_restatement(ix, q, keys, k, scan_k, what=(dim, dtype, layout, nq, k, scan_k))
            _same(got, [np.ascontiguousarray(x[:, :k]) for x in oracle], ("oracle", dim, dtype, layout, nq, k, scan_k))
            redone += int((rounds > 1).sum())
        ix.close()
    # which layouts meet a redo at these depths is a property of the cases: none when every row is its own key
    assert (redone == 0) == (layout == "distinct"), (layout, redone)


# ------------------------------------------------------------------------------------------------ 2. the redo case
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_every_probe_of_the_redo_case_is_redone_and_no_filler(dtype):
    c, keys, probes, fill = sc.redo_case()
    ix = _index(c, keys, dtype=dtype)
    q = np.concatenate([fill[:5], probes[:1], fill[5:9], probes[1:], fill[9:]])
    at = [5, 10, 11]
    for k, scan_k in sc.REDO_K_SCAN:
        got, rounds = _vs_restatement(ix, q, keys, k, scan_k, what=(k, scan_k))
        _same(got, _oracle32(q, c, keys, k), (k, scan_k))
        lc = ix.last_collapsed()
        assert lc["redone_queries"] == len(at) and (rounds[at] >= 2).all() and lc["redo_rounds"] >= len(at)
        assert (np.delete(rounds, at) == 1).all()                             # the fillers standing in the same call are not redone
        assert (got[2][at, 0] == sc.REDO_KEY).all() and (got[1][at, 0] == 600).all() and (got[0][at, 0] == 64).all()
        assert lc["max_rows_per_key"] == 300 and lc["distinct_keys"] == len(np.unique(keys))
        assert ix.last_filter()["allowed"] < sc.N_EXACT - 300 + 1             # the last redo round's filtered search is what it reports
    ix.close()


# ------------------------------------------------------------------------------------------------ 3. the fp64 oracle
@pytest.mark.parametrize("dim", sc.DIMS)
def test_gaussian_rows_against_the_fp64_oracle(dim):
    c, keys, q = sc.gaussian_case(dim)
    base = 1000
    ix = _index(c, keys, id_base=base)
    s, ids, kk = ix.search_collapsed(q, sc.GAUSS_K, normalize=False)           # the default depth
    lc = ix.last_collapsed()
    assert lc["scan_k"] == 28 and lc["redone_queries"] == 0 and lc["redo_rounds"] == 0
    assert lc["max_rows_per_key"] == 3 and lc["distinct_keys"] == 668
    rv, ri, rk = sc.oracle_collapsed(q, c, keys, sc.GAUSS_K, id_base=base)
    _check_oracle(s, ids, rv, ri)
    assert (kk == keys[ids - base]).all()
    assert all(len(set(row)) == sc.GAUSS_K for row in kk.tolist())
    _vs_restatement(ix, q, keys, sc.GAUSS_K, None, id_base=base)
    ix.close()


# ------------------------------------------------------------------------------------------------ 4. layout properties
def test_distinct_keys_are_the_plain_search_and_one_key_is_one_hit():
    c, q = sc.exact_case(96, 17)
    g_c, g_q = sc.gaussian_rows(sc.N_EXACT, 96, 1901), sc.gaussian_rows(17, 96, 1902)
    for rows, qs in ((c, q), (g_c, g_q)):
        ix = _index(rows, sc.LAYOUTS["distinct"](sc.N_EXACT))
        for k in (1, 10, 64, 65, 200, 256):
            got = ix.search_collapsed(qs, k, normalize=False)
            plain = ix.search(qs, k, normalize=False)
            _same(got[:2], plain, k)
            assert (got[2] == got[1]).all() and ix.last_collapsed()["scan_k"] == k and ix.last_collapsed()["redone_queries"] == 0
        ix.set_row_keys(sc.LAYOUTS["one_key"](sc.N_EXACT))
        for k, scan_k in ((1, None), (10, None), (10, 64), (256, 256)):
            got = ix.search_collapsed(qs, k, scan_k=scan_k, normalize=False)
            best = ix.search(qs, 1, normalize=False)
            _same((got[0][:, :1], got[1][:, :1]), best, k)
            assert (got[2][:, 0] == 5).all()
            assert np.isneginf(got[0][:, 1:]).all() and (got[1][:, 1:] == -1).all() and (got[2][:, 1:] == -1).all()
            lc = ix.last_collapsed()
            assert lc["max_rows_per_key"] == sc.N_EXACT and lc["distinct_keys"] == 1 and lc["redone_queries"] == (17 if k > 1 else 0)
        ix.close()


def test_fewer_keys_than_k_fewer_rows_than_scan_k_and_an_empty_index():
    dim = 64
    c, q = sc.exact_case(dim, 9)
    keys = sc.interleaved(5)(sc.N_EXACT)
    ix = _index(c, keys)
    for k, scan_k in ((10, None), (10, 64), (200, 256)):                      # 5 keys: 5 hits, then tails
        got, _ = _vs_restatement(ix, q, keys, k, scan_k)
        assert (np.sort(got[2][:, :5], axis=1) == np.arange(5)).all()
        assert np.isneginf(got[0][:, 5:]).all() and (got[1][:, 5:] == -1).all() and (got[2][:, 5:] == -1).all()
    ix.close()
    small = _index(c[:40], sc.runs(3)(40))                                    # fewer rows than scan_k: every row is seen in round 0
    for k, scan_k in ((10, None), (10, 64), (20, 256), (256, 256)):
        got, rounds = _vs_restatement(small, q, sc.runs(3)(40), k, scan_k)
        _same(got, _oracle32(q, c[:40], sc.runs(3)(40), k))
        assert ((got[1] >= 0).sum(axis=1) == min(k, 14)).all()
        if scan_k is not None and scan_k > 40:
            assert (rounds == 1).all()
    small.close()
    empty = _index(np.zeros((0, dim), dtype=np.float16))                       # no rows at all: no keys needed, all tails
    for keys0 in (None, np.zeros(0, dtype=np.int32)):
        if keys0 is not None:
            empty.set_row_keys(keys0)
        got = empty.search_collapsed(q, 10, normalize=False)
        assert np.isneginf(got[0]).all() and (got[1] == -1).all() and (got[2] == -1).all()
        assert empty.last_collapsed()["redone_queries"] == 0
    empty.close()


def test_id_base_moves_the_ids_and_nothing_else():
    c, q = sc.exact_case(96, 17, seed=1)
    keys = sc.runs(7)(sc.N_EXACT)
    base = 123_456_789_012
    ix0, ix1 = _index(c, keys), _index(c, keys, id_base=base)
    for k, scan_k in ((10, 12), (10, None), (200, 256)):
        a, _ = _vs_restatement(ix0, q, keys, k, scan_k)
        b, _ = _vs_restatement(ix1, q, keys, k, scan_k, id_base=base)
        assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()
        assert (b[1] == np.where(a[1] >= 0, a[1] + base, -1)).all() and b[1][b[1] >= 0].min() >= base
    ix0.close(); ix1.close()


# ------------------------------------------------------------------------------------------------ 5. position
def test_a_query_does_not_depend_on_its_place_or_its_neighbours():
    c, keys, probes, _ = sc.redo_case()
    fill = sc.redo_case(n_fill=129)[3]
    g_c, g_keys, g_q = sc.gaussian_case(96, nq=130)
    for rows, kk, probe, others in ((c, keys, probes[:1], fill), (g_c, g_keys, g_q[:1], g_q[1:])):
        ix = _index(rows, kk)
        for k, scan_k in ((10, 64), (10, 12), (200, 256)):
            first = None
            for at in (0, 65, 129):
                qs = sc.place(probe, others, at)
                assert len(qs) == 130
                got = ix.search_collapsed(qs, k, scan_k=scan_k, normalize=False)
                if first is None:
                    first = [x[0].copy() for x in got]
                _same([x[at] for x in got], first, (k, scan_k, at))
            if rows is c:
                assert first[2][0] == sc.REDO_KEY and ix.last_collapsed()["redone_queries"] >= 1     # the probe was redone in every place
        ix.close()


# ------------------------------------------------------------------------------------------------ 6. device buffers
def test_cuda_queries_out_and_keys_give_the_bits_of_host_buffers():
    import torch
    c, keys, probes, fill = sc.redo_case()
    q = np.concatenate([fill, probes])
    g_c, g_keys, g_q = sc.gaussian_case(96, nq=16)
    for rows, kk, qs in ((c, keys, q), (g_c, g_keys, g_q)):
        ix = _index(rows, kk)
        dev_ix = _index(rows)
        dev_ix.set_row_keys(torch.from_numpy(kk).cuda())                      # keys from a device tensor
        for k, scan_k in ((10, 64), (200, 256), (10, None)):
            host = ix.search_collapsed(qs, k, scan_k=scan_k, normalize=False)
            lc = ix.last_collapsed()
            _same(dev_ix.search_collapsed(qs, k, scan_k=scan_k, normalize=False), host)
            assert dev_ix.last_collapsed() == lc
            dq = torch.from_numpy(qs).cuda()
            dev = ix.search_collapsed(dq, k, scan_k=scan_k, normalize=False)
            assert all(t.is_cuda for t in dev) and ix.last_collapsed() == lc
            torch.cuda.synchronize()
            _same([t.cpu().numpy() for t in dev], host, k)
            out = (torch.full((len(qs), k), 5.0, device="cuda"), torch.full((len(qs), k), 5, dtype=torch.int64, device="cuda"),
                   torch.full((len(qs), k), 5, dtype=torch.int32, device="cuda"))
            back = ix.search_collapsed(dq, k, scan_k=scan_k, normalize=False, out=out)
            assert all(a is b for a, b in zip(back, out))
            torch.cuda.synchronize()
            _same([t.cpu().numpy() for t in out], host, k)
            two = ix.search_collapsed(dq, k, scan_k=scan_k, normalize=False, return_keys=False)   # no key buffer at all
            torch.cuda.synchronize()
            _same([t.cpu().numpy() for t in two], host[:2], k)
        ix.close(); dev_ix.close()


# ------------------------------------------------------------------------------------------------ 7. the other searches
def test_the_other_searches_are_left_alone():
    c, keys, probes, fill = sc.redo_case()
    q = np.concatenate([probes, fill])
    n = sc.N_EXACT
    g_c, g_q = sc.gaussian_rows(n, 64, 1911), sc.gaussian_rows(len(q), 64, 1912)
    allow = np.arange(n) % 3 != 1
    sets = [np.arange(0, n, 7), np.arange(5, 900)]
    set_of = (np.arange(len(q)) % 2).astype(np.int32)
    for rows, qs in ((c, q), (g_c, g_q)):
        ix = _index(rows)

        def others(nq, k):
            return (ix.search(qs[:nq], k, normalize=False), ix.search(qs[:nq], k, normalize=False, allow=allow),
                    ix.search_groups(qs, k, sizes=[3, len(qs) - 3], normalize=False, return_which=True),
                    ix.search_sets(qs, k, sets, set_of=set_of, normalize=False))
        for nq, k in ((1, 10), (len(q), 10), (3, 200)):
            before = others(nq, k)
            ix.set_row_keys(keys)
            with_keys = others(nq, k)
            ix.search_collapsed(qs, 10, scan_k=64, normalize=False)
            if rows is c:
                assert ix.last_collapsed()["redone_queries"] == 3
            after = others(nq, k)
            ix.set_row_keys(None)
            for a, b, d in zip(before, with_keys, after):
                _same(a, b, (nq, k))
                _same(a, d, (nq, k))
        ix.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def _raw(ix, q, k, scan_k=0, nq=None, dtype=None, h=None, null=()):
    """the C call itself on output buffers pre-filled with UNTOUCHED -> (status, message, scores, ids, keys)"""
    from mrag_amd import _native as N
    lib = N.load()
    q = np.ascontiguousarray(q, dtype=np.float32)
    s = np.full((max(len(q), 1), max(k, 1)), float(UNTOUCHED), dtype=np.float32)
    ids, kk = np.full(s.shape, UNTOUCHED, dtype=np.int64), np.full(s.shape, UNTOUCHED, dtype=np.int32)
    bufs = {"q": q.ctypes.data, "sc": s.ctypes.data, "ids": ids.ctypes.data, "keys": kk.ctypes.data}
    for name in null:
        bufs[name] = None
    st = lib.mrag_index_search_collapsed(ix._h if h is None else h, bufs["q"], len(q) if nq is None else nq,
                                         N.MRAG_F32 if dtype is None else dtype, 0, 0, k, scan_k, bufs["sc"], bufs["ids"], bufs["keys"],
                                         0, None)
    return st, (lib.mrag_last_error() or b"").decode(), s, ids, kk


def _untouched(s, ids, kk):
    return (s == UNTOUCHED).all() and (ids == UNTOUCHED).all() and (kk == UNTOUCHED).all()


def test_refusals_leave_the_outputs_untouched_and_name_the_cause():
    from mrag_amd import _native as N
    from mrag_amd._native import MragError
    lib = N.load()
    n, dim = 500, 64
    c, q = sc.small_int_rows(n, dim, 1931), sc.small_int_rows(5, dim, 1932)
    keys = sc.runs(3)(n)
    ix = _index(c)
    INVALID, UNSUPPORTED = -1, -5
    with pytest.raises(MragError):                                             # nothing completed yet
        ix.last_collapsed()
    st, msg, *out = _raw(ix, q, 4)                                             # no keys set
    assert st == INVALID and "no row keys" in msg and _untouched(*out)
    # set_row_keys: a wrong length, a negative key (the keys set before stay), NULL with rows
    for bad, word in ((keys[:-1], "rows"), (np.concatenate([keys[:-1], [-1]]).astype(np.int32), "negative")):
        assert lib.mrag_index_set_row_keys(ix._h, bad.ctypes.data, len(bad), 0) == INVALID and word.encode() in lib.mrag_last_error()
    assert lib.mrag_index_set_row_keys(ix._h, None, n, 0) == INVALID and b"NULL" in lib.mrag_last_error()
    assert lib.mrag_index_set_row_keys(ix._h, keys.ctypes.data, -1, 0) == INVALID
    for bad in (keys[:-1], np.full(n, -1), np.zeros((n, 1), dtype=np.int32), np.zeros(n), np.full(n, 2 ** 31)):
        with pytest.raises((ValueError, MragError)):
            ix.set_row_keys(bad)
    assert _raw(ix, q, 4)[0] == INVALID                                        # still no keys
    ix.set_row_keys(keys)
    st, _, s, ids, kk = _raw(ix, q, 4)
    assert st == 0
    _same((s, ids, kk), _oracle32(q, c, keys, 4))
    assert lib.mrag_index_set_row_keys(ix._h, np.full(n, -7, dtype=np.int32).ctypes.data, n, 0) == INVALID
    st, _, s2, ids2, kk2 = _raw(ix, q, 4)                                      # ... the refused keys changed nothing
    assert st == 0
    _same((s2, ids2, kk2), (s, ids, kk))
    st, _, s2, ids2, kk2 = _raw(ix, q, 4, null=("keys",))                      # out_keys may be NULL
    assert st == 0 and (kk2 == UNTOUCHED).all()
    _same((s2, ids2), (s, ids))
    cases = [
        (dict(nq=-1), INVALID, "nq"),
        (dict(k=0), INVALID, "k"), (dict(k=-3), INVALID, "k"),
        (dict(k=257), UNSUPPORTED, "257"),
        (dict(k=10, scan_k=9), INVALID, "scan_k"), (dict(k=10, scan_k=257), INVALID, "scan_k"), (dict(k=10, scan_k=-1), INVALID, "scan_k"),
        (dict(null=("q",)), INVALID, "NULL"), (dict(null=("sc",)), INVALID, "NULL"), (dict(null=("ids",)), INVALID, "NULL"),
        (dict(dtype=99), INVALID, "dtype"),
        (dict(h=0xdead), INVALID, "handle"),
    ]
    for kw, want, word in cases:
        args = dict(k=4)
        args.update(kw)
        st, msg, *out = _raw(ix, q, args.pop("k"), **args)
        assert st == want and word in msg, (kw, st, msg)
        assert _untouched(*out), kw
    st, _, *out = _raw(ix, q[:0], 4)                                           # no queries: nothing to do, nothing written
    assert st == 0 and _untouched(*out)
    # rows added after set_row_keys: refused until the keys are set again for all rows
    ix.add(c[:10], normalize=False)
    st, msg, *out = _raw(ix, q, 4)
    assert st == INVALID and "500" in msg and "510" in msg and _untouched(*out)
    with pytest.raises(MragError):
        ix.search_collapsed(q, 4, normalize=False)
    keys2 = np.concatenate([keys, keys[:10]])
    ix.set_row_keys(keys2)
    _vs_restatement(ix, q.astype(np.float16), keys2, 4, None)
    assert ix.last_collapsed()["max_rows_per_key"] == 6
    # the Python method refuses before the library is called
    for kw in (dict(k=0), dict(k=257), dict(k=10, scan_k=9), dict(k=10, scan_k=257), dict(k=10, scan_k=0), dict(k=4, out=(s, ids))):
        with pytest.raises(ValueError):
            ix.search_collapsed(q, normalize=False, **kw)
    ix.close()


# ------------------------------------------------------------------------------------------------ 9. the backend
class _Router:
    def embed(self, *, model_hint, texts, require=None):
        return {"vectors": [sc.pm1_vec(t) for t in texts]}


@pytest.fixture()
def docs(tmp_path):
    import filter_sets_cases as fs
    from mrag_amd import corpus
    path = tmp_path / "docs.jsonl"
    corpus.write_docs_jsonl(path, fs.doc_rows())
    corpus.drop_shared("dense-index|"); corpus.drop_shared("bm25-index|")
    yield str(path)
    corpus.drop_shared("dense-index|"); corpus.drop_shared("bm25-index|")


def _requests():
    import filter_sets_cases as fs
    from mrag_amd.dto import RetrievalIn
    return [RetrievalIn(query=t, graph_id="", top_k=(1, 15, 300)[g % 3], trace_id=f"t{g}") for g, t in enumerate(fs.doc_queries())]


@pytest.mark.parametrize("collapse", ["title", sc.title_of, "search_collapsed_cases:title_of"], ids=["field", "callable", "string"])
@pytest.mark.parametrize("variant", ["dense-only", "bm25"])
def test_run_batch_gives_every_request_the_hits_of_run_with_one_dense_hit_per_title(docs, variant, collapse):
    from mrag_amd.backend import DenseRetrievalBackend, resolve_embed_model
    kw = dict(index_path=docs, dense_pool_k=100)
    if variant == "bm25":
        kw["text_channel"] = "bm25"
    reqs = _requests()
    b = DenseRetrievalBackend(_Router(), dense_collapse=collapse, **kw)
    plain = DenseRetrievalBackend(_Router(), **kw)
    before = [plain.run(r) for r in reqs[:6]]
    got = b.run_batch(reqs)
    state = b._get_state(resolve_embed_model(b.router), "t")
    ix, rows = state["index"], state["rows"]
    for g, r in enumerate(reqs):
        want = b.run(r)
        assert want["diagnostics"]["dense_error"] is None and want["hits"], (g, r.query)
        assert got[g]["hits"] == want["hits"], (variant, g, r.query)
        diag, wdiag = dict(got[g]["diagnostics"]), dict(want["diagnostics"])
        dc, wdc = diag.pop("dense_collapse"), wdiag.pop("dense_collapse")
        assert diag.pop("batch_size") == len(reqs) and diag == wdiag, (variant, g)
        pool = max(r.top_k, 100)
        k_eff = min(pool, 200)                                                 # 200 titles of 4 sentences each
        for d in (dc, wdc):
            assert d["keys"] == 200 and d["max_rows_per_key"] == 4 and k_eff <= d["scan_k"] <= 256 and d["redone"] >= 0
        assert diag["pool"]["dense_pool_k_effective"] == k_eff
        assert diag["dense_scored"] == k_eff                                   # one dense hit per title reached
        # the dense channel itself: the representatives of the k_eff best titles, no title twice
        s, ids, kk = ix.search_collapsed(np.asarray([sc.pm1_vec(r.query)], dtype=np.float32), k_eff)
        titles = [rows[i]["title"] for i in ids[0].tolist()]
        assert len(set(titles)) == k_eff == len(titles)
        if variant == "dense-only":
            docs_hit = [h["meta"]["doc"] for h in want["hits"]]
            assert len(set(docs_hit)) == len(docs_hit) == min(r.top_k, k_eff) and set(docs_hit) <= set(titles)
    # the same backend without dense_collapse returns what it returned before, also on the index that now holds keys
    for r, was in zip(reqs[:6], before):
        assert plain.run(r) == was
        assert "dense_collapse" not in was["diagnostics"]
    assert [o["hits"] for o in plain.run_batch(reqs[:6])] == [o["hits"] for o in before]


def test_the_refused_constructor_combinations_raise(docs):
    from mrag_amd.backend import DenseRetrievalBackend
    for bad in (dict(dense_mode="rerank", text_channel="bm25"), dict(dense_row_filter=lambda req, rows: None),
                dict(query_expander=lambda **k: [], dense_expanded=True)):
        with pytest.raises(ValueError):
            DenseRetrievalBackend(_Router(), index_path=docs, dense_collapse="title", **bad)
    with pytest.raises(TypeError):
        DenseRetrievalBackend(_Router(), index_path=docs, dense_collapse=4)
