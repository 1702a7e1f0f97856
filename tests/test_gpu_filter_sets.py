"""GPU tests of the dense search over per-question allow-sets (``DenseIndex.search_sets``, ``mrag_index_search_sets``):
the top-k of every question over its own set's rows against the fp64 oracle over ``c16[set]`` with the yardstick of
tests/test_gpu_filtered.py (atol 1e-5, ``gap_aware_id_match`` with 0 bad, (-inf, -1) tails, descending order); ties;
bit-for-bit independence of a question's place in the batch; bit-for-bit agreement with the single filtered search on
exactly summing rows; the two routes; the refusals; and ``DenseRetrievalBackend(dense_filter_batch=True)``.  What the cases
hold is established on the CPU in tests/test_filter_sets_host.py.  The 1 GiB scratch cut is not reached here: the library
has no setter for that limit, and no test allocates a gigabyte of segments."""
import functools

import numpy as np
import pytest

import filter_sets_cases as fs
from oracle import dense_search as ds

pytestmark = pytest.mark.gpu
UNTOUCHED = 7777


def _index(c, id_base=0, **kw):
    from mrag_amd.index import DenseIndex
    ix = DenseIndex(c.shape[1], **kw)
    if id_base:
        ix.set_id_base(id_base)
    ix.add(c, normalize=False)
    return ix


def _check_result(sc, ids, rv, ri, tol=fs.TOL):
    assert sc.shape == rv.shape and sc.dtype == np.float32 and ids.dtype == np.int64
    valid = ri >= 0
    assert ((ids >= 0) == valid).all()
    assert np.isneginf(sc[~valid]).all() and (ids[~valid] == -1).all()
    np.testing.assert_allclose(sc[valid], rv[valid], rtol=0, atol=tol)
    with np.errstate(invalid="ignore"):                              # (-inf) - (-inf) in the tails, which `valid` leaves out
        assert (np.diff(sc, axis=1)[valid[:, 1:]] <= 0).all()        # descending
    strict, bad = ds.gap_aware_id_match(ids, sc, ri, rv, tol=tol)
    assert bad == 0, (strict, bad)


@functools.lru_cache(maxsize=None)
def _grid(dim):
    sets, set_of = fs.grid_layout()
    return fs.gaussian_rows(fs.N_GRID, dim, 1000 + dim), fs.gaussian_rows(len(set_of), dim, 2000 + dim), sets, set_of


# ------------------------------------------------------------------------------------------------ parity grid
@pytest.mark.parametrize("dim", fs.DIMS)
def test_parity_grid_against_the_fp64_oracle(dim):
    c, q, sets, set_of = _grid(dim)
    ix = _index(c)
    for k in fs.KS:
        sc, ids = ix.search_sets(q, k, sets, set_of=set_of, normalize=False)
        _check_result(sc, ids, *fs.oracle(q, c, sets, set_of, k))
        ls = ix.last_sets()
        assert ls["scanned"] == len(set_of) and ls["routed"] == 0
        per = np.bincount(set_of, minlength=len(sets))
        assert ls["descriptors"] == sum(-(-len(s) // 128) * -(-int(n) // 128) for s, n in zip(sets, per))
    # masks give what positions give, and set_of defaults to one set per question
    few = np.flatnonzero(np.bincount(set_of, minlength=len(sets)) == 1)[:6]
    qs = np.asarray([np.flatnonzero(set_of == s)[0] for s in few])
    masks = [np.isin(np.arange(fs.N_GRID), sets[s]) for s in few]
    a = ix.search_sets(q[qs], 10, masks, normalize=False)
    b = ix.search_sets(q[qs], 10, [sets[s] for s in few], set_of=np.arange(len(few)), normalize=False)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    _check_result(*a, *fs.oracle(q[qs], c, [sets[s] for s in few], np.arange(len(few)), 10))
    ix.close()


def test_bf16_storage_id_base_and_unnormalised_queries():
    from mrag_amd.index import DenseIndex
    dim, base = 96, 123_456
    sets, set_of = fs.grid_layout()
    x = ds.l2_normalize(ds.make_gaussian(fs.N_GRID, dim, 61))
    raw = ds.make_gaussian(len(set_of), dim, 62) * np.float32(3.5)            # un-normalised questions
    for dtype in ("f16", "bf16"):
        ix = DenseIndex(dim, dtype=dtype)
        ix.set_id_base(base)
        ix.add(x, normalize=False)
        stored = ix.rows()                                                   # the stored values, widened
        prep = DenseIndex(dim, dtype=dtype)                                  # the row preparation (K1) of the questions, read back:
        prep.add(raw, normalize=True)                                        # add and search prepare rows with the same kernel
        prepared = prep.rows()
        prep.close()
        want = fs.round_bf16(ds.l2_normalize(raw)) if dtype == "bf16" else ds.normalize_round(raw).astype(np.float32)
        assert (prepared != want).mean() < 1e-4                              # the oracle's rounding, but for a vanishing fraction
        for k in (10, 200):
            sc, ids = ix.search_sets(raw, k, sets, set_of=set_of, normalize=True)
            _check_result(sc, ids, *fs.oracle(prepared, stored, sets, set_of, k, id_base=base))
            assert ids[ids >= 0].min() >= base
        ix.close()


# ------------------------------------------------------------------------------------------------ ties
def test_identical_rows_come_out_in_row_order():
    c, q, sets, set_of = fs.identical_rows_case()
    ix = _index(c)
    for k in (1, 10, 256):
        sc, ids = ix.search_sets(q, k, sets, set_of=set_of, normalize=False)
        assert (ids == sets[0][:k]).all()                                       # ids ascending: the first k of the set
        assert (sc == sc[:, :1]).all()
        _check_result(sc, ids, *fs.oracle(q, c, sets, set_of, k))
    ix.close()


def test_integer_rows_with_ties_cut_by_k():
    c, q, sets, set_of = fs.integer_rows_case()
    ix = _index(c)
    for k in (10, 200, 256):
        sc, ids = ix.search_sets(q, k, sets, set_of=set_of, normalize=False)
        rv, ri = fs.oracle(q, c, sets, set_of, k)
        assert (ids == ri).all() and (sc == rv).all()                             # exact scores, the tie resolved by row
    ix.close()


# ------------------------------------------------------------------------------------------------ position
def test_a_question_does_not_depend_on_its_place_or_its_neighbours():
    c, pq, pset, fq, fsets, fof = fs.position_case()
    ix = _index(c)
    for k in (10, 256):
        alone = ix.search_sets(pq, k, [pset], normalize=False)
        _check_result(*alone, *fs.oracle(pq, c, [pset], [0], k))
        for at in (0, fs.B_POS // 2, fs.B_POS - 1):
            q, sets, set_of = fs.place(pq, pset, fq, fsets, fof, at)
            sc, ids = ix.search_sets(q, k, sets, set_of=set_of, normalize=False)
            assert sc[at].tobytes() == alone[0][0].tobytes() and ids[at].tobytes() == alone[1][0].tobytes(), (k, at)
            if at == 0:
                _check_result(sc, ids, *fs.oracle(q, c, sets, set_of, k))
    ix.close()


# ------------------------------------------------------------------------------------------------ the single filtered search
@pytest.mark.parametrize("rows,dim", [("pm1", 96), ("int", 64)])
def test_exact_rows_equal_the_single_filtered_search_bit_for_bit(rows, dim):
    n = 3000
    c = fs.pm1_rows(n, dim, 71) if rows == "pm1" else fs.small_int_rows(n, dim, 72)
    q = fs.pm1_rows(12, dim, 73) if rows == "pm1" else fs.small_int_rows(12, dim, 74)
    sets = [fs.pick(n, m, 80 + i) for i, m in enumerate((1, 9, 129, 300, 2000))]
    set_of = np.asarray([0, 1, 2, 3, 4, 4, 3, 2, 1, 0, 4, 3], dtype=np.int32)
    ix = _index(c)
    for k in (10, 200):
        sc, ids = ix.search_sets(q, k, sets, set_of=set_of, normalize=False)
        rv, ri = fs.oracle(q, c, sets, set_of, k)
        assert (ids == ri).all() and (sc == rv).all()
        for path in ("mask", "compact"):
            for g in range(len(q)):
                one = ix.search(q[g:g + 1], k, normalize=False, allow=sets[set_of[g]], filter_path=path)
                assert one[0][0].tobytes() == sc[g].tobytes() and one[1][0].tobytes() == ids[g].tobytes(), (k, path, g)
    ix.close()


def test_gaussian_rows_against_the_single_filtered_search():
    """cross-kernel bits are reported, not asserted (the project's precedent): both sides meet the oracle yardstick"""
    n, dim, k = 3000, 96, 10
    c, q = fs.gaussian_rows(n, dim, 75), fs.gaussian_rows(8, dim, 76)
    sets = [fs.pick(n, m, 90 + i) for i, m in enumerate((9, 129, 300, 2000))]
    set_of = np.asarray([0, 1, 2, 3, 3, 2, 1, 0], dtype=np.int32)
    ix = _index(c)
    sc, ids = ix.search_sets(q, k, sets, set_of=set_of, normalize=False)
    rv, ri = fs.oracle(q, c, sets, set_of, k)
    _check_result(sc, ids, rv, ri)
    for path in ("mask", "compact"):
        same = 0
        for g in range(len(q)):
            one = ix.search(q[g:g + 1], k, normalize=False, allow=sets[set_of[g]], filter_path=path)
            _check_result(one[0], one[1], rv[g:g + 1], ri[g:g + 1])
            same += one[0][0].tobytes() == sc[g].tobytes()
        print(f"search_sets vs single filtered search ({path}): {same} of {len(q)} questions agree in every score bit")
    ix.close()


# ------------------------------------------------------------------------------------------------ routing
def test_sets_above_the_select_capacity_are_routed_to_one_filtered_search():
    n, dim, k = 20000, 64, 10
    c = fs.gaussian_rows(n, dim, 81)
    sets = [fs.pick(n, fs.SEL_CAP, 82), fs.pick(n, fs.SEL_CAP + 1, 83), fs.pick(n, 40, 84), fs.pick(n, 300, 85), np.zeros(0, dtype=np.int64)]
    set_of = np.asarray([2, 0, 1, 3] + [1] * 39 + [0, 0, 4, 2], dtype=np.int32)
    q = fs.gaussian_rows(len(set_of), dim, 86)
    ix = _index(c)
    sc, ids = ix.search_sets(q, k, sets, set_of=set_of, normalize=False)
    ls = ix.last_sets()
    assert ls["routed"] == 40 and ls["scanned"] == len(set_of) - 40
    assert ls["descriptors"] == fs.SEL_CAP // 128 + 1 + 3
    assert ix.last_filter()["allowed"] == fs.SEL_CAP + 1                          # ONE routed search: the last filtered search is it
    _check_result(sc, ids, *fs.oracle(q, c, sets, set_of, k))
    # only routed sets, and k above 64 for a routed set
    sc, ids = ix.search_sets(q[:3], 200, [sets[1]], set_of=np.zeros(3, dtype=np.int32), normalize=False)
    assert ix.last_sets() == {"scanned": 0, "routed": 3, "descriptors": 0}
    _check_result(sc, ids, *fs.oracle(q[:3], c, [sets[1]], np.zeros(3, dtype=np.int32), 200))
    ix.close()


# ------------------------------------------------------------------------------------------------ refusals
def _raw(ix, q, k, set_ptr, set_rows, set_of, nq=None, n_sets=None, dtype=None, h=None, null=()):
    """the C call itself on output buffers pre-filled with UNTOUCHED -> (status, message, scores, ids)"""
    from mrag_amd import _native as N
    lib = N.load()
    q = np.ascontiguousarray(q, dtype=np.float32)
    set_ptr, set_rows = np.ascontiguousarray(set_ptr, dtype=np.int64), np.ascontiguousarray(set_rows, dtype=np.int64)
    set_of = np.ascontiguousarray(set_of, dtype=np.int32)
    rows = max(len(q), 1)
    sc, ids = np.full((rows, max(k, 1)), float(UNTOUCHED), dtype=np.float32), np.full((rows, max(k, 1)), UNTOUCHED, dtype=np.int64)
    bufs = {"q": q.ctypes.data, "ptr": set_ptr.ctypes.data, "rows": set_rows.ctypes.data, "of": set_of.ctypes.data,
            "sc": sc.ctypes.data, "ids": ids.ctypes.data}
    for name in null:
        bufs[name] = None
    st = lib.mrag_index_search_sets(ix._h if h is None else h, bufs["q"], len(q) if nq is None else nq, N.MRAG_F32 if dtype is None else dtype, 0, k,
                                    len(set_ptr) - 1 if n_sets is None else n_sets, bufs["ptr"], bufs["rows"], bufs["of"], bufs["sc"],
                                    bufs["ids"], None)
    return st, (lib.mrag_last_error() or b"").decode(), sc, ids


def test_refusals_leave_the_outputs_untouched_and_name_the_set_or_question():
    n, dim = 500, 64
    c = fs.gaussian_rows(n, dim, 91)
    q = fs.gaussian_rows(3, dim, 92)
    ix = _index(c)
    ptr, rows, of = [0, 2, 5], [3, 7, 1, 2, 499], [1, 0, 1]
    st, _, sc, ids = _raw(ix, q, 4, ptr, rows, of)
    assert st == 0 and ids[0].tolist()[3] == -1 and set(ids[1].tolist()) == {3, 7, -1}
    INVALID, UNSUPPORTED = -1, -5
    cases = [
        (dict(nq=-1), INVALID, "nq"),
        (dict(n_sets=-1), INVALID, "n_sets"),
        (dict(set_ptr=[1, 2, 5]), INVALID, "set 0"),
        (dict(set_ptr=[0, 3, 2], set_rows=[1, 2, 3]), INVALID, "set 1"),
        (dict(set_rows=[3, 7, 1, 2, 500]), INVALID, "set 1"),
        (dict(set_rows=[-1, 7, 1, 2, 499]), INVALID, "set 0"),
        (dict(set_rows=[7, 3, 1, 2, 499]), INVALID, "set 0"),
        (dict(set_rows=[3, 7, 1, 1, 499]), INVALID, "set 1"),                  # a duplicate
        (dict(set_of=[1, 0, 2]), INVALID, "question 2"),
        (dict(set_of=[-1, 0, 1]), INVALID, "question 0"),
        (dict(null=("q",)), INVALID, "NULL"), (dict(null=("ptr",)), INVALID, "NULL"), (dict(null=("rows",)), INVALID, "NULL"),
        (dict(null=("of",)), INVALID, "NULL"), (dict(null=("sc",)), INVALID, "NULL"), (dict(null=("ids",)), INVALID, "NULL"),
        (dict(dtype=99), INVALID, "dtype"),
        (dict(h=0xdead), INVALID, "handle"),
        (dict(k=0), INVALID, "k"), (dict(k=-3), INVALID, "k"),
        (dict(k=257), UNSUPPORTED, "257"),
    ]
    for kw, want, word in cases:
        args = dict(k=4, set_ptr=ptr, set_rows=rows, set_of=of)
        args.update(kw)
        st, msg, sc, ids = _raw(ix, q, args.pop("k"), args.pop("set_ptr"), args.pop("set_rows"), args.pop("set_of"), **args)
        assert st == want and word in msg, (kw, st, msg)
        assert (sc == UNTOUCHED).all() and (ids == UNTOUCHED).all(), kw
    # no questions: nothing to do, nothing written
    st, _, sc, ids = _raw(ix, q[:0], 4, ptr, rows, [])
    assert st == 0 and (sc == UNTOUCHED).all() and (ids == UNTOUCHED).all()
    # the Python method refuses before the library is called
    for bad in (dict(sets=[[3, 500]]), dict(sets=[[1], [2]]), dict(sets=[[1]], set_of=[0, 1, 0]), dict(sets=[[1]], set_of=[0, 0, 1])):
        with pytest.raises(ValueError):
            ix.search_sets(q, 4, bad["sets"], set_of=bad.get("set_of"), normalize=False)
    with pytest.raises(ValueError):
        ix.search_sets(q, 257, [[1]], set_of=[0, 0, 0])
    ix.close()


# ------------------------------------------------------------------------------------------------ the other searches
def test_the_plain_and_the_filtered_search_are_left_alone():
    n, dim = 6000, 96
    c, q = fs.gaussian_rows(n, dim, 95), fs.gaussian_rows(40, dim, 96)
    sets = [fs.pick(n, 300, 97), fs.pick(n, 40, 98)]
    set_of = (np.arange(40) % 2).astype(np.int32)
    allow = fs.pick(n, 700, 99)
    ix = _index(c)
    for nq, k in ((1, 10), (40, 10), (3, 200)):
        plain = ix.search(q[:nq], k, normalize=False)
        filt = ix.search(q[:nq], k, normalize=False, allow=allow)
        got = ix.search_sets(q, k, sets, set_of=set_of, normalize=False)
        again, fagain = ix.search(q[:nq], k, normalize=False), ix.search(q[:nq], k, normalize=False, allow=allow)
        for a, b in ((plain, again), (filt, fagain)):
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (nq, k)
        _check_result(*got, *fs.oracle(q, c, sets, set_of, k))
    ix.close()


# ------------------------------------------------------------------------------------------------ the backend
class _Router:
    def embed(self, *, model_hint, texts, require=None):
        return {"vectors": [fs.pm1_vec(t) for t in texts]}


@pytest.fixture()
def docs(tmp_path):
    from mrag_amd import corpus
    path = tmp_path / "docs.jsonl"
    corpus.write_docs_jsonl(path, fs.doc_rows())
    corpus.drop_shared("dense-index|"); corpus.drop_shared("bm25-index|")
    yield str(path)
    corpus.drop_shared("dense-index|"); corpus.drop_shared("bm25-index|")


def test_run_batch_with_the_switch_gives_every_request_the_hits_of_run(docs):
    from mrag_amd.backend import DenseRetrievalBackend
    from mrag_amd.dto import RetrievalIn
    reqs = [RetrievalIn(query=t, graph_id="", top_k=(1, 15, 300)[g % 3], trace_id=f"t{g}") for g, t in enumerate(fs.doc_queries())]
    kw = dict(index_path=docs, text_channel="bm25", dense_pool_k=100, dense_row_filter=fs.three_sets_or_none)
    on = DenseRetrievalBackend(_Router(), dense_filter_batch=True, **kw)
    off = DenseRetrievalBackend(_Router(), **kw)
    got, loop = on.run_batch(reqs), off.run_batch(reqs)
    allowed = set()
    for g, r in enumerate(reqs):
        want = off.run(r)
        assert want["diagnostics"]["dense_error"] is None and got[g]["diagnostics"]["dense_error"] is None
        assert got[g]["hits"] == want["hits"] and want["hits"], (g, r.query)
        # the switch off: the loop's diagnostics, which are run's
        diag = dict(loop[g]["diagnostics"])
        assert diag.pop("batch_size") == len(reqs) and diag == want["diagnostics"] and loop[g]["hits"] == want["hits"]
        # the switch on: the same diagnostics but for the filter's path
        diag = dict(got[g]["diagnostics"])
        assert diag.pop("batch_size") == len(reqs)
        if fs.three_sets_or_none(r, fs.doc_rows()) is None:
            assert "dense_filter" not in diag and diag == want["diagnostics"]
        else:
            df = diag.pop("dense_filter")
            assert df["path"] == "sets" and df["allowed"] == want["diagnostics"]["dense_filter"]["allowed"]
            allowed.add(df["allowed"])
            assert diag == {k: v for k, v in want["diagnostics"].items() if k != "dense_filter"}
    assert allowed == {200, 300, 400}
    # the requests with a set went through ONE search_sets call in which equal sets are shared: 4 + 3 + 2 row chunks, each
    # with one group of questions
    from mrag_amd.backend import resolve_embed_model
    n_sets = sum(fs.three_sets_or_none(r, fs.doc_rows()) is not None for r in reqs)
    ix = on._get_state(resolve_embed_model(on.router), "t")["index"]
    assert ix.last_sets() == {"scanned": n_sets, "routed": 0, "descriptors": 9}
