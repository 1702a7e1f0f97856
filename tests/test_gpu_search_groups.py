"""GPU tests of the grouped dense search (``DenseIndex.search_groups``, ``mrag_index_search_groups``): bit for bit against
the host restatement ``search_groups_cases.merge_groups`` over the same build's ``search`` of the same queries (scores,
ids and ``which``) on exactly summing rows, so that the comparison does not depend on which search kernel served which
call; against the fp64 oracle over the row-wise max on Gaussian rows with the yardstick of tests/test_gpu_filter_sets.py
(atol 1e-5, ``gap_aware_id_match`` with 0 bad, (-inf, -1) tails, descending order); a question's bits wherever it stands
in the batch; device buffers; ``allow=``; the other searches left alone; the refusals; and
``DenseRetrievalBackend(query_expander=..., dense_expanded=...)``.  What the cases hold is established on the CPU in
tests/test_search_groups_host.py."""
import numpy as np
import pytest

import search_groups_cases as sg
from oracle import dense_search as ds

pytestmark = pytest.mark.gpu
UNTOUCHED = 7777


def _index(c, id_base=0, **kw):
    from mrag_amd.index import DenseIndex
    ix = DenseIndex(c.shape[1], **kw)
    if id_base:
        ix.set_id_base(id_base)
    if len(c):
        ix.add(c, normalize=False)
    return ix


def _same(got, want, what=None):
    for a, b, name in zip(got, want, ("scores", "ids", "which")):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (what, name, np.argwhere(a != b)[:5].tolist())


def _check_oracle(sc, ids, rv, ri, tol=sg.TOL):
    assert sc.shape == rv.shape and sc.dtype == np.float32 and ids.dtype == np.int64
    valid = ri >= 0
    assert ((ids >= 0) == valid).all()
    assert np.isneginf(sc[~valid]).all() and (ids[~valid] == -1).all()
    np.testing.assert_allclose(sc[valid], rv[valid], rtol=0, atol=tol)
    with np.errstate(invalid="ignore"):
        assert (np.diff(sc, axis=1)[valid[:, 1:]] <= 0).all()
    strict, bad = ds.gap_aware_id_match(ids, sc, ri, rv, tol=tol)
    assert bad == 0, (strict, bad)


def _groups_vs_restatement(ix, q, k, sizes, what=None, **kw):
    """search_groups against merge_groups of the same build's search of the same queries, bit for bit"""
    ptr = sg.ptr_of(sizes)
    got = ix.search_groups(q, k, sizes=sizes, normalize=False, return_which=True, **kw)
    lg = ix.last_groups()
    assert lg == {"queries": len(q), "groups": len(sizes), "max_entries": max(sizes, default=0) * k}
    per_query = ix.search(q, k, normalize=False, **kw) if len(q) else (np.zeros((0, k), np.float32), np.zeros((0, k), np.int64))
    want = sg.merge_groups(*per_query, ptr, k)
    _same(got, want, what)
    two = ix.search_groups(q, k, group_ptr=ptr, normalize=False, **kw)           # group_ptr instead of sizes, no `which`
    assert len(two) == 2
    _same(two, want[:2], what)
    return got, per_query


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("dim", sg.DIMS)
def test_exact_rows_equal_the_merge_of_the_plain_search_bit_for_bit(dim, dtype):
    for layout in sg.LAYOUTS:
        c, q, sizes = sg.exact_case(dim, layout)
        ix = _index(c, dtype=dtype)
        ptr = sg.ptr_of(sizes)
        for k in sg.KS:
            if max(sizes) * k > sg.MAX_ENTRIES:
                continue
            got, _ = _groups_vs_restatement(ix, q, k, sizes, (dim, dtype, layout, k))
            for g, n in enumerate(sizes):
                if n == 0:
                    assert np.isneginf(got[0][g]).all() and (got[1][g] == -1).all() and (got[2][g] == -1).all()
                if n == 1:                                                    # a group of one is the search of that query alone
                    one = ix.search(q[ptr[g]:ptr[g] + 1], k, normalize=False)
                    _same((got[0][g], got[1][g]), (one[0][0], one[1][0]), (dim, dtype, layout, k, g))
                    assert (got[2][g] == 0).all()
        ix.close()
    # every k of the grid met the largest group it allows: 16 queries at k = 256 is exactly 4096 entries
    assert max(sg.LAYOUTS["mixed"]) * 256 == sg.MAX_ENTRIES


def test_exactly_4096_entries_pass_and_4097_are_refused():
    from mrag_amd._native import MragError
    dim = 64
    c = sg.small_int_rows(sg.N_EXACT, dim, 601)
    ix = _index(c)
    for q_n, k in ((64, 64), (4096, 1), (20, 200)):                             # 4096, 4096, 4000 entries
        q = sg.small_int_rows(q_n + 3, dim, 602 + k)
        _groups_vs_restatement(ix, q, k, [q_n, 3], (q_n, k))
    for q_n, k in ((241, 17), (4097, 1), (17, 256), (21, 200)):                 # 4097, 4097, 4352, 4200 entries
        q = sg.small_int_rows(q_n + 1, dim, 603)
        with pytest.raises(MragError) as e:
            ix.search_groups(q, k, sizes=[1, q_n], normalize=False)
        assert e.value.code == -5 and "question 1" in str(e.value) and "4096" in str(e.value), str(e.value)
    ix.close()


def test_id_base_moves_the_ids_and_nothing_else():
    c, q, sizes = sg.exact_case(96, "mixed", seed=1)
    base = 123_456_789_012
    ix0, ix1 = _index(c), _index(c, id_base=base)
    for k in (10, 200):
        a, _ = _groups_vs_restatement(ix0, q, k, sizes)
        b, _ = _groups_vs_restatement(ix1, q, k, sizes)
        assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()
        assert (b[1] == np.where(a[1] >= 0, a[1] + base, -1)).all() and b[1][b[1] >= 0].min() >= base
    ix0.close(); ix1.close()


def test_fewer_distinct_rows_than_k():
    dim = 64
    q = sg.small_int_rows(9, dim, 611)
    sizes = [3, 1, 0, 5]
    small = _index(sg.small_int_rows(7, dim, 612))                             # a corpus smaller than k
    for k in (10, 65, 256):
        got, _ = _groups_vs_restatement(small, q, k, sizes)
        assert ((got[1] >= 0).sum(axis=1) == [7, 7, 0, 7]).all()
        assert (np.sort(got[1][0, :7]) == np.arange(7)).all()
    small.close()
    empty = _index(np.zeros((0, dim), dtype=np.float16))                       # no rows at all
    got = empty.search_groups(q, 10, sizes=sizes, normalize=False, return_which=True)
    assert np.isneginf(got[0]).all() and (got[1] == -1).all() and (got[2] == -1).all()
    empty.close()
    c = sg.small_int_rows(sg.N_EXACT, dim, 613)                                # an allow-set smaller than k
    ix = _index(c)
    allow = sg.pick(sg.N_EXACT, 5, 614)
    for k in (10, 200):
        got, _ = _groups_vs_restatement(ix, q, k, sizes, allow=allow)
        assert ((got[1] >= 0).sum(axis=1) == [5, 5, 0, 5]).all() and set(got[1][0, :5].tolist()) == set(allow.tolist())
    ix.close()


def test_duplicated_rows_and_queries_name_the_lowest_query_position():
    c, q, sizes = sg.duplicates_case()
    ix = _index(c)
    for k in (10, 200, 256):
        got, per_query = _groups_vs_restatement(ix, q, k, sizes)
        sc, ids, which = got
        assert (which[0] == 0).all()                                           # four copies of one query: every id four times, equal scores
        _same((sc[0], ids[0]), (per_query[0][0], per_query[1][0]))
        assert set(which[1].tolist()) <= {0, 1} and (which[1] == 0).any() and (which[1] == 1).any()     # (a, b, a): never position 2
        m = min(k, 100)                                                         # the identical rows lead and tie: ids ascending
        assert ids[0, :m].tolist() == list(range(100, 100 + m)) and (sc[0, :m] == 96).all()
        assert ids[1, :10].tolist() == list(range(50, 55)) + list(range(300, 305)) and which[1, :10].tolist() == [1] * 5 + [0] * 5
    ix.close()


def test_zeros_of_both_signs_for_one_id():
    """every score is a zero; the restatement and the kernel compare them as floats, so whichever signs the search emits
    the merged rows are the first query's lists (printed: whether a -0.0 was met at all)"""
    c, q, sizes = sg.signed_zero_case()
    ix = _index(c, dtype="bf16")
    for k in (1, 10, 256):
        got, per_query = _groups_vs_restatement(ix, q, k, sizes)
        assert (got[0] == 0).all() and (got[1][0] == np.arange(k)).all() and (got[2] == 0).all()
        _same((got[0][0], got[1][0]), (per_query[0][0], per_query[1][0]))
        print(f"k = {k}: the search gave {int(np.signbit(per_query[0]).sum())} negative zeros of {per_query[0].size} scores")
    ix.close()


# ------------------------------------------------------------------------------------------------ the fp64 oracle
@pytest.mark.parametrize("dim,dtype", [(64, "f16"), (96, "f16"), (768, "f16")])
def test_gaussian_rows_against_the_fp64_oracle_over_the_row_wise_max(dim, dtype):
    n, base = 5003, 1000
    sizes = sg.LAYOUTS["mixed"] + [20]
    c, q = sg.gaussian_rows(n, dim, 700 + dim), sg.gaussian_rows(int(np.sum(sizes)), dim, 800 + dim)
    ix = _index(c, id_base=base, dtype=dtype)
    for k in (1, 10, 64, 65, 200):
        sc, ids, which = ix.search_groups(q, k, sizes=sizes, normalize=False, return_which=True)
        rv, ri = sg.oracle_groups(q, c, sizes, k, id_base=base)
        _check_oracle(sc, ids, rv, ri)
        _same((sc, ids, which), sg.merge_groups(*ix.search(q, k, normalize=False), sg.ptr_of(sizes), k), (dim, k))
        # `which` names a query under which the row scores what was kept
        ptr = sg.ptr_of(sizes)
        for g in (1, 4, len(sizes) - 1):
            s64 = q[ptr[g]:ptr[g + 1]].astype(np.float64) @ c[ids[g] - base].astype(np.float64).T
            assert np.abs(s64[which[g], np.arange(k)] - sc[g]).max() <= sg.TOL
    ix.close()


# ------------------------------------------------------------------------------------------------ position
def test_a_question_does_not_depend_on_its_place_or_its_neighbours():
    c, pq, fq, fsizes = sg.position_case()
    ix = _index(c)
    for k in (10, 200):
        alone = ix.search_groups(pq, k, sizes=[len(pq)], normalize=False, return_which=True)
        _check_oracle(alone[0], alone[1], *sg.oracle_groups(pq, c, [len(pq)], k))
        first = None
        for at in (0, sg.B_POS // 2, sg.B_POS - 1):
            q, sizes = sg.place(pq, fq, fsizes, at)
            got = ix.search_groups(q, k, sizes=sizes, normalize=False, return_which=True)
            if at == 0:
                first = [x[0].copy() for x in got]
                _check_oracle(got[0], got[1], *sg.oracle_groups(q, c, sizes, k))
            _same([x[at] for x in got], first, (k, at))
        # alone it may be served by another search kernel: the same rows within the oracle's yardstick
        _check_oracle(alone[0], alone[1], first[0][None, :].astype(np.float64), first[1][None, :])
    ix.close()


# ------------------------------------------------------------------------------------------------ device buffers
def test_cuda_queries_and_out_give_the_bits_of_host_buffers():
    import torch
    c, q, sizes = sg.exact_case(96, "mixed", seed=2)
    g_rows, g_q = sg.gaussian_rows(3000, 96, 901), sg.gaussian_rows(len(q), 96, 902)
    for rows, qs in ((c, q), (g_rows, g_q)):
        ix = _index(rows)
        for k in (10, 200):
            host = ix.search_groups(qs, k, sizes=sizes, normalize=False, return_which=True)
            dq = torch.from_numpy(qs).cuda()
            dev = ix.search_groups(dq, k, sizes=sizes, normalize=False, return_which=True)
            assert all(t.is_cuda for t in dev)
            torch.cuda.synchronize()
            _same([t.cpu().numpy() for t in dev], host, k)
            out = (torch.full((len(sizes), k), 5.0, device="cuda"), torch.full((len(sizes), k), 5, dtype=torch.int64, device="cuda"),
                   torch.full((len(sizes), k), 5, dtype=torch.int32, device="cuda"))
            back = ix.search_groups(dq, k, sizes=sizes, normalize=False, out=out, return_which=True)
            assert all(a is b for a, b in zip(back, out))
            torch.cuda.synchronize()
            _same([t.cpu().numpy() for t in out], host, k)
            two = ix.search_groups(dq, k, sizes=sizes, normalize=False)            # no `which` buffer at all
            torch.cuda.synchronize()
            _same([t.cpu().numpy() for t in two], host[:2], k)
        ix.close()


# ------------------------------------------------------------------------------------------------ allow=
def test_an_allow_set_gives_the_merge_of_the_filtered_search():
    c, q, sizes = sg.exact_case(96, "mixed", seed=3)
    ix = _index(c)
    for m in (300, 1500):
        allow = sg.pick(sg.N_EXACT, m, 910 + m)
        mask = np.isin(np.arange(sg.N_EXACT), allow)
        for k in (10, 200):
            got, _ = _groups_vs_restatement(ix, q, k, sizes, allow=allow)
            assert np.isin(got[1][got[1] >= 0], allow).all()
            _same(ix.search_groups(q, k, sizes=sizes, normalize=False, allow=mask, return_which=True), got)
            assert ix.last_filter()["allowed"] == m
    ix.close()


# ------------------------------------------------------------------------------------------------ the other searches
def test_the_other_searches_are_left_alone():
    n, dim = 6000, 96
    c, q = sg.gaussian_rows(n, dim, 921), sg.gaussian_rows(44, dim, 922)
    sizes = sg.LAYOUTS["mixed"]
    sets = [sg.pick(n, 300, 923), sg.pick(n, 40, 924)]
    set_of = (np.arange(44) % 2).astype(np.int32)
    cand = (np.arange(0, 441, 10), sg.pick(n, 440, 925))
    ix = _index(c)
    for nq, k in ((1, 10), (40, 10), (3, 200)):
        before = (ix.search(q[:nq], k, normalize=False), ix.search_sets(q, k, sets, set_of=set_of, normalize=False),
                  ix.score_rows_batch(q, cand, normalize=False))
        ix.search_groups(q, k, sizes=sizes, normalize=False)
        after = (ix.search(q[:nq], k, normalize=False), ix.search_sets(q, k, sets, set_of=set_of, normalize=False),
                 ix.score_rows_batch(q, cand, normalize=False))
        for a, b in zip(before, after):
            _same(a, b, (nq, k))
    ix.close()


# ------------------------------------------------------------------------------------------------ refusals
def _raw(ix, q, k, ptr, nq=None, n_groups=None, dtype=None, h=None, null=(), allow=None, allow_n=0):
    """the C call itself on output buffers pre-filled with UNTOUCHED -> (status, message, scores, ids, which)"""
    from mrag_amd import _native as N
    lib = N.load()
    q = np.ascontiguousarray(q, dtype=np.float32)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    rows = max(len(ptr) - 1, 1)
    sc = np.full((rows, max(k, 1)), float(UNTOUCHED), dtype=np.float32)
    ids, wh = np.full(sc.shape, UNTOUCHED, dtype=np.int64), np.full(sc.shape, UNTOUCHED, dtype=np.int32)
    bufs = {"q": q.ctypes.data, "ptr": ptr.ctypes.data, "sc": sc.ctypes.data, "ids": ids.ctypes.data, "wh": wh.ctypes.data}
    for name in null:
        bufs[name] = None
    st = lib.mrag_index_search_groups(ix._h if h is None else h, bufs["q"], len(q) if nq is None else nq,
                                      N.MRAG_F32 if dtype is None else dtype, 0, 0, k, len(ptr) - 1 if n_groups is None else n_groups,
                                      bufs["ptr"], None if allow is None else allow.ctypes.data, allow_n, N.ALLOW_BITS32,
                                      bufs["sc"], bufs["ids"], bufs["wh"], 0, None)
    return st, (lib.mrag_last_error() or b"").decode(), sc, ids, wh


def test_refusals_leave_the_outputs_untouched_and_name_the_question():
    n, dim = 500, 64
    c = sg.small_int_rows(n, dim, 931)
    q = sg.small_int_rows(5, dim, 932)
    ix = _index(c)
    ptr = [0, 2, 2, 5]
    st, _, sc, ids, wh = _raw(ix, q, 4, ptr)
    assert st == 0
    _same((sc, ids, wh), sg.merge_groups(*ix.search(q, 4, normalize=False), ptr, 4))
    st, _, sc, ids, wh = _raw(ix, q, 4, ptr, null=("wh",))                     # out_which may be NULL
    assert st == 0 and (wh == UNTOUCHED).all()
    _same((sc, ids), sg.merge_groups(*ix.search(q, 4, normalize=False), ptr, 4)[:2])
    INVALID, UNSUPPORTED = -1, -5
    bits = np.zeros((n + 31) // 32, dtype=np.uint32)
    cases = [
        (dict(nq=-1), INVALID, "nq"),
        (dict(n_groups=-1), INVALID, "n_groups"),
        (dict(ptr=[1, 2, 2, 5]), INVALID, "question 0"),
        (dict(ptr=[0, 3, 2, 5]), INVALID, "question 1"),
        (dict(ptr=[0, 2, 2, 4]), INVALID, "question 2"),
        (dict(ptr=[0, 2, 2, 6]), INVALID, "question 2"),
        (dict(null=("q",)), INVALID, "NULL"), (dict(null=("ptr",)), INVALID, "NULL"),
        (dict(null=("sc",)), INVALID, "NULL"), (dict(null=("ids",)), INVALID, "NULL"),
        (dict(dtype=99), INVALID, "dtype"),
        (dict(h=0xdead), INVALID, "handle"),
        (dict(k=0), INVALID, "k"), (dict(k=-3), INVALID, "k"),
        (dict(k=257), UNSUPPORTED, "257"),
        (dict(k=256, ptr=[0, 17], q=sg.small_int_rows(17, dim, 933)), UNSUPPORTED, "question 0"),
        (dict(allow=bits, allow_n=n - 1), INVALID, "allow"),                    # an allow-set of the wrong length
    ]
    for kw, want, word in cases:
        args = dict(k=4, ptr=ptr, q=q)
        args.update(kw)
        st, msg, sc, ids, wh = _raw(ix, args.pop("q"), args.pop("k"), args.pop("ptr"), **args)
        assert st == want and word in msg, (kw, st, msg)
        assert (sc == UNTOUCHED).all() and (ids == UNTOUCHED).all() and (wh == UNTOUCHED).all(), kw
    # no questions: nothing to do, nothing written
    st, _, sc, ids, wh = _raw(ix, q[:0], 4, [0])
    assert st == 0 and (sc == UNTOUCHED).all() and (ids == UNTOUCHED).all() and (wh == UNTOUCHED).all()
    # only empty questions: all-padding rows
    st, _, sc, ids, wh = _raw(ix, q[:0], 4, [0, 0, 0])
    assert st == 0 and np.isneginf(sc).all() and (ids == -1).all() and (wh == -1).all()
    # the Python method refuses before the library is called
    for kw in (dict(sizes=[2, 2]), dict(group_ptr=[0, 6]), dict(group_ptr=[0, 3, 2, 5]), dict(), dict(sizes=[5], group_ptr=[0, 5])):
        with pytest.raises(ValueError):
            ix.search_groups(q, 4, normalize=False, **kw)
    with pytest.raises(ValueError):
        ix.search_groups(q, 257, sizes=[5])
    ix.close()


def test_last_groups_before_the_first_call_is_refused():
    from mrag_amd._native import MragError
    ix = _index(sg.small_int_rows(10, 64, 941))
    with pytest.raises(MragError):
        ix.last_groups()
    ix.close()


# ------------------------------------------------------------------------------------------------ the backend
class _Router:
    def embed(self, *, model_hint, texts, require=None):
        return {"vectors": [sg.pm1_vec(t) for t in texts]}


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


@pytest.mark.parametrize("variant", ["bm25", "bm25-fused-on-device", "filter", "dense-only", "not-dense-expanded"])
def test_run_batch_gives_every_request_the_hits_of_run_with_an_expander(docs, variant):
    import filter_sets_cases as fs
    from mrag_amd.backend import DenseRetrievalBackend
    kw = dict(index_path=docs, dense_pool_k=100, query_expander=sg.expander, dense_expanded=variant != "not-dense-expanded")
    if variant != "dense-only":
        kw["text_channel"] = "bm25"
    if variant == "bm25-fused-on-device":
        kw["fuse_on_device"] = True
    if variant == "filter":
        kw["dense_row_filter"] = fs.three_sets_or_none
    reqs = _requests()
    b = DenseRetrievalBackend(_Router(), **kw)
    got = b.run_batch(reqs)
    filtered = 0
    for g, r in enumerate(reqs):
        want = b.run(r)
        assert want["diagnostics"]["dense_error"] is None and want["hits"], (g, r.query)
        assert got[g]["hits"] == want["hits"], (variant, g, r.query)
        diag = dict(got[g]["diagnostics"])
        assert diag.pop("batch_size") == len(reqs) and diag == want["diagnostics"], (variant, g)
        assert diag["queries"] == [r.query] + sg.expander(query=r.query, trace_id="t") and "expand_error" not in diag
        filtered += "dense_filter" in diag
    assert (filtered > 0) == (variant == "filter")
    if variant == "filter":                                                   # dense_filter_batch has no effect on expanded requests
        on = DenseRetrievalBackend(_Router(), dense_filter_batch=True, **kw).run_batch(reqs)
        assert [o["hits"] for o in on] == [o["hits"] for o in got]
        assert [o["diagnostics"] for o in on] == [o["diagnostics"] for o in got]


def test_expanded_dense_hits_cover_the_plain_ones_by_score(docs):
    from mrag_amd.backend import DenseRetrievalBackend
    kw = dict(index_path=docs, dense_pool_k=100, alpha_text=0.0, alpha_graph=0.0, alpha_dense=1.0)
    plain = DenseRetrievalBackend(_Router(), **kw)
    text_only = DenseRetrievalBackend(_Router(), query_expander=sg.expander, **kw)           # the dense channel uses req.query alone
    wide = DenseRetrievalBackend(_Router(), query_expander=sg.expander, dense_expanded=True, **kw)
    from mrag_amd.backend import resolve_embed_model
    ix = wide._get_state(resolve_embed_model(wide.router), "t")["index"]
    for r in _requests()[:9]:
        queries = [r.query] + sg.expander(query=r.query, trace_id="t")
        Q = np.asarray([sg.pm1_vec(t) for t in queries], dtype=np.float32)
        one = ix.search(Q[:1], 100)
        many = ix.search_groups(Q, 100, sizes=[len(queries)], return_which=True)
        # per id, the expanded score is at least the plain one; an id that drops out is beaten by the expanded k-th score
        exp = dict(zip(many[1][0].tolist(), many[0][0].tolist()))
        for i, s in zip(one[1][0].tolist(), one[0][0].tolist()):
            assert exp.get(i, many[0][0, -1]) >= s
        assert (many[2][0] >= 0).all() and (many[2][0] < len(queries)).all()
        # through the backend: the hits of the text-only expansion are the plain backend's, the expanded ones rank by the merged scores
        a, b, c = plain.run(r), text_only.run(r), wide.run(r)
        assert a["hits"] == b["hits"] and b["diagnostics"]["queries"] == queries == c["diagnostics"]["queries"]
        assert a["diagnostics"]["queries"] == [r.query]
        assert c["diagnostics"]["dense_error"] is None and c["diagnostics"]["pool"]["dense_pool_k_effective"] == min(max(r.top_k, 100), 256)


def test_a_failing_expander_gives_the_plain_result_and_too_many_queries_a_dense_error(docs):
    from mrag_amd.backend import DenseRetrievalBackend
    kw = dict(index_path=docs, dense_pool_k=200, text_channel="bm25")
    reqs = _requests()[:6]
    plain = DenseRetrievalBackend(_Router(), **kw)
    down = DenseRetrievalBackend(_Router(), query_expander=sg.failing_expander, dense_expanded=True, **kw)
    batch = down.run_batch(reqs)
    for g, r in enumerate(reqs):
        want, got = plain.run(r), down.run(r)
        assert got["hits"] == want["hits"] == batch[g]["hits"] and want["hits"]
        assert "the expander is down" in got["diagnostics"]["expand_error"] and got["diagnostics"]["queries"] == [r.query]
        assert batch[g]["diagnostics"]["expand_error"] == got["diagnostics"]["expand_error"]
        assert "expand_error" not in want["diagnostics"]
    # 25 queries x the pool of 200 exceed the merge's 4096 entries: reported like any other dense failure, in run and in run_batch
    many = DenseRetrievalBackend(_Router(), query_expander=sg.long_expander, dense_expanded=True, **kw)
    batch = many.run_batch(reqs)
    for g, r in enumerate(reqs):
        got = many.run(r)
        assert "4096" in got["diagnostics"]["dense_error"] and got["hits"]
        assert batch[g]["hits"] == got["hits"] and batch[g]["diagnostics"]["dense_error"] == got["diagnostics"]["dense_error"]
