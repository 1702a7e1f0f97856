"""GPU parity of the range search (DenseIndex.range_search, mrag_index_search_range) and of the self-join built on it
(DenseIndex.self_join, pairwise.semantic_edges_index), against an fp64 oracle over the same fp16 / bf16 bits: the rows
scoring >= a floor, the best min(k, c) of them, and c itself."""
import numpy as np
import pytest

from oracle import dense_search as ds

pytestmark = pytest.mark.gpu
TOL = 1e-5
PATHS = ("mask", "compact", "auto")


def _index(c, id_base=0, **kw):
    from mrag_amd.index import DenseIndex
    ix = DenseIndex(c.shape[1], **kw)
    if id_base:
        ix.set_id_base(id_base)
    ix.add(c, normalize=False)
    return ix


def _scores(q, c, mask=None):
    s = np.asarray(q, dtype=np.float64) @ np.asarray(c, dtype=np.float64).T
    if mask is not None:
        s[:, ~mask] = -np.inf
    return s


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _check_range(sc, ids, cnt, S, floor, k, id_base=0, tol=TOL):
    """The contract, checked against the fp64 scores S [nq, n] (rows within tol of the floor are not held against it)."""
    sc, ids, cnt = _np(sc), _np(ids), _np(cnt)
    nq, n = S.shape
    assert sc.shape == (nq, k) and ids.shape == (nq, k) and cnt.shape == (nq,) and cnt.dtype == np.int64
    f = np.float32(floor)
    lo, hi = (S >= floor + tol).sum(1), (S >= floor - tol).sum(1)
    assert (cnt >= lo).all() and (cnt <= hi).all(), "count outside the oracle's band"
    valid = ids >= 0
    assert (valid.sum(1) == np.minimum(cnt, k)).all(), "valid slots != min(count, k)"
    assert (np.diff(valid.astype(np.int8), axis=1) <= 0).all(), "valid slots are not a prefix"
    assert np.isneginf(sc[~valid]).all() and (ids[~valid] == -1).all()
    assert (sc[valid] >= f).all(), "a returned score lies below the floor"
    rows = ids - id_base
    qi = np.nonzero(valid)[0]
    np.testing.assert_allclose(sc[valid], S[qi, rows[valid]], rtol=0, atol=tol)
    # (score desc, row asc)
    both = valid[:, 1:] & valid[:, :-1]
    with np.errstate(invalid="ignore"):
        d = np.diff(sc, axis=1)
    assert (d[both] <= 0).all()
    assert (np.diff(rows, axis=1)[both & (d == 0)] > 0).all()
    # completeness: every row clearly above the query's cut is listed
    n_l = valid.sum(1)
    last = np.where(n_l > 0, sc[np.arange(nq), np.maximum(n_l - 1, 0)], np.inf).astype(np.float64)
    cut = np.where(n_l < k, float(floor), np.maximum(last, float(floor)))
    listed = np.zeros(S.shape, dtype=bool)
    listed[qi, rows[valid]] = True
    missing = (S >= cut[:, None] + tol) & ~listed
    assert not missing.any(), f"{int(missing.sum())} rows above the cut are missing"
    # positions: the oracle's top rows among those >= floor (near-ties and the TOL band around the floor excepted)
    rv, ri = ds.topk_desc_rowasc(np.where(S >= floor, S, -np.inf), k)
    if rv.shape[1] < k:
        pad = k - rv.shape[1]
        rv = np.concatenate([rv, np.full((nq, pad), -np.inf)], 1)
        ri = np.concatenate([ri, np.full((nq, pad), -1, dtype=np.int64)], 1)
    ri = np.where(rv >= floor + tol, ri + id_base, -1)
    strict, bad = ds.gap_aware_id_match(ids, sc, ri, rv, tol=tol)
    assert bad == 0, (strict, bad)
    return cnt


def _floor_for(S, k, frac=0.5):
    """a floor near the median k-th best score: some queries are truncated, others keep fewer than k rows"""
    kth = np.sort(S, axis=1)[:, -k]
    return float(np.quantile(kth, frac))


# (nq, n, d, k): streaming (nq <= 16, and nq <= 8 with k > 32, k = 200 included), dense batch, 17 000 queries (two
# launches of the query-batch loop), wide batch (nq > 32, 64 < k <= 256, >= 64 corpus tiles); dims not multiples of 64
SHAPES = [(1, 20000, 384, 10), (5, 30000, 200, 200), (16, 5000, 96, 20),
          (300, 20000, 768, 10), (40, 3000, 130, 64), (17000, 4000, 64, 5),
          (100, 20000, 72, 200)]


@pytest.mark.parametrize("nq,n,d,k", SHAPES)
def test_range_regimes(nq, n, d, k):
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 1000 + d))
    q16 = ds.normalize_round(ds.make_gaussian(nq, d, 2000 + d))
    ix = _index(c16)
    S = _scores(q16, c16)
    floor = _floor_for(S, k)
    sc, ids, cnt = ix.range_search(q16, floor, k, normalize=False)
    cnt = _check_range(sc, ids, cnt, S, floor, k)
    if nq >= 16:
        assert (cnt > k).any() and (cnt < k).any()
    ix.close()


def test_range_mixed_hits_in_one_batch():
    """One batch (streaming and batch kernels) with queries that reach nothing, fewer than k rows, and more than k."""
    d, n, k = 64, 30000, 10
    rng = np.random.default_rng(7)
    u = ds.l2_normalize(rng.standard_normal((1, d)))[0]
    base = rng.standard_normal((n, d)).astype(np.float32)
    base[:400] = u + 0.1 * rng.standard_normal((400, d)).astype(np.float32)    # a hub of 400 rows around u
    c16 = ds.normalize_round(base)
    # queries cycle through three kinds: near u (hundreds of hits), random (none), a noisy copy of one row (a few)
    qs = rng.standard_normal((600, d)).astype(np.float32)
    qs[0::3] = u + 0.05 * rng.standard_normal((200, d)).astype(np.float32)
    qs[2::3] = base[rng.integers(400, n, size=200)] + 0.5 * rng.standard_normal((200, d)).astype(np.float32)
    q16 = ds.normalize_round(qs)
    ix = _index(c16)
    floor = 0.6
    for nq in (12, 600):
        S = _scores(q16[:nq], c16)
        sc, ids, cnt = ix.range_search(q16[:nq], floor, k, normalize=False)
        cnt = _check_range(sc, ids, cnt, S, floor, k)
        assert (cnt == 0).any() and ((cnt > 0) & (cnt < k)).any() and (cnt > k).any()
    ix.close()


@pytest.mark.parametrize("nq,n,d,k", [(3, 20000, 128, 10), (300, 20000, 128, 10), (100, 20000, 64, 200)])
def test_range_floor_properties(nq, n, d, k):
    """Floor below every score: bit-identical to search / the filtered search, counts = searched rows.
    Floor above every score: all (-inf, -1), counts 0.  Plain and every filter path."""
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 31))
    q16 = ds.normalize_round(ds.make_gaussian(nq, d, 32))
    ix = _index(c16, id_base=123)
    s0, i0 = ix.search(q16, k, normalize=False)
    sc, ids, cnt = ix.range_search(q16, -2.0, k, normalize=False)
    assert np.array_equal(sc, s0) and np.array_equal(ids, i0) and (cnt == n).all()
    sc, ids, cnt = ix.range_search(q16, 2.0, k, normalize=False)
    assert np.isneginf(sc).all() and (ids == -1).all() and (cnt == 0).all()
    mask = np.random.default_rng(33).random(n) < 0.3
    for path in PATHS:
        sf, idf = ix.search(q16, k, normalize=False, allow=mask, filter_path=path)
        sc, ids, cnt = ix.range_search(q16, -2.0, k, normalize=False, allow=mask, filter_path=path)
        assert np.array_equal(sc, sf) and np.array_equal(ids, idf) and (cnt == int(mask.sum())).all(), path
        if path != "auto":
            assert ix.last_filter()["path"] == path
        sc, ids, cnt = ix.range_search(q16, 2.0, k, normalize=False, allow=mask, filter_path=path)
        assert np.isneginf(sc).all() and (ids == -1).all() and (cnt == 0).all()
        # and an ordinary floor over the allowed rows only
        S = _scores(q16, c16, mask)
        floor = _floor_for(np.where(np.isfinite(S), S, -1.0), k)
        sc, ids, cnt = ix.range_search(q16, floor, k, normalize=False, allow=mask, filter_path=path)
        _check_range(sc, ids, cnt, S, floor, k, id_base=123)
    ix.close()


@pytest.mark.parametrize("nq", [4, 300])
def test_range_exact_counts_integer_ip(nq):
    """Integer-valued rows, inner product: every fp32 sum is exact.  A row exactly at the floor is included and counted;
    ties across the k boundary break by row."""
    d, n, k = 64, 12000, 10
    rng = np.random.default_rng(41)
    c = rng.integers(-3, 4, size=(n, d)).astype(np.float16)
    q = rng.integers(-3, 4, size=(nq, d)).astype(np.float16)
    ix = _index(c, metric="ip")
    S = _scores(q, c)
    top0 = np.sort(S[0])[::-1]
    # query 0's 5th best score (a row exactly at the floor inside the k returned) and its 3k-th (ties across the cut)
    for floor in (float(top0[4]), float(top0[3 * k])):
        sc, ids, cnt = ix.range_search(q, floor, k, normalize=False)
        exact = (S >= floor).sum(1)
        assert np.array_equal(cnt, exact)
        rv, ri = ds.topk_desc_rowasc(np.where(S >= floor, S, -np.inf), k)
        ri = np.where(np.isfinite(rv), ri, -1)
        rv = np.where(np.isfinite(rv), rv, -np.inf)
        assert np.array_equal(ids, ri) and np.array_equal(sc.astype(np.float64), rv)
        assert (S == floor).sum() > 0
        if floor == float(top0[4]):
            assert (sc[0] == np.float32(floor)).any()     # the row exactly at the floor came back
    ix.close()


def test_range_replay_path_no_double_count():
    """Increasing scores in storage order (every tile beats the last: the batch kernel replays its tiles) -- counts
    exact, lists exact."""
    d, n, nq, k = 64, 6000, 300, 10
    u = ds.l2_normalize(ds.make_gaussian(1, d, 9))[0]
    a = np.linspace(0.05, 1.0, n, dtype=np.float32)
    c = (a[:, None] * u[None, :]).astype(np.float16)
    q = ds.normalize_round(u[None, :] + 0.01 * ds.make_gaussian(nq, d, 10))
    ix = _index(c, metric="ip")
    S = _scores(q, c)
    for floor in (0.3, 0.9, -1.0):
        sc, ids, cnt = ix.range_search(q, floor, k, normalize=False)
        _check_range(sc, ids, cnt, S, floor, k)
    ix.close()


def test_range_wide_redo_no_double_count():
    """Rows stored cluster by cluster (the wide batch path flags and redoes queries): counts from the batch pass stay
    exact, lists come from the redo, both respect the floor."""
    d, k = 64, 200
    rng = np.random.default_rng(83)
    cent = rng.standard_normal((280, d)).astype(np.float32)
    rows = np.repeat(cent, 250, axis=0) + 0.05 * rng.standard_normal((280 * 250, d)).astype(np.float32)
    c2 = ds.normalize_round(rows)
    q2 = ds.normalize_round(cent[rng.integers(0, 280, size=200)] + 0.01 * rng.standard_normal((200, d)).astype(np.float32))
    ix = _index(c2)
    S = _scores(q2, c2)
    for floor in (_floor_for(S, k), 0.99, -2.0):
        sc, ids, cnt = ix.range_search(q2, floor, k, normalize=False)
        _check_range(sc, ids, cnt, S, floor, k)
    ix.range_search(q2, _floor_for(S, k, 0.9), k, normalize=False)
    assert ix.last_wide_redone() > 0
    ix.close()


@pytest.mark.parametrize("nq,k", [(8, 10), (200, 64)])
def test_range_bf16_and_id_base(nq, k):
    import torch
    n, d = 20000, 96
    c = ds.l2_normalize(ds.make_gaussian(n, d, 51))
    cb = torch.from_numpy(c).to(torch.bfloat16)
    q = ds.l2_normalize(ds.make_gaussian(nq, d, 52))
    qb = torch.from_numpy(q).to(torch.bfloat16)
    from mrag_amd.index import DenseIndex
    ix = DenseIndex(d, dtype="bf16")
    ix.set_id_base(10_000)
    ix.add(cb, normalize=False)
    S = _scores(qb.float().numpy(), cb.float().numpy())
    floor = _floor_for(S, k)
    sc, ids, cnt = ix.range_search(qb, floor, k, normalize=False)
    _check_range(sc, ids, cnt, S, floor, k, id_base=10_000)
    ix.close()


def test_range_device_tensors_side_stream():
    import torch
    n, d, nq, k = 20000, 128, 300, 20
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 61))
    q16 = ds.normalize_round(ds.make_gaussian(nq, d, 62))
    ix = _index(c16)
    S = _scores(q16, c16)
    floor = _floor_for(S, k)
    side = torch.cuda.Stream()
    qd = torch.from_numpy(q16).cuda()
    side.wait_stream(torch.cuda.current_stream())
    out = (torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"),
           torch.empty(nq, dtype=torch.int64, device="cuda"))
    with torch.cuda.stream(side):
        sc, ids, cnt = ix.range_search(qd, floor, k, normalize=False, stream=side, out=out)
    side.synchronize()
    assert sc.is_cuda and ids.is_cuda and cnt.is_cuda and sc.data_ptr() == out[0].data_ptr() and cnt.data_ptr() == out[2].data_ptr()
    _check_range(sc, ids, cnt, S, floor, k)
    # device allow mask
    mask = np.random.default_rng(63).random(n) < 0.5
    sc, ids, cnt = ix.range_search(qd, floor, k, normalize=False, allow=torch.from_numpy(mask).cuda(), filter_path="mask")
    torch.cuda.synchronize()
    _check_range(sc, ids, cnt, _scores(q16, c16, mask), floor, k)
    ix.close()


def test_range_errors():
    from mrag_amd.index import DenseIndex
    c16 = ds.normalize_round(ds.make_gaussian(1000, 64, 71))
    ix = _index(c16)
    q = c16[:2]
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            ix.range_search(q, bad, 10)
    for k in (0, 257, -1):
        with pytest.raises(ValueError):
            ix.range_search(q, 0.5, k)
    with pytest.raises(ValueError):
        ix.range_search(q, 0.5, 10, precision="fp8")
    ix.close()
    f8 = DenseIndex(64, fp8_scan=True)
    f8.add(c16, normalize=False)
    with pytest.raises(ValueError):
        f8.range_search(q, 0.5, 10, precision="fp8")
    f8.close()


def _pairs_oracle(c, floor, tol=TOL):
    """(sure, possible) pair sets of the fp64 self-join: sure = sim >= floor + tol, possible = sim >= floor - tol"""
    S = _scores(c, c)
    np.fill_diagonal(S, -np.inf)
    iu, ju = np.triu_indices(S.shape[0], k=1)
    s = S[iu, ju]
    sure = set(zip(iu[s >= floor + tol].tolist(), ju[s >= floor + tol].tolist()))
    possible = set(zip(iu[s >= floor - tol].tolist(), ju[s >= floor - tol].tolist()))
    return S, sure, possible


def test_self_join_planted_duplicates_batches():
    import torch
    from mrag_amd.pairwise import semantic_edges_index
    rng = np.random.default_rng(91)
    n, d = 5000, 64
    base = rng.standard_normal((n, d)).astype(np.float32)
    src = rng.integers(0, n, size=600)
    dst = rng.integers(0, n, size=600)
    base[dst] = base[src] + 0.15 * rng.standard_normal((600, d)).astype(np.float32)   # planted near-duplicates
    hub = rng.integers(0, n, size=90)
    base[hub] = base[hub[0]] + 0.05 * rng.standard_normal((90, d)).astype(np.float32)   # one cluster of 90 > k rows
    c16 = ds.normalize_round(base)
    ix = _index(c16, id_base=77)
    floor, k = 0.9, 32
    S, sure, possible = _pairs_oracle(c16, floor)
    ref = None
    for batch in (n, 1700, 16):
        sc, ids, cnt = ix.self_join(floor, k=k, batch=batch)
        torch.cuda.synchronize()
        got = (sc.cpu().numpy(), ids.cpu().numpy(), cnt.cpu().numpy())
        if ref is None:
            ref = got
            _check_range(got[0], got[1], got[2], S, floor, k, id_base=77)
            assert not (got[1] == (np.arange(n) + 77)[:, None]).any()     # no row lists itself
        else:
            for a, b in zip(ref, got):
                assert np.array_equal(a, b), f"batch {batch} changed the result"
    edges, trunc = semantic_edges_index(ix, floor, k=k, batch=1700)
    es = {(i, j) for i, j, _ in edges}
    assert all(i < j for i, j in es) and [(i, j) for i, j, _ in edges] == sorted(es)
    assert set(trunc.tolist()) == set(np.nonzero(ref[2] > k)[0].tolist()) and len(trunc) > 0
    full = np.setdiff1d(np.arange(n), trunc)
    fullset = set(full.tolist())
    # rows that are not truncated keep all their pairs; every edge is a possible pair with the fp64 similarity
    assert {p for p in sure if p[0] in fullset or p[1] in fullset} <= es
    assert es <= possible
    for i, j, v in edges[:2000]:
        assert abs(v - S[i, j]) <= TOL
    ix.close()


def test_self_join_exact_duplicates_self_exclusion():
    """Exact duplicate rows tie with the row itself: only the row's own entry goes, every duplicate stays, counts
    exclude the row itself; more duplicates than k + 1 (own entry not listed) and an ip index where rows miss the floor."""
    import torch
    rng = np.random.default_rng(95)
    d = 64
    base = ds.normalize_round(rng.standard_normal((3000, d)).astype(np.float32))
    dup = np.repeat(base[:1], 40, axis=0)          # 40 identical rows
    dup5 = np.repeat(base[1:2], 5, axis=0)         # 5 identical rows
    c16 = np.concatenate([base[2:1000], dup, base[1000:2000], dup5, base[2000:]], 0)
    n = c16.shape[0]
    ix = _index(c16)
    for k in (8, 64):
        sc, ids, cnt = ix.self_join(0.999, k=k, batch=1000)
        torch.cuda.synchronize()
        sc, ids, cnt = sc.cpu().numpy(), ids.cpu().numpy(), cnt.cpu().numpy()
        S = _scores(c16, c16)
        exact = (S >= 0.999).sum(1) - 1
        assert np.array_equal(cnt, exact)
        assert not (ids == np.arange(n)[:, None]).any()
        g40 = np.arange(998, 1038)
        for r in g40:
            want = [x for x in g40 if x != r][:k]
            assert ids[r, :len(want)].tolist() == want
    ix.close()
    # inner product: a row's own score may sit below the floor
    c = rng.integers(-2, 3, size=(2000, d)).astype(np.float16)
    c[::2, 16:] = 0                                   # half the rows: self score well below the floor
    ixp = _index(c, metric="ip")
    sc, ids, cnt = ixp.self_join(40.0, k=16, batch=700)
    torch.cuda.synchronize()
    S = _scores(c, c)
    self_s = np.diag(S).copy()
    np.fill_diagonal(S, -np.inf)
    assert np.array_equal(cnt.cpu().numpy(), (S >= 40.0).sum(1))
    assert (self_s < 40.0).any() and (self_s >= 40.0).any()
    ixp.close()
