"""GPU parity of the IVF range search (IVFFlatIndex.range_search, mrag_ivf_search_range), of the neighbour join built on
it (IVFFlatIndex.self_join, mrag_ivf_self_join) and of pairwise.semantic_edges_index over an IVF index.

The oracle is fp64 over the same fp16 / bf16 bits: S = q @ c.T, set to -inf outside the rows of the query's probed lists
(the nprobe best centroids by (score desc, list id asc), the index's own assignments).  Per query: the rows >= the floor,
the best min(k, c) of them, and c itself.  A query whose nprobe-th and (nprobe+1)-th centroid scores lie within TOL of
each other may probe another list in fp32: such queries are left out, and must be at most 1 % of the batch."""
import os
import subprocess
import sys
import tempfile
import textwrap

import numpy as np
import pytest

from oracle import dense_search as ds

pytestmark = pytest.mark.gpu
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _ivf(c, cen, id_base=0, **kw):
    from mrag_amd.index import IVFFlatIndex
    ix = IVFFlatIndex(c.shape[1], cen.shape[0], **kw)
    ix.set_centroids(cen, normalize=False)
    if id_base:
        ix.set_id_base(id_base)
    ix.add(c, normalize=False)
    return ix


def _f64(x):
    return (x.float().numpy() if hasattr(x, "float") else np.asarray(x)).astype(np.float64)


def _probed_oracle(q, c, cen, assign, nprobe):
    """-> (S [nq, n] fp64 with -inf outside the probed lists, ambiguous [nq] bool, probed lists [nq, nprobe])"""
    q, c, cen = _f64(q), _f64(c), _f64(cen)
    nq, nlist = q.shape[0], cen.shape[0]
    cs = q @ cen.T
    pv, pl = ds.topk_desc_rowasc(cs, min(nprobe + 1, nlist))
    amb = np.zeros(nq, dtype=bool)
    if nprobe < nlist:
        amb = (pv[:, nprobe - 1] - pv[:, nprobe]) <= TOL
    pl = pl[:, :nprobe]
    probed = np.zeros((nq, nlist), dtype=bool)
    probed[np.arange(nq)[:, None], pl] = True
    S = q @ c.T
    S[~probed[:, np.asarray(assign, dtype=np.int64)]] = -np.inf
    return S, amb, pl


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


def _floor_for(S, k):
    """the median k-th best probed score: some queries are truncated, others keep fewer than k rows"""
    kth = np.sort(np.sort(S, axis=1)[:, -k])
    f = float(kth[len(kth) // 2])
    assert np.isfinite(f)
    return f


def _keep(amb, *arrays):
    assert amb.sum() <= 0.01 * len(amb), f"{int(amb.sum())} of {len(amb)} queries have an ambiguous probe set"
    return [_np(a)[~amb] for a in arrays]


def _setup(n, nq, d, nlist, seed, n_centroids):
    rows, qs = ds.make_clustered(n, nq, d, seed, n_centroids=n_centroids)
    c16, q16 = ds.normalize_round(rows), ds.normalize_round(qs)
    cen = ds.kmeans_spherical(c16, nlist, 4, seed=3)
    return c16, q16, cen


# register path with the per-wave bound | one segment, k > 16 (workgroup bound) | lists up to ~7 500 rows, > 8 192 candidates
# per query (streamed path) | d not a multiple of 64
PATH_CASES = [(20000, 300, 128, 64, 8, 10, 7, 64), (20000, 300, 128, 64, 1, 200, 7, 64),
              (60000, 40, 96, 16, 12, 64, 11, 16), (30000, 500, 200, 128, 16, 32, 5, 64)]


@pytest.mark.parametrize("n,nq,d,nlist,nprobe,k,seed,n_centroids", PATH_CASES)
def test_ivf_range_paths_against_oracle(n, nq, d, nlist, nprobe, k, seed, n_centroids):
    c16, q16, cen = _setup(n, nq, d, nlist, seed, n_centroids)
    ix = _ivf(c16, cen)
    assign = ix.assignments()
    S, amb, _ = _probed_oracle(q16, c16, cen, assign, nprobe)
    floor = _floor_for(S, k)
    sc, ids, cnt = ix.range_search(q16, floor, k, nprobe, normalize=False)
    sc, ids, cnt = _keep(amb, sc, ids, cnt)
    cnt = _check_range(sc, ids, cnt, S[~amb], floor, k)
    print(f"candidates per query max {int(np.isfinite(S).sum(1).max())}, counts min {cnt.min()} max {cnt.max()}, ambiguous {int(amb.sum())}")
    assert (cnt > k).any() and (cnt < k).any()
    if (n, nprobe) == (60000, 12):
        assert np.isfinite(S).sum(1).max() > 8192          # the streamed path ran
    ix.close()


@pytest.mark.parametrize("n,nq,d,nlist,k", [(20000, 300, 128, 64, 10), (6000, 200, 96, 16, 64)])
def test_ivf_range_every_list_probed_equals_dense(n, nq, d, nlist, k):
    """nprobe = nlist: the same rows in a DenseIndex give the same lists and counts (the dense index may take another
    kernel for the batch: scores within TOL, ids equal outside near-ties, counts equal where no row is within TOL of the
    floor)."""
    from mrag_amd.index import DenseIndex
    c16, q16, cen = _setup(n, nq, d, nlist, 7, 64)
    ix = _ivf(c16, cen)
    dx = DenseIndex(d)
    dx.add(c16, normalize=False)
    S = _f64(q16) @ _f64(c16).T
    floor = _floor_for(S, k)
    sc, ids, cnt = ix.range_search(q16, floor, k, nlist, normalize=False)
    sd, idd, cd = dx.range_search(q16, floor, k, normalize=False)
    _check_range(sc, ids, cnt, S, floor, k)
    clear = ~(np.abs(S - floor) <= TOL).any(axis=1)          # queries with no row within TOL of the floor
    assert clear.sum() >= nq // 2                            # (a band of 2 TOL against ~1e-4 between neighbouring scores)
    assert np.array_equal(cnt[clear], cd[clear])
    assert np.array_equal(ids[clear] >= 0, idd[clear] >= 0)
    with np.errstate(invalid="ignore"):
        diff = np.where(idd[clear] >= 0, sc[clear] - sd[clear], 0.0)
    assert np.abs(diff).max() <= TOL
    assert ds.gap_aware_id_match(ids[clear], sc[clear], idd[clear], sd[clear].astype(np.float64), tol=TOL)[1] == 0
    print("bit-identical to the dense range search:", bool(np.array_equal(sc, sd) and np.array_equal(ids, idd) and np.array_equal(cnt, cd)))
    ix.close()
    dx.close()


# (the plain search serves k <= 64: the one-segment case runs at k = 64 here)
@pytest.mark.parametrize("n,nq,d,nlist,nprobe,k,seed,n_centroids",
                         [PATH_CASES[0], (20000, 300, 128, 64, 1, 64, 7, 64), PATH_CASES[2]])
def test_ivf_range_floor_below_and_above_every_score(n, nq, d, nlist, nprobe, k, seed, n_centroids):
    c16, q16, cen = _setup(n, nq, d, nlist, seed, n_centroids)
    ix = _ivf(c16, cen, id_base=1000)
    assign = ix.assignments().astype(np.int64)
    s0, i0 = ix.search(q16, k, nprobe, normalize=False)
    sc, ids, cnt = ix.range_search(q16, -2.0, k, nprobe, normalize=False)
    assert np.array_equal(sc, s0) and np.array_equal(ids, i0)
    _, amb, pl = _probed_oracle(q16, c16, cen, assign, nprobe)
    sizes = np.bincount(assign, minlength=nlist)
    want = sizes[pl].sum(1)
    cnt_k, want_k = _keep(amb, cnt, want)
    assert np.array_equal(cnt_k, want_k)
    sc, ids, cnt = ix.range_search(q16, 2.0, k, nprobe, normalize=False)
    assert np.isneginf(sc).all() and (ids == -1).all() and (cnt == 0).all() and cnt.dtype == np.int64
    ix.close()


def _integer_setup(n, nq, d, nlist, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(-3, 4, size=(n, d)).astype(np.float16)
    q = rng.integers(-3, 4, size=(nq, d)).astype(np.float16)
    cen = rng.integers(-3, 4, size=(nlist, d)).astype(np.float16)
    return c, q, cen


def _exact_expect(S, floor, k):
    rv, ri = ds.topk_desc_rowasc(np.where(S >= floor, S, -np.inf), k)
    return np.where(np.isfinite(rv), rv, -np.inf), np.where(np.isfinite(rv), ri, -1)


@pytest.mark.parametrize("nprobe", [3, 8])
def test_ivf_range_exact_ties_integer_ip(nprobe):
    """Integer-valued rows, inner product: every fp32 sum is exact (the probe selection too), so counts, lists and the
    order of ties are the oracle's exactly.  nprobe 3: register path; nprobe 8 = nlist over 12 000 rows: streamed path."""
    d, n, nq, k, nlist = 64, 12000, 300, 10, 8
    c, q, cen = _integer_setup(n, nq, d, nlist, 41)
    ix = _ivf(c, cen, metric="ip")
    S, _, _ = _probed_oracle(q, c, cen, ix.assignments(), nprobe)
    top0 = np.sort(S[0])[::-1]
    for floor in (float(top0[4]), float(top0[3 * k])):
        sc, ids, cnt = ix.range_search(q, floor, k, nprobe, normalize=False)
        assert np.array_equal(cnt, (S >= floor).sum(1))
        rv, ri = _exact_expect(S, floor, k)
        assert np.array_equal(ids, ri) and np.array_equal(sc.astype(np.float64), rv)
        assert (S == floor).sum() > 0
    ix.close()


@pytest.mark.parametrize("nprobe", [3, 8])
def test_ivf_range_more_ties_at_the_floor_than_the_shortlist(nprobe):
    """600 copies of one row, the row itself as query 0, the floor on their score: more than 512 entries tie at the bound,
    the shortlist overflows and the serial path lists the lowest rows and counts all of them."""
    d, n, nq, nlist = 64, 12000, 40, 8
    c, q, cen = _integer_setup(n, nq, d, nlist, 43)
    rng = np.random.default_rng(44)
    where = np.sort(rng.choice(n, size=600, replace=False))
    c[where] = c[where[0]]
    q[0] = c[where[0]]
    ix = _ivf(c, cen, metric="ip")
    S, _, _ = _probed_oracle(q, c, cen, ix.assignments(), nprobe)
    floor = float(S[0, where[0]])
    assert (S[0] == floor).sum() >= 600 and (S[0] > floor).sum() < 10
    for k in (10, 200):
        sc, ids, cnt = ix.range_search(q, floor, k, nprobe, normalize=False)
        assert np.array_equal(cnt, (S >= floor).sum(1)) and cnt[0] > 512
        rv, ri = _exact_expect(S, floor, k)
        assert np.array_equal(ids, ri) and np.array_equal(sc.astype(np.float64), rv)
    ix.close()


@pytest.mark.parametrize("n,nq,d,nlist,nprobe,k,seed,n_centroids", [PATH_CASES[0], PATH_CASES[2]])
def test_ivf_range_exclusion(n, nq, d, nlist, nprobe, k, seed, n_centroids):
    """exclude=e: the unexcluded result with row e[q] removed; the count is one lower exactly when that row was probed and
    reached the floor; exact duplicates of the excluded row stay; -1 changes nothing."""
    c16, q16, cen = _setup(n, nq, d, nlist, seed, n_centroids)
    q16 = q16.copy()
    q16[:20] = c16[100:120]                      # queries that are stored rows: their own row is the best hit
    c16 = c16.copy()
    c16[5000] = c16[100]                         # an exact duplicate of a row that will be excluded
    ix = _ivf(c16, cen, id_base=50)
    assign = ix.assignments()
    S, amb, _ = _probed_oracle(q16, c16, cen, assign, nprobe)
    floor = _floor_for(S, k)
    s0, i0, c0 = ix.range_search(q16, floor, k, nprobe, normalize=False)
    none = np.full(nq, -1, dtype=np.int64)
    s1, i1, c1 = ix.range_search(q16, floor, k, nprobe, normalize=False, exclude=none)
    assert np.array_equal(s0, s1) and np.array_equal(i0, i1) and np.array_equal(c0, c1)
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, size=nq).astype(np.int64)
    e[:20] = np.arange(100, 120)                 # the query's own row
    top = i0[:, 0] - 50
    e[20:60] = np.where(top[20:60] >= 0, top[20:60], e[20:60])     # the best hit of the unexcluded search
    e[60:70] = -1
    sx, ixd, cx = ix.range_search(q16, floor, k, nprobe, normalize=False, exclude=e)
    # oracle: the same scores with the excluded row removed
    Sx = S.copy()
    has = e >= 0
    Sx[np.nonzero(has)[0], e[has]] = -np.inf
    keep = ~amb
    assert amb.sum() <= 0.01 * nq
    _check_range(sx[keep], ixd[keep], cx[keep], Sx[keep], floor, k, id_base=50)
    assert not (ixd == (e + 50)[:, None])[has].any()
    f32 = np.float32(floor)
    # the excluded row was listed (so it was probed and reached the floor) -> exactly one fewer; and never more than one
    was_listed = (i0 == (e + 50)[:, None]).any(axis=1) & has
    assert was_listed.sum() >= 40
    assert (c0 - cx)[was_listed].tolist() == [1] * int(was_listed.sum())
    assert set(np.unique(c0 - cx).tolist()) <= {0, 1}
    gone = (c0 - cx) == 1
    sure_in = has & np.isfinite(S[np.arange(nq), np.maximum(e, 0)]) & (S[np.arange(nq), np.maximum(e, 0)] >= floor + TOL)
    sure_out = ~has | ~np.isfinite(S[np.arange(nq), np.maximum(e, 0)]) | (S[np.arange(nq), np.maximum(e, 0)] < floor - TOL)
    assert gone[sure_in & keep].all() and not gone[sure_out & keep].any()
    assert (s0[was_listed] >= f32).any()
    # query 0 is row 100 and excludes it: its duplicate, row 5000, stays and now leads
    assert ixd[0, 0] == 5000 + 50 and i0[0, 0] == 100 + 50 and i0[0, 1] == 5000 + 50
    ix.close()


def test_ivf_self_join_equals_range_search_with_exclusion():
    import torch
    n, d, nlist, nprobe = 6000, 64, 32, 4
    rng = np.random.default_rng(91)
    base = rng.standard_normal((n, d)).astype(np.float32)
    src, dst = rng.integers(0, n, size=700), rng.integers(0, n, size=700)
    base[dst] = base[src] + 0.15 * rng.standard_normal((700, d)).astype(np.float32)      # planted near-duplicates
    c16 = ds.normalize_round(base)
    c16[3000:3030] = c16[10]                                                              # 31 exact duplicates
    cen = ds.kmeans_spherical(c16, nlist, 4, seed=3)
    ix = _ivf(c16, cen)
    floor = 0.9
    own = np.arange(n, dtype=np.int64)
    ref = None
    for k in (16, 256):
        want = ix.range_search(c16, floor, k, nprobe, normalize=False, exclude=own)
        for batch in (n, 1700):
            sc, ids, cnt = ix.self_join(floor, nprobe, k=k, batch=batch)
            torch.cuda.synchronize()
            got = (sc.cpu().numpy(), ids.cpu().numpy(), cnt.cpu().numpy())
            assert sc.is_cuda and got[2].dtype == np.int64
            for a, b in zip(want, got):
                assert np.array_equal(a, b), f"k {k} batch {batch}: self_join differs from range_search(exclude=i)"
        if k == 16:
            ref = got
    sc, ids, cnt = ref
    assert not (ids == own[:, None]).any()                    # no row lists itself
    grp = [10] + list(range(3000, 3030))
    for r in grp:                                             # exact duplicates list each other, lowest rows first
        others = [x for x in grp if x != r][:16]
        assert ids[r].tolist() == others and cnt[r] >= 30
    # the contract against the oracle, with each row's own entry removed
    S, amb, _ = _probed_oracle(c16, c16, cen, ix.assignments(), nprobe)
    S[own, own] = -np.inf
    assert amb.sum() <= 0.01 * n
    _check_range(sc[~amb], ids[~amb], cnt[~amb], S[~amb], floor, 16)
    assert (cnt > 0).sum() > 500
    # id_base shifts the ids and nothing else
    ix.set_id_base(7000)
    assert ix.id_base == 7000
    s2, i2, c2 = ix.self_join(floor, nprobe, k=16)
    torch.cuda.synchronize()
    assert np.array_equal(s2.cpu().numpy(), sc) and np.array_equal(c2.cpu().numpy(), cnt)
    assert np.array_equal(i2.cpu().numpy(), np.where(ids >= 0, ids + 7000, -1))
    ix.close()


def test_ivf_range_bf16_device_tensors_side_stream_out_reuse():
    import torch
    n, nq, d, nlist, nprobe, k = 20000, 300, 96, 32, 8, 20
    rows, qs = ds.make_clustered(n, nq, d, 51, n_centroids=32)
    cb = torch.from_numpy(ds.l2_normalize(rows)).to(torch.bfloat16)
    qb = torch.from_numpy(ds.l2_normalize(qs)).to(torch.bfloat16)
    cen = torch.from_numpy(ds.kmeans_spherical(cb.float().numpy(), nlist, 4, seed=3, dtype=np.float32)).to(torch.bfloat16)
    from mrag_amd.index import IVFFlatIndex
    ix = IVFFlatIndex(d, nlist, dtype="bf16")
    ix.set_centroids(cen, normalize=False)
    ix.set_id_base(10_000)
    ix.add(cb, normalize=False)
    S, amb, _ = _probed_oracle(qb, cb, cen, ix.assignments(), nprobe)
    floor = _floor_for(S, k)
    side = torch.cuda.Stream()
    qd = qb.cuda()
    excl = torch.full((nq,), -1, dtype=torch.int64, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    out = (torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"),
           torch.empty(nq, dtype=torch.int64, device="cuda"))
    with torch.cuda.stream(side):
        sc, ids, cnt = ix.range_search(qd, floor, k, nprobe, normalize=False, stream=side, out=out)
    side.synchronize()
    assert sc.is_cuda and ids.is_cuda and cnt.is_cuda
    assert sc.data_ptr() == out[0].data_ptr() and ids.data_ptr() == out[1].data_ptr() and cnt.data_ptr() == out[2].data_ptr()
    first = [t.cpu().numpy().copy() for t in (sc, ids, cnt)]
    a, b, c = _keep(amb, *first)
    _check_range(a, b, c, S[~amb], floor, k, id_base=10_000)
    # the same buffers again, a device exclusion of nothing, the default stream: the same answer; and host queries
    sc, ids, cnt = ix.range_search(qd, floor, k, nprobe, normalize=False, exclude=excl, out=out)
    torch.cuda.synchronize()
    for x, y in zip(first, (sc, ids, cnt)):
        assert np.array_equal(x, y.cpu().numpy())
    hs, hi, hc = ix.range_search(qb, floor, k, nprobe, normalize=False)
    assert isinstance(hs, np.ndarray) and np.array_equal(hs, first[0]) and np.array_equal(hi, first[1]) and np.array_equal(hc, first[2])
    ix.close()


_CHILD = textwrap.dedent('''
    import sys, numpy as np
    sys.path.insert(0, ".")
    from oracle import dense_search as ds
    from mrag_amd.index import IVFFlatIndex
    from mrag_amd._native import MragError
    rows, qs = ds.make_clustered(30000, 3000, 128, 31, n_centroids=64)
    c16, q16 = ds.normalize_round(rows), ds.normalize_round(qs)
    cen = ds.kmeans_spherical(c16, 96, 3, seed=4)
    ix = IVFFlatIndex(128, 96); ix.set_centroids(cen, normalize=False); ix.add(c16, normalize=False)
    excl = np.arange(3000, dtype=np.int64) * 7 % 30000
    try:
        sc, ids, cnt = ix.range_search(q16, 0.93, 10, 8, normalize=False, exclude=excl)
        s0, i0 = ix.search(q16, 10, 8, normalize=False)
        np.savez(sys.argv[1], sc=sc, ids=ids, cnt=cnt, s0=s0, i0=i0, code=0)
    except MragError as e:
        np.savez(sys.argv[1], code=e.code, msg=str(e))
''')


def _run_child(td, name, env):
    path = os.path.join(td, name + ".npz")
    subprocess.run([sys.executable, "-c", _CHILD, path], check=True, env={**os.environ, **env}, cwd=ROOT, timeout=600)
    return np.load(path)


def test_ivf_range_chunked_batch_and_disabled_score_buffer():
    """A 48 MB score buffer cuts the 3 000 queries into several chunks: the same lists and counts, per query.  With the
    buffer disabled the search would take the fused regime, which has no range form: MRAG_ERR_UNSUPPORTED, no answer."""
    with tempfile.TemporaryDirectory() as td:
        whole = _run_child(td, "whole", {})
        cut = _run_child(td, "cut", {"MRAG_IVF_SCORES_MB": "48"})
        off = _run_child(td, "off", {"MRAG_IVF_SCORES_MB": "0"})
        assert int(whole["code"]) == 0 and int(cut["code"]) == 0
        for key in ("sc", "ids", "cnt"):
            assert np.array_equal(whole[key], cut[key]), key
        assert (whole["cnt"] > 10).any() and (whole["cnt"] <= 10).any()      # the floor cuts some lists and not others
        assert int(off["code"]) == -5 and "MRAG_ERR_UNSUPPORTED" in str(off["msg"]) and "MRAG_IVF_SCORES_MB" in str(off["msg"])


def test_ivf_range_refusals():
    from mrag_amd._native import MragError
    from mrag_amd.index import IVFFlatIndex
    d = 64
    c16 = ds.normalize_round(ds.make_gaussian(6000, d, 71))
    q = c16[:4]
    # exhaustive probing of 512 lists: more segments per query than the selection holds, and no fused range form
    ix = _ivf(c16, c16[:512].copy())
    with pytest.raises(MragError, match="MRAG_ERR_UNSUPPORTED") as ei:
        ix.range_search(q, 0.5, 10, 512, normalize=False)
    assert ei.value.code == -5
    with pytest.raises(MragError, match="MRAG_ERR_UNSUPPORTED"):
        ix.self_join(0.5, 512, k=10)
    with pytest.raises(MragError, match="MRAG_ERR_UNSUPPORTED"):      # 257 .. nlist - 1: as the plain search, not clamped to 256
        ix.range_search(q, 0.5, 10, 300, normalize=False)
    sc, ids, cnt = ix.range_search(q, 0.5, 10, 256, normalize=False)   # the largest supported probe count works
    assert (ids[:, 0] == np.arange(4)).all() and (cnt >= 1).all()
    with pytest.raises(MragError):                                    # a host exclusion outside the rows
        ix.range_search(q, 0.5, 10, 8, normalize=False, exclude=np.array([0, 1, 2, 6000]))
    ix.close()
    empty = IVFFlatIndex(d, 16)
    with pytest.raises(MragError):                                    # no centroids
        empty.range_search(q, 0.5, 10, 4, normalize=False)
    empty.close()


def test_semantic_edges_index_ivf_equals_dense_when_every_list_is_probed():
    from mrag_amd.index import DenseIndex
    from mrag_amd.pairwise import semantic_edges_index
    n, d, nlist, k = 5000, 64, 32, 128
    rng = np.random.default_rng(97)
    base = rng.standard_normal((n, d)).astype(np.float32)
    src, dst = rng.integers(0, n, size=600), rng.integers(0, n, size=600)
    base[dst] = base[src] + 0.15 * rng.standard_normal((600, d)).astype(np.float32)
    hub = rng.integers(0, n, size=90)
    base[hub] = base[hub[0]] + 0.05 * rng.standard_normal((90, d)).astype(np.float32)     # rows with ~90 neighbours (< k: none truncated)
    c16 = ds.normalize_round(base)
    cen = ds.kmeans_spherical(c16, nlist, 4, seed=3)
    ix = _ivf(c16, cen, id_base=77)
    dx = DenseIndex(d)
    dx.set_id_base(77)
    dx.add(c16, normalize=False)
    e_ivf, t_ivf = semantic_edges_index(ix, 0.9, k=k, batch=1700, nprobe=nlist)
    e_den, t_den = semantic_edges_index(dx, 0.9, k=k, batch=1700)
    assert len(t_ivf) == 0 and len(t_den) == 0
    S = _f64(c16) @ _f64(c16).T
    a = {(i, j): v for i, j, v in e_ivf if abs(S[i, j] - 0.9) > TOL}      # pairs within TOL of the threshold are left aside
    b = {(i, j): v for i, j, v in e_den if abs(S[i, j] - 0.9) > TOL}
    assert sorted(a) == sorted(b) and len(a) > 500
    assert all(abs(a[p] - b[p]) <= TOL and abs(a[p] - S[p]) <= TOL for p in a)
    assert [(i, j) for i, j, _ in e_ivf] == sorted((i, j) for i, j, _ in e_ivf) and all(i < j for i, j, _ in e_ivf)
    # fewer probes: a subset of those pairs, the same similarities
    e_few, _ = semantic_edges_index(ix, 0.9, k=k, batch=1700, nprobe=2)
    few = {(i, j): v for i, j, v in e_few}
    assert 0 < len(few) <= len(e_ivf) and set(few) <= {(i, j) for i, j, _ in e_ivf}
    assert all(abs(S[p] - v) <= TOL for p, v in few.items())
    ix.close()
    dx.close()
