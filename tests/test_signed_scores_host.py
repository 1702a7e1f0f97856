"""CPU side of the signed-score tests: the inputs of tests/signed_scores_cases.py have the properties they were built for,
at every shape tests/test_gpu_signed_scores.py hands to the GPU; the comparison used there catches each wrong selector
(mutant) on those inputs; the same mutants pass on the Gaussian data of the older tests (the gap these cases close); and
the comparison accepts the oracle against itself."""
import numpy as np
import pytest

import signed_scores_cases as sc
from oracle import dense_search as ds

DENSE_A = [(r[0], k) for r in sc.DENSE + [sc.WIDE] for k in r[5]]
DENSE_B = [(r[0], k, s) for r in sc.DENSE for k in r[5] for s in r[6]]
IVF_A = [(r[0], k, cl) for r in sc.IVF for k in r[7] for cl in (0, 1)]
ROWS = dict(sc.DENSE_BY_NAME, **{sc.WIDE[0]: sc.WIDE})


def _dense_a(name, k):
    _, nq, n, d, amp = ROWS[name][:5]
    return sc.family_a(n, nq, d, amp, k), nq, n, d, amp


def _ivf_a(name, k, cl):
    _, n, nq, d, amp, nlist, nprobe, _, _, q_cols = sc.IVF_BY_NAME[name]
    return sc.ivf_a(n, nq, d, amp, nlist, nprobe, k, cl, q_cols=q_cols), nq


def _survives_16_bits(x):
    x = np.asarray(x, dtype=np.float32)
    return bool((x.astype(np.float16).astype(np.float32) == x).all()) and bool(((x.view(np.uint32) & 0xFFFF) == 0).all())


def _kind_properties(rv, S, b, k, nq):
    """The five domains, per query, from the shifted oracle top-k rv [nq, k] over the candidate scores S."""
    kind = np.arange(nq) % 5
    m = np.maximum((rv > -np.inf).sum(1), 1)
    cut = np.minimum(k, m) - 1
    first, last = rv[:, 0], rv[np.arange(nq), cut]
    assert (b[kind == 0] == 0).all()
    assert (last[kind == 1] == 0).all()                                    # the k-th best is exactly 0.0
    assert ((first[kind == 2] >= 0) & (last[kind == 2] <= 0)).all()        # the sign changes inside the top-k
    assert (first[kind == 3] == -1).all()                                  # all negative, the best is -1
    assert (first[kind == 4] < -100).all()                                 # far negative
    # rows tied with the cut that the cut leaves out: for some query, and at exactly 0.0 for some zero-at-cut query
    beyond = (S == last[:, None]).sum(1) - (rv == last[:, None]).sum(1)
    return kind, beyond


# ------------------------------------------------------------------------------------------------ inputs, family A
@pytest.mark.parametrize("name,k", DENSE_A)
def test_family_a_dense_inputs(name, k):
    a, nq, n, d, amp = _dense_a(name, k)
    c, q, b, S = a["c"], a["q"], a["b"], sc.S_of(a)
    assert c.shape == (n, d) and q.shape == (nq, d) and (c[:, -1] == 1).all() and (q[:, -1] == -b).all()
    assert np.abs(c[:, :-1]).max() <= amp and np.abs(q[:, :-1]).max() <= amp
    assert _survives_16_bits(c) and _survives_16_bits(q)
    assert np.abs(b).max() <= 256 and np.abs(S).max() < 2 ** 24 and (S == np.round(S)).all()
    # the shift moves no row: ids of the unshifted problem, scores rv - b exactly
    rv0, ri0 = ds.brute_force_topk(a["q0"], c, k)
    assert np.array_equal(a["ri"], ri0) and np.array_equal(a["rv"], rv0 - b[:, None])
    assert np.array_equal(S, sc.scores64(a["q0"], c) - b[:, None])
    kind, beyond = _kind_properties(a["rv"], S, b, k, nq)
    assert (beyond > 0).any()
    assert (beyond[kind == 1] > 0).any(), "no zero-at-cut query with more rows at 0.0 behind the cut"
    assert len(set(kind.tolist())) == min(nq, 5)
    assert sc.accept_exact(a["rv"].astype(np.float32), a["ri"], a["rv"], a["ri"])          # (c)


@pytest.mark.parametrize("name,k", sc.FILTERED)
def test_family_a_filtered_inputs(name, k):
    _, nq, n, d, amp = ROWS[name][:5]
    assert k in ROWS[name][5]
    masks = sc.allow_masks(n, k)
    assert 0.4 * n < masks["half"].sum() < 0.6 * n and 0 < masks["1pct"].sum() < 0.03 * n and 0 < masks["few"].sum() < k
    for mname, mask in masks.items():
        a = sc.family_a_masked(n, nq, d, amp, k, mname)
        assert _survives_16_bits(a["q"]) and np.abs(a["b"]).max() <= 256 and np.array_equal(a["mask"], mask)
        assert ((a["ri"] >= 0).sum(1) == min(k, int(mask.sum()))).all()
        assert mask[a["ri"][a["ri"] >= 0]].all()
        _kind_properties(a["rv"], sc.S_of(a), a["b"], k, nq)


@pytest.mark.parametrize("k", sc.WIDE[5])
def test_family_a_sorted_wide_batch_inputs(k):
    """the rows stored by descending score of query 0: its whole top-k is rows 0 .. k - 1, inside the first of the S >= 13
    corpus splits of the wide batch (66 tiles), and the domains are those of the unsorted problem"""
    _, nq, n, d, amp, _ = sc.WIDE
    w, a = sc.wide_sorted(k), sc.family_a(n, nq, d, amp, k)
    assert (w["ri"][0] == np.arange(k)).all() and k <= 256
    assert np.array_equal(np.sort(w["c"], axis=0), np.sort(a["c"], axis=0)) and np.array_equal(w["rv"], a["rv"])
    _kind_properties(w["rv"], sc.S_of(w), w["b"], k, nq)


@pytest.mark.parametrize("frac", sc.IVF_FILTER_FRACS)
def test_family_a_ivf_filtered_inputs(frac):
    from test_ivf_filtered_host import ivf_filtered_ref
    _, n, nq, d, amp, nlist, nprobe = sc.IVF_BY_NAME["register"][:7]
    k = sc.IVF_FILTER_K
    f = sc.ivf_a_filtered(frac)
    mask, ivf = f["mask"], f["ivf"]
    assert f["n_clear"] == nq, "too few queries with a clear cut between probed and unprobed live lists"
    assert 0.8 * frac * n < mask.sum() < 1.2 * frac * n
    for path in ("probe", "exact"):
        q, rv, ri = f[path]
        assert q.shape == (nq, d) and _survives_16_bits(q) and np.abs(q[:, -1]).max() <= 256
        v2, i2, margin = ivf_filtered_ref(q, ivf["c"], ivf["cen"], ivf["assign"], mask, nprobe, k, path=path)
        assert np.array_equal(v2, rv) and np.array_equal(i2, ri)             # the restatement tests/test_gpu_ivf_filtered.py uses
        assert (margin > 0).all()
        assert mask[ri[ri >= 0]].all() and ((ri >= 0).sum(1) >= 1).all()
        S = sc.scores64(q, ivf["c"])
        S[:, ~mask] = -np.inf
        if path == "probe":
            live = np.flatnonzero(np.bincount(ivf["assign"][mask], minlength=nlist) > 0)
            cs = sc.scores64(q, ivf["cen"])
            for g in range(nq):
                pick = live[np.lexsort((live, -cs[g, live]))][:nprobe]
                S[g, ~np.isin(ivf["assign"], pick)] = -np.inf
        _kind_properties(rv, S, -q[:, -1].astype(np.float64), k, nq)


def test_family_a_sets_inputs():
    p = sc.SETS
    sets, set_of, a = sc.sets_case()
    assert [len(s) for s in sets] == list(p["sizes"]) and len(set_of) == p["nq"] and set(set_of.tolist()) == {0, 1, 2}
    assert _survives_16_bits(a["q"]) and np.abs(a["b"]).max() <= 256
    assert ((a["ri"] >= 0).sum(1) == np.minimum(p["k"], np.asarray(p["sizes"])[set_of])).all()
    _kind_properties(a["rv"], a["S"], a["b"], p["k"], p["nq"])


@pytest.mark.parametrize("name,k,cl", IVF_A)
def test_family_a_ivf_inputs(name, k, cl):
    a, nq = _ivf_a(name, k, cl)
    _, n, _, d, amp, nlist, nprobe, _, _, _ = sc.IVF_BY_NAME[name]
    c, cen, q, b, S = a["c"], a["cen"], a["q"], a["b"], a["S"]
    assert a["n_clear"] == nq == q.shape[0], "too few queries with a clear probe cut"
    assert cen.shape == (nlist, d) and (cen[:, -1] == cl).all() and len(np.unique(cen, axis=0)) == nlist
    assert _survives_16_bits(c) and _survives_16_bits(q) and _survives_16_bits(cen) and np.abs(b).max() <= 256
    # the probe scores: unshifted with last centroid column 0, shifted by -b_q with 1; the probed lists are the same
    cs = sc.scores64(q, cen)
    q0 = np.array(q); q0[:, -1] = 0
    assert np.array_equal(cs, sc.scores64(q0, cen) - cl * b[:, None])
    assert np.array_equal(sc.probes_of(q, cen, nprobe), a["probes"])
    if nprobe < nlist:
        srt = -np.sort(-cs, axis=1)
        assert (srt[:, nprobe - 1] != srt[:, nprobe]).all()
        if cl:
            assert (srt[:, :nprobe] < 0).all(axis=1).any() and (srt[:, nprobe - 1] <= 0).any()   # probes picked among negatives
    # the oracle is ds.ivf_search on the same assignment
    rv, ri = ds.ivf_search(q, c, cen, a["assign"], nprobe, k)
    assert np.array_equal(ri, a["ri"]) and np.array_equal(rv, a["rv"])
    kind, beyond = _kind_properties(a["rv"], S, b, k, nq)
    cands = (S > -np.inf).sum(1)
    ties = (S == a["rv"][np.arange(nq), np.minimum(k, np.maximum(cands, 1)) - 1][:, None]).sum(1)
    if name == "register":
        assert (cands > k).all() and (cands <= 8192).all() and (ties <= 512).all()
    elif name == "streamed":
        assert (cands > 8192).all() and (ties <= 512).all()
    elif name == "serial-ties":
        assert all((ties[kind == j] > 512).any() for j in range(5)), ties
    else:
        assert (cands <= k).all()
    assert sc.accept_exact(a["rv"].astype(np.float32), a["ri"], a["rv"], a["ri"])          # (c)


# ------------------------------------------------------------------------------------------------ inputs, family B
@pytest.mark.parametrize("name,k,spread", DENSE_B)
def test_family_b_dense_inputs(name, k, spread):
    _, nq, n, d = ROWS[name][:4]
    b = sc.family_b(n, nq, d, spread, k)
    rv, S = b["rv"], sc.S_of(b)
    assert np.abs(S).max() <= 1.0 + 1e-3                      # the 1e-5 bar is the project's for |score| <= 1
    if spread == 0.1:
        assert (S < 0).all()                                  # all top-k < 0: in fact every score of every query
    else:
        assert rv[:, 0].max() > 0 > rv[:, -1].min()           # positive and negative entries decide in one batch
        if k >= 10:                                           # first > 0 > last within one list, for a quarter of the queries
            assert ((rv[:, 0] > 0) & (rv[:, -1] < 0)).mean() >= 0.25      # (measured: 0.33 ... 1.0 over the shapes)
    assert sc.accept_tol(rv.astype(np.float32), b["ri"], rv, b["ri"])                      # (c)


@pytest.mark.parametrize("spread", sc.SPREADS_B)
def test_family_b_ivf_inputs(spread):
    """enough queries with a clear probe cut, and (with the oracle's own assignment standing in for the index's) the
    claimed signs among the rows of the probed lists"""
    _, n, nq, d, _, nlist, nprobe, ks = sc.IVF_BY_NAME["register"][:8]
    b = sc.ivf_b(n, nq, d, nlist, nprobe, spread)
    assert b["n_clear"] == nq == b["q"].shape[0]
    rv, _ = ds.ivf_search(b["q"], b["c"], b["cen"], ds.ivf_assign(b["c"], b["cen"]), nprobe, max(ks))
    assert (rv < 0).all() if spread == 0.1 else (rv[:, 0].max() > 0 > rv[:, -1].min())


@pytest.mark.parametrize("nq,d", sc.FP8)
def test_family_b_fp8_inputs(nq, d):
    for spread in sc.SPREADS_B:
        rv = sc.family_b(sc.FP8_N, nq, d, spread, sc.FP8_K)["rv"]
        assert (rv < 0).all() if spread == 0.1 else (rv[:, 0].max() > 0 > rv[:, -1].min())


# ------------------------------------------------------------------------------------------------ mutants
def _range_all(fn, S, k):
    return [fn(S, f, k) for f in sc.FLOORS_A]


MUTANT_QUERIES = 60      # the selectors work per query: the first 60 (twelve of each kind) stand for a batch of 1 025


def _range_caught(fn, S, k):
    """the range answers over FLOORS_A, as the GPU test compares them: counts and lists exact per floor, and the two zero
    floors alike"""
    got, ref = _range_all(fn, S, k), _range_all(sc.range_of, S, k)
    same_zero = all(np.array_equal(x, y) for x, y in zip(got[0], got[1]))
    return not (all(sc.accept_range_exact(g, r) for g, r in zip(got, ref)) and same_zero)


@pytest.mark.parametrize("name,k", DENSE_A)
def test_mutants_change_family_a_dense(name, k):
    """(a): every mutant changes an answer the exact comparison would accept."""
    a = _dense_a(name, k)[0]
    S, rv, ri = sc.scores64(a["q"][:MUTANT_QUERIES], a["c"]), a["rv"][:MUTANT_QUERIES], a["ri"][:MUTANT_QUERIES]
    for mname, fn in sc.TOPK_MUTANTS.items():
        assert not sc.accept_exact(*fn(S, k), rv, ri), mname
    for mname, fn in sc.RANGE_MUTANTS.items():
        assert _range_caught(fn, S, min(k, 64)), mname
    assert not _range_caught(sc.range_of, S, min(k, 64))                                    # (c)


@pytest.mark.parametrize("name,k,cl", IVF_A)
def test_mutants_change_family_a_ivf(name, k, cl):
    a, nq = _ivf_a(name, k, cl)
    for mname, fn in sc.TOPK_MUTANTS.items():
        if mname == "ties-high-row" and name == "serial-small":
            continue                                          # at most k candidates: nothing is cut, no tie to take wrongly
        assert not sc.accept_exact(*fn(a["S"], k), a["rv"], a["ri"]), mname
    for mname, fn in sc.RANGE_MUTANTS.items():
        assert _range_caught(fn, a["S"], k), mname


@pytest.mark.parametrize("name,k,spread", DENSE_B)
def test_mutants_change_family_b(name, k, spread):
    _, nq, n, d = ROWS[name][:4]
    b = sc.family_b(n, nq, d, spread, k)
    S, rv, ri = sc.scores64(b["q"][:MUTANT_QUERIES], b["c"]), b["rv"][:MUTANT_QUERIES], b["ri"][:MUTANT_QUERIES]
    for mname in ("magnitude", "threshold-zero", "zero-padding"):
        assert not sc.accept_tol(*sc.TOPK_MUTANTS[mname](S, k), rv, ri), mname


GAUSSIAN = [(7, 255, 40, 4), (64, 257, 96, 10), (300, 20000, 768, 10), (33, 4097, 384, 16), (20, 3000, 128, 17),
            (10, 2500, 256, 64)]      # tests/test_gpu_bruteforce.py::test_shapes_f16, n >= 255


@pytest.mark.parametrize("nq,n,d,k", GAUSSIAN)
def test_mutants_pass_on_gaussian_data(nq, n, d, k):
    """(b): on normalised Gaussian rows mutants 1-5 give the oracle's answer -- the older tests cannot see them."""
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 1234))
    q16 = ds.normalize_round(ds.make_gaussian(nq, d, 5678))
    rv, ri = ds.brute_force_topk(q16, c16, k)
    S = sc.scores64(q16, c16)
    assert (rv > 0).all()
    for mname in ("magnitude", "threshold-zero", "zero-padding"):
        v, i = sc.TOPK_MUTANTS[mname](S, k)
        assert sc.accept_tol(v, i, rv, ri) and np.array_equal(i, ri), mname
    for mname, fn in sc.RANGE_MUTANTS.items():
        for floor in (0.0, -0.0, 0.1):
            assert sc.accept_range_exact(fn(S, floor, k), sc.range_of(S, floor, k)), (mname, floor)


def test_acceptance_rejects_the_smallest_errors():
    """(c), the other way round: one wrong id, one score off by one, a count off by one are not accepted."""
    a = _dense_a("k2-certificate", 10)[0]
    rv, ri = a["rv"], a["ri"]
    assert sc.accept_exact(rv, ri, rv, ri)
    i2 = ri.copy(); i2[3, 9] += 1
    v2 = rv.copy(); v2[5, 0] += 1
    assert not sc.accept_exact(rv, i2, rv, ri) and not sc.accept_exact(v2, ri, rv, ri)
    assert sc.accept_exact(np.where(rv == 0, -0.0, rv), ri, rv, ri)                        # 0.0 == -0.0
    r = sc.range_of(sc.S_of(a), 0.0, 10)
    for floor in sc.FLOORS_A:
        for x, y in zip(sc.range_from_topk(sc.S_of(a), rv, ri, floor), sc.range_of(sc.S_of(a), floor, 10)):
            assert np.array_equal(x, y)
    assert sc.accept_range_exact(r, r) and not sc.accept_range_exact((r[0], r[1], r[2] + 1), r)
    b = sc.family_b(2053, 40, 64, 0.2, 10)
    v3 = b["rv"].copy(); v3[0, 0] += 3e-5
    assert sc.accept_tol(b["rv"], b["ri"], b["rv"], b["ri"]) and not sc.accept_tol(v3, b["ri"], b["rv"], b["ri"])
