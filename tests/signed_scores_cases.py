"""Inputs, oracles and wrong selectors for the signed-score tests of the dense and IVF searches
(tests/test_signed_scores_host.py, tests/test_gpu_signed_scores.py).  numpy only.

Every selection kernel of the vector side orders fp32 scores through an orderable key (``f32_ord`` / ``make_key`` in
csrc/bf_kernels.h, ``s_f32_ord`` in csrc/ivf_scan.hip) and several use sentinels (-inf for masked rows, key 0 for "no
entry", zero rows as padding).  Normalised Gaussian rows keep every deciding score positive, so the negative half of the
key space, an exact 0.0 at the cut and the sentinels' neighbourhood never decide there.  Two families put them in play:

A. exact, shifted integers.  Rows and queries are small integers over d - 1 columns, the last column of every row is 1
   and the last column of query q is -b_q, so score = unshifted score - b_q: the order per query is unchanged, every
   value is an exact integer in fp16, bf16 and fp32, and the comparison is ``==``.  b_q cycles through KINDS, computed from
   the query's own unshifted top-k, so neighbouring query columns of one tile sit in different score domains.
B. rounded cosine rows around +u, queries around -u: all scores negative (spread 0.1) or a top-k that crosses zero
   (spread 0.2; 0.17 over 40 000 rows), compared with the project's 1e-5 tolerance for |score| <= 1.

The mutants are the mistakes these inputs are there to catch, written over the oracle's fp64 score matrix."""
from __future__ import annotations

import functools
from typing import Optional, Tuple

import numpy as np

from oracle import dense_search as ds

TOL = 1e-5                     # the project's bar for |score| <= 1 with fp32 accumulation (tests/test_gpu_bruteforce.py)
KINDS = ("control", "zero-at-cut", "sign-inside", "all-negative", "far-negative")
FAR = 255.0                    # kind 5's shift: exact in bf16 (8 significant bits), |score| stays far below 2^24
FLOORS_A = (0.0, -0.0, -3.0, 2.0, -1000.0)
FLOOR_B = -0.01
SPREADS_B = (0.1, 0.2)
SEED_A = 5                     # a seed at which every shape has a zero-at-cut query with more rows at 0.0 behind the cut (the host test asserts it)


# ------------------------------------------------------------------------------------------------ family A
def shifts(rv: np.ndarray, k: int) -> np.ndarray:
    """b_q for each query from its unshifted top-k scores ``rv`` [nq, k] ((-inf) past the candidates): query q is of kind
    ``q % 5``.  With m valid entries the cut is entry min(k, m) - 1."""
    nq = rv.shape[0]
    m = np.maximum((rv > -np.inf).sum(1), 1)
    last = rv[np.arange(nq), np.minimum(k, m) - 1]
    mid = rv[np.arange(nq), np.minimum(k // 2, m - 1)]
    b = np.zeros(nq)
    kind = np.arange(nq) % 5
    b[kind == 1] = last[kind == 1]
    b[kind == 2] = mid[kind == 2]
    b[kind == 3] = rv[kind == 3, 0] + 1.0
    b[kind == 4] = FAR
    return b


@functools.lru_cache(maxsize=None)
def int_base(n: int, nq: int, d: int, amp: int, seed: int, q_cols: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Integer rows [n, d] (last column 1) and queries [nq, d] (last column 0: unshifted), fp32, values in [-amp, amp];
    with ``q_cols`` the queries are zero behind their first q_cols columns (few distinct scores: many rows tie)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-amp, amp + 1, size=(n, d)).astype(np.float32)
    q = rng.integers(-amp, amp + 1, size=(nq, d)).astype(np.float32)
    if q_cols is not None:
        q[:, q_cols:] = 0.0
    c[:, -1] = 1.0
    q[:, -1] = 0.0
    c.setflags(write=False)
    q.setflags(write=False)
    return c, q


def scores64(q, c) -> np.ndarray:
    return np.asarray(q, dtype=np.float64) @ np.asarray(c, dtype=np.float64).T


def topk_of(S: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """top-k per row of S by (score desc, column asc); -inf entries are no candidates: (-inf, -1), padded to k columns."""
    v, i = ds.topk_desc_rowasc(S, k)
    i = np.where(v > -np.inf, i, -1)
    if v.shape[1] < k:
        pad = k - v.shape[1]
        v = np.concatenate([v, np.full((S.shape[0], pad), -np.inf)], 1)
        i = np.concatenate([i, np.full((S.shape[0], pad), -1, dtype=np.int64)], 1)
    return v, i


def shift_queries(q0: np.ndarray, S0: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (queries with last column -b_q, b): b from the top-k of the unshifted candidate scores S0 (-inf = no candidate)."""
    rv, _ = topk_of(S0, k)
    b = shifts(rv, k)
    q = np.array(q0, dtype=np.float32)
    q[:, -1] = -b
    return q, b


@functools.lru_cache(maxsize=None)
def family_a(n: int, nq: int, d: int, amp: int, k: int, seed: int = SEED_A):
    """-> dict(c, q, q0, b, rv, ri): the dense family-A problem of one shape and k; (rv, ri) = ds.brute_force_topk of the
    shifted arrays.  The fp64 score matrix is not kept (1 025 x 40 000 doubles per k): ``S_of`` computes it on demand."""
    c, q0 = int_base(n, nq, d, amp, seed)
    q, b = shift_queries(q0, scores64(q0, c), k)
    rv, ri = ds.brute_force_topk(q, c, k)
    return {"c": c, "q": q, "q0": q0, "b": b, "rv": rv, "ri": ri}


def S_of(a) -> np.ndarray:
    """the fp64 scores of a dense problem's (shifted) arrays, -inf on the rows its allow-set leaves out"""
    S = scores64(a["q"], a["c"])
    if "mask" in a:
        S[:, ~a["mask"]] = -np.inf
    return S


@functools.lru_cache(maxsize=None)
def family_a_masked(n: int, nq: int, d: int, amp: int, k: int, mname: str, seed: int = SEED_A):
    """family A for a filtered search under ``allow_masks(n, k)[mname]``: b from the unshifted top-k over the allowed rows,
    so the kinds describe the filtered problem.  -> dict(c, q, b, mask, rv, ri); the scores through ``S_of``."""
    mask = allow_masks(n, k)[mname]
    c, q0 = int_base(n, nq, d, amp, seed)
    S0 = scores64(q0, c)
    S0[:, ~mask] = -np.inf
    q, b = shift_queries(q0, S0, k)
    del S0
    a = {"c": c, "q": q, "b": b, "mask": mask}
    a["rv"], a["ri"] = topk_of(S_of(a), k)
    return a


def allow_masks(n: int, k: int, seed: int = 99):
    """The three allow-sets of a filtered case: about half the rows, about 1 %, fewer than k (the (-inf, -1) tail)."""
    rng = np.random.default_rng(seed + n)
    few = np.zeros(n, dtype=bool)
    few[rng.choice(n, size=max(1, k - 1) if k > 1 else 0, replace=False)] = True
    return {"half": rng.random(n) < 0.5, "1pct": rng.random(n) < 0.01, "few": few}


@functools.lru_cache(maxsize=None)
def sets_case():
    """search_sets over family A: -> (sets: row positions per set, set_of [nq], dict(c, q, b, S (rows outside the question's
    set -inf), rv, ri)); b from the unshifted top-k inside each question's own set."""
    p = SETS
    c, q0 = int_base(p["n"], p["nq"], p["d"], p["amp"], SEED_A)
    rng = np.random.default_rng(17)
    sets = [np.sort(rng.choice(p["n"], size=m, replace=False)) for m in p["sizes"]]
    set_of = (np.arange(p["nq"]) % len(sets)).astype(np.int32)
    member = np.zeros((p["nq"], p["n"]), dtype=bool)
    for g, s in enumerate(set_of):
        member[g, sets[s]] = True
    q, b = shift_queries(q0, np.where(member, scores64(q0, c), -np.inf), p["k"])
    S = np.where(member, scores64(q, c), -np.inf)
    rv, ri = topk_of(S, p["k"])
    return sets, set_of, {"c": c, "q": q, "b": b, "S": S, "rv": rv, "ri": ri}


# ------------------------------------------------------------------------------------------------ family B
@functools.lru_cache(maxsize=None)
def family_b(n: int, nq: int, d: int, spread: float, k: int, seed: int = 5):
    """-> dict(c, q, rv, ri; the scores through ``S_of``): fp16 rows around +u, fp16 queries around -u, the oracle on those bits.  ``spread`` is the
    noise per coordinate at d = 64; at another d it is scaled by (64 / d)^(1/4).  A score is about (-1 + s^2 g.g') /
    (1 + s^2 d) with g, g' standard normal vectors, so whether the best scores reach zero is decided by s^2 sqrt(d), the
    spread of the cross term against the -1 of u.-u; the scaling keeps that product: all negative at 0.1, crossing zero
    at 0.2, at every d (the host test asserts both at every shape used)."""
    u = ds.l2_normalize(ds.make_gaussian(1, d, seed))[0]
    spread = spread * float((64.0 / d) ** 0.25)
    c = ds.normalize_round(u[None, :] + np.float32(spread) * ds.make_gaussian(n, d, seed + 1))
    q = ds.normalize_round(-u[None, :] + np.float32(spread) * ds.make_gaussian(nq, d, seed + 2))
    rv, ri = ds.brute_force_topk(q, c, k)
    return {"c": c, "q": q, "rv": rv, "ri": ri}


# ------------------------------------------------------------------------------------------------ IVF, family A
def probes_of(q, cen, nprobe: int) -> np.ndarray:
    """[nq, nprobe] probed lists by (centroid score desc, list id asc)."""
    return ds.topk_desc_rowasc(scores64(q, cen), min(nprobe, cen.shape[0]))[1]


def probed_mask(probes: np.ndarray, assign: np.ndarray) -> np.ndarray:
    """[nq, n] bool: row r is in one of query q's probed lists."""
    nlist = int(max(assign.max(initial=0), probes.max(initial=0))) + 1
    hit = np.zeros((probes.shape[0], nlist), dtype=bool)
    np.put_along_axis(hit, probes, True, axis=1)
    return hit[:, assign]


def clear_probe_queries(q0: np.ndarray, cen: np.ndarray, nprobe: int, need: int, margin: float = 0.0) -> np.ndarray:
    """Indices of the first ``need`` queries whose nprobe-th and (nprobe+1)-th centroid scores differ by more than
    ``margin`` (all of them when every list is probed); fewer when there are not enough."""
    if nprobe >= cen.shape[0]:
        return np.arange(min(need, q0.shape[0]))
    cs = -np.sort(-scores64(q0, cen), axis=1)
    return np.flatnonzero(cs[:, nprobe - 1] - cs[:, nprobe] > margin)[:need]


@functools.lru_cache(maxsize=None)
def ivf_a(n: int, nq: int, d: int, amp: int, nlist: int, nprobe: int, k: int, cen_last: int, seed: int = 11,
          q_cols: Optional[int] = None):
    """The IVF family-A problem: centroids = ``nlist`` distinct integer rows of the corpus with last column ``cen_last`` (0:
    probe scores unshifted; 1: they shift by -b_q too), assignment = argmax of the exact integer scores (lowest list on
    ties), queries = the first nq of 3 nq spare ones with a clear probe cut, b from the unshifted top-k of the probed rows.
    -> dict(c, cen, q, b, assign, probes, S (rows outside the probed lists -inf), rv, ri, n_clear)."""
    c, q0 = int_base(n, 3 * nq, d, amp, seed, q_cols)
    rng = np.random.default_rng(seed + 1)
    uniq = np.unique(c, axis=0, return_index=True)[1]
    cen = np.array(c[np.sort(rng.choice(uniq, size=nlist, replace=False))])
    cen[:, -1] = float(cen_last)
    assign = ds.ivf_assign(c, cen)
    keep = clear_probe_queries(q0, cen, nprobe, nq)
    q0 = q0[keep]
    probes = probes_of(q0, cen, nprobe)           # the shift is one constant per query: the probed lists do not move
    inside = probed_mask(probes, assign)
    S0 = np.where(inside, scores64(q0, c), -np.inf)
    q, b = shift_queries(q0, S0, k)
    S = np.where(inside, scores64(q, c), -np.inf)
    rv, ri = topk_of(S, k)
    return {"c": c, "cen": cen, "q": q, "b": b, "assign": assign, "probes": probes, "S": S, "rv": rv, "ri": ri,
            "n_clear": int(keep.shape[0])}


@functools.lru_cache(maxsize=None)
def ivf_b(n: int, nq: int, d: int, nlist: int, nprobe: int, spread: float, seed: int = 5):
    """The IVF family-B problem: family-B rows, spherical k-means centroids over them, the first nq of 3 nq spare queries
    whose probe cut is clear by more than 1e-4 (ten times the fp32 bar).  The assignment is the index's own, so the oracle
    is computed beside the GPU.  -> dict(c, cen, q, n_clear)."""
    b = family_b(n, 3 * nq, d, spread, 1, seed)
    cen = ds.kmeans_spherical(b["c"], nlist, 3, seed=seed + 3)
    keep = clear_probe_queries(b["q"], cen, nprobe, nq, margin=1e-4)
    return {"c": b["c"], "cen": cen, "q": b["q"][keep], "n_clear": int(keep.shape[0])}


def ivf_filtered_ref(q, c, cen, assign, mask, nprobe: int, k: int, path: str = "probe"):
    """The filtered IVF search in fp64: a list is live when it holds an allowed row; path "probe": every query probes its
    nprobe best live lists by (centroid score desc, list id asc) and returns the top-k of the allowed rows there; path
    "exact": the top-k over all allowed rows.  -> (scores, ids, margin [nq]: the gap between the last probed and the first
    unprobed live list's centroid score, inf when every live list is probed)."""
    assign = np.asarray(assign, dtype=np.int64)
    nlist, nq = cen.shape[0], q.shape[0]
    live = np.flatnonzero(np.bincount(assign[mask], minlength=nlist) > 0)
    cs = scores64(q, cen)
    S = scores64(q, c)
    S[:, ~mask] = -np.inf
    margin = np.full(nq, np.inf)
    if path == "probe" and nprobe < nlist:
        for i in range(nq):
            order = live[np.lexsort((live, -cs[i, live]))]
            if live.size > nprobe:
                margin[i] = cs[i, order[nprobe - 1]] - cs[i, order[nprobe]]
            S[i, ~np.isin(assign, order[:nprobe])] = -np.inf
    v, ids = topk_of(S, k)
    return v, ids, margin


IVF_FILTER_FRACS = (0.5, 0.01)
IVF_FILTER_K = 10


@functools.lru_cache(maxsize=None)
def ivf_a_filtered(frac: float):
    """family A under an allow-set of about ``frac`` of the rows, on the register row with shifted probe scores: the first
    nq of the spare queries with a clear cut between the probed and the unprobed live lists, b from the filtered unshifted
    top-k of each path.  -> dict(mask, n_clear, ivf (the unfiltered problem: c, cen, assign), probe: (q, rv, ri),
    exact: (q, rv, ri))."""
    _, n, nq, d, amp, nlist, nprobe = IVF_BY_NAME["register"][:7]
    k = IVF_FILTER_K
    a = ivf_a(n, nq, d, amp, nlist, nprobe, k, 1)
    mask = np.random.default_rng(41).random(n) < frac
    q0 = np.array(int_base(n, 3 * nq, d, amp, 11)[1])
    _, _, margin = ivf_filtered_ref(q0, a["c"], a["cen"], a["assign"], mask, nprobe, k)
    q0 = q0[margin > 0][:nq]
    out = {"mask": mask, "n_clear": int(q0.shape[0]), "ivf": a}
    for path in ("probe", "exact"):
        rv0, _, _ = ivf_filtered_ref(q0, a["c"], a["cen"], a["assign"], mask, nprobe, k, path=path)
        q = np.array(q0)
        q[:, -1] = -shifts(rv0, k)
        rv, ri, _ = ivf_filtered_ref(q, a["c"], a["cen"], a["assign"], mask, nprobe, k, path=path)
        out[path] = (q, rv, ri)
    return out


@functools.lru_cache(maxsize=None)
def wide_sorted(k: int):
    """The wide-batch problem with the rows stored by descending score of query 0 (stable), so that its whole top-k sits in
    the first corpus split.  -> dict(c, q, rv, ri) on the reordered rows; the queries, and so every b_q, are unchanged."""
    _, nq, n, d, amp, _ = WIDE
    a = family_a(n, nq, d, amp, k)
    c2 = np.array(a["c"][np.argsort(-scores64(a["q"][:1], a["c"])[0], kind="stable")])
    rv, ri = ds.brute_force_topk(a["q"], c2, k)
    return {"c": c2, "q": a["q"], "b": a["b"], "rv": rv, "ri": ri}


# ------------------------------------------------------------------------------------------------ range oracle
def range_of(S: np.ndarray, floor: float, k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(scores, ids, counts): counts = rows with score >= floor (value comparison: -0.0 == 0.0), listed = the top min(k,
    count) of them."""
    ok = S >= floor
    v, i = topk_of(np.where(ok, S, -np.inf), k)
    return v, i, ok.sum(1).astype(np.int64)


def range_from_topk(S: np.ndarray, rv: np.ndarray, ri: np.ndarray, floor: float):
    """``range_of`` from the problem's own top-k (rv, ri) at the same k: the listed rows are the entries of the top-k that
    reach the floor, so only the counts need the whole matrix."""
    ok = rv >= floor
    return np.where(ok, rv, -np.inf), np.where(ok, ri, -1), (S >= floor).sum(1).astype(np.int64)


# ------------------------------------------------------------------------------------------------ acceptance
def accept_exact(got_v, got_i, ref_v, ref_i) -> bool:
    """family A: ids and scores equal as values (0.0 == -0.0, -inf == -inf)."""
    got_v, got_i = np.asarray(got_v), np.asarray(got_i)
    return got_i.shape == ref_i.shape and bool(np.array_equal(got_i, ref_i)) and bool((got_v == ref_v).all())


def accept_range_exact(got, ref) -> bool:
    return bool(np.array_equal(np.asarray(got[2]), ref[2])) and accept_exact(got[0], got[1], ref[0], ref[1])


def accept_tol(got_v, got_i, ref_v, ref_i, tol: float = TOL) -> bool:
    """family B: what tests/test_gpu_bruteforce.py::_check accepts -- scores within tol, descending, ids by the gap-aware
    rule with no mismatch, empty slots exactly (-inf, -1)."""
    got_v, got_i = np.asarray(got_v, dtype=np.float64), np.asarray(got_i)
    valid = ref_i >= 0
    if got_i.shape != ref_i.shape or not ((got_i >= 0) == valid).all() or not np.isneginf(got_v[~valid]).all():
        return False
    if not np.allclose(got_v[valid], ref_v[valid], rtol=0, atol=tol):
        return False
    with np.errstate(invalid="ignore"):
        if not (np.diff(got_v, axis=1)[valid[:, 1:]] <= 0).all():
            return False
    return ds.gap_aware_id_match(got_i, got_v, ref_i, ref_v, tol=tol)[1] == 0


# ------------------------------------------------------------------------------------------------ mutants
def _f32_bits(S):
    return np.asarray(S, dtype=np.float32).view(np.uint32).astype(np.int64)


def _select(key: np.ndarray, S: np.ndarray, k: int, row_desc: bool = False):
    """top-k per row of ``key`` (larger = better; key < 0 = no candidate), ties by row asc (or desc) -> (S values, ids)."""
    nq, n = key.shape
    v = np.full((nq, k), -np.inf)
    ids = np.full((nq, k), -1, dtype=np.int64)
    kth = np.partition(key, n - k, axis=1)[:, n - k] if n > k else np.full(nq, -1)
    for i in range(nq):
        cand = np.flatnonzero((key[i] >= kth[i]) & (key[i] >= 0))
        order = cand[np.lexsort((-cand if row_desc else cand, -key[i, cand]))[:k]]
        v[i, :order.size] = S[i, order]
        ids[i, :order.size] = order
    return v, ids


def mutant_magnitude(S, k):
    """1. negatives ranked by magnitude: key = bits ^ 0x80000000 for every score."""
    key = np.where(S > -np.inf, _f32_bits(S) ^ 0x80000000, -1)
    return _select(key, S, k)


def mutant_threshold_zero(S, k):
    """2. a threshold that starts at 0: candidates with score <= 0 never enter."""
    return topk_of(np.where(S > 0, S, -np.inf), k)


def mutant_zero_padding(S, k):
    """3. the corpus padded to a multiple of 256 with rows that score 0.0 and compete: their ids are >= n."""
    n = S.shape[1]
    pad = (-n) % 256
    return topk_of(np.concatenate([S, np.zeros((S.shape[0], pad))], axis=1), k)


def mutant_range_strict(S, floor, k):
    """4. the range search with > for >=."""
    ok = S > floor
    v, i = topk_of(np.where(ok, S, -np.inf), k)
    return v, i, ok.sum(1).astype(np.int64)


def mutant_range_bits(S, floor, k):
    """5. the floor compared on raw bits where it is met: a row counts when its score is above the floor or has the floor's
    very bits, so floors -0.0 and +0.0 differ on the rows that score 0.0."""
    f = np.float32(floor)
    ok = (S > floor) | (_f32_bits(S) == int(f.view(np.uint32)))
    v, i = topk_of(np.where(ok, S, -np.inf), k)
    return v, i, ok.sum(1).astype(np.int64)


def mutant_ties_high_row(S, k):
    """6. the rows tied on the k-th score are taken highest row first (the list itself stays (score desc, row asc))."""
    v, i = _select(np.where(S > -np.inf, _rank_key(S), -1), S, k, row_desc=True)
    out_v, out_i = np.array(v), np.array(i)
    for q in range(S.shape[0]):
        m = int((i[q] >= 0).sum())
        o = np.lexsort((i[q, :m], -v[q, :m]))
        out_v[q, :m], out_i[q, :m] = v[q, o], i[q, o]
    return out_v, out_i


def _rank_key(S):
    """a non-negative integer key in float order (the correct transform): flip all bits of negatives, set the top bit of
    the others."""
    b = _f32_bits(S)
    return np.where(b >> 31, b ^ 0xFFFFFFFF, b | 0x80000000)


TOPK_MUTANTS = {"magnitude": mutant_magnitude, "threshold-zero": mutant_threshold_zero, "zero-padding": mutant_zero_padding,
                "ties-high-row": mutant_ties_high_row}
RANGE_MUTANTS = {"range-strict": mutant_range_strict, "range-bits": mutant_range_bits}


# ------------------------------------------------------------------------------------------------ the shape table
# The regime of each row on 256 CUs, from bf_regime (csrc/bf_kernels.h; TM = 256 rows per corpus tile, KMAX = 64, SQ = 16)
# and choose_split / stream_regions / launch_stream (csrc/bf_index.hip):
#   stream when k > 64 and not (nq > 32 and tiles >= 64), or nq <= (k > 32 ? 8 : 16) and tiles >= 8; the stream kernel is
#   "wide" (8 queries a launch) for k > 32; its merge is K4 when narrow with <= 64 regions (regions = min(tiles, 256)),
#   else K4s (+ K4w for what K4s flags);
#   wide batch when k > 64, nq > 32 and tiles >= 64; everything else is the batch kernel K2, whose thresholds come from the
#   row-count certificate for k <= 16 and from the scheduled radix compactions for 16 < k <= 64, over S = min(tiles,
#   256 / T) splits of T = ceil(nq / 256) query tiles.
# (name, nq, n, d, amp, ks, family B spreads (all negative, crossing zero) or () where the row runs family A only)
# Over 40 000 rows the best scores lie higher, and at 0.2 only 2 % of the top-10 lists (22 % of the top-64) still cross
# zero; at 0.17 a third of the top-10 and 70 % of the top-64 lists do, so those rows cross at 0.17.
DENSE = [
    # 9 tiles >= 8, nq = 16 <= 16, k <= 32: stream narrow, 9 regions <= 64 -> K4
    ("k2s-narrow-k4", 16, 2053, 64, 2, (1, 10, 32), SPREADS_B),
    # 66 tiles, nq = 5: stream narrow, 66 regions > 64 -> K4s
    ("k2s-narrow-k4s", 5, 16641, 64, 2, (32,), ()),
    # 9 tiles, nq = 8 <= 8, 32 < k <= 64: stream wide
    ("k2s-wide", 8, 2053, 64, 2, (33, 64), SPREADS_B),
    # k = 200 > 64, nq = 20 <= 32: stream wide, launches of 8 + 8 + 4 queries (zero rows behind the last 4)
    ("k2s-wide-3-launches", 20, 2053, 64, 2, (200,), SPREADS_B),
    # d = 200 (padded to 256), 67 tiles, k = 200, nq = 3: stream wide, 67 regions
    ("k2s-wide-d200", 3, 17000, 200, 1, (200,), SPREADS_B),
    # 9 tiles, nq = 40 > 16: batch, T = 1, S = min(9, 256) = 9 splits of one tile; k <= 16: certificate
    ("k2-certificate", 40, 2053, 64, 2, (10, 16), SPREADS_B),
    # 157 tiles, T = 5, S = 256 / 5 = 51 splits of about 3 tiles: the thresholds of later tiles decide
    ("k2-certificate-5-qtiles", 1025, 40000, 64, 2, (10,), (0.1, 0.17)),
    # the same grid, 16 < k <= 64: radix compactions
    ("k2-radix-5-qtiles", 1025, 40000, 64, 2, (17, 64), (0.1, 0.17)),
    # d = 256, 12 tiles, nq = 40: batch, T = 1, S = 12; k = 33: radix compactions
    ("k2-radix-d256", 40, 3000, 256, 1, (33,), SPREADS_B),
]
# 66 tiles >= 64, nq = 40 > 32, 64 < k <= 256: wide batch (K2 at k' = 64 + verifier + redo through the stream kernel)
WIDE = ("wide-batch", 40, 16641, 64, 2, (100, 200))
# the rows that run again with MRAG_K4S_CAP=0 (every query through K4w)
K4W = ("k2s-wide-3-launches", "k2s-wide-d200")
# filtered and range searches: (row, k), every regime and every multi-tile row.  With filter_path="compact" the regime is
# decided by the rows that remain: of the 2 053-row shapes at most 5 tiles (< 8), so their compact runs take the batch
# kernel whatever nq is (k = 200 excepted: k > 64 with nq <= 32 streams at any size); stream + compact is the k4s row
# under the half mask (8 320 rows, 33 tiles, nq = 5) and the d = 200 row; the 5-query-tile rows keep 20 000 rows under the
# half mask (79 tiles, S = 51: later-tile thresholds decide on masked rows and on the floor).
FILTERED = [("k2s-narrow-k4", 10), ("k2s-narrow-k4s", 32), ("k2s-wide", 33), ("k2s-wide-3-launches", 200),
            ("k2s-wide-d200", 200), ("k2-certificate", 10), ("k2-certificate-5-qtiles", 10), ("k2-radix-5-qtiles", 17),
            ("k2-radix-5-qtiles", 64), ("k2-radix-d256", 33)]
DENSE_BY_NAME = {r[0]: r for r in DENSE}
# search_sets: 12 questions over 3 sets of 40, 300 and 5 rows
SETS = {"nq": 12, "n": 2053, "d": 64, "amp": 2, "k": 10, "sizes": (40, 300, 5)}
# fp8 scan, family B only
FP8 = [(7, 256), (300, 256), (7, 200), (300, 200)]
FP8_N, FP8_K = 3000, 10

# IVF-flat (csrc/ivf_scan.hip): per query the select kernel takes the register path up to SEL_CAP = 8 192 candidates (the
# per-wave bound for k <= 16, the block bisection above), the streamed path beyond, and the serial path when more than
# 512 rows tie on the k-th score or the candidates are at most k.
# (name, n, nq, d, amp, nlist, nprobe, ks, family B too, q_cols)
IVF = [
    # 20 000 rows in 64 lists, 8 probed: ~2 500 candidates <= 8 192
    ("register", 20000, 30, 64, 2, 64, 8, (10, 16, 17, 64), True, None),
    # every one of 8 lists probed: 20 000 candidates > 8 192
    ("streamed", 20000, 10, 64, 2, 8, 8, (10,), False, None),
    # 8 integer columns in [-1, 1], queries zero behind their first 3: at most 7 distinct scores over 20 000 candidates, the
    # best of them held by 20 000 / 27 rows or more -> more than 512 tie on the k-th
    ("serial-ties", 20000, 10, 9, 1, 8, 8, (10,), False, 3),
    # 7 candidates <= k
    ("serial-small", 7, 10, 64, 2, 4, 4, (10,), False, None),
]
IVF_BY_NAME = {r[0]: r for r in IVF}
IVF_FUSED_KS = (10, 40)
