"""Case builders shared by tests/test_filter_sets_host.py (which checks, without a GPU, that the cases hold what they are
built for) and tests/test_gpu_filter_sets.py (which runs them through ``DenseIndex.search_sets``).  numpy only.

A case is ``(sets, set_of)``: a list of ascending row-position arrays and, per question, the index of its set."""
import zlib

import numpy as np

from oracle import dense_search as ds

N_GRID = 5003                     # 19 whole 256-row tiles + 139 rows: the last tile is partial
DIMS = (64, 96, 768)
KS = (1, 10, 64, 200, 256)
SET_SIZES = (0, 1, 7, 8, 9, 127, 128, 129, 300, 2000)
QUESTIONS_PER_SET = (1, 2, 127, 128, 129, 130)
SEL_CAP = 8192                    # the scan route's largest set
TOL = 1e-5


def round_bf16(x):
    """fp32 -> bf16 (round to nearest even) -> fp32"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def gaussian_rows(n, dim, seed):
    """normalised Gaussian rows, rounded once to fp16 (the stored bits)"""
    return ds.normalize_round(ds.make_gaussian(n, dim, seed))


def pick(n, m, seed):
    return np.sort(np.random.default_rng(seed).choice(n, size=m, replace=False)).astype(np.int64)


def grid_layout(n=N_GRID):
    """Every set size shared by a cycling number of questions, then one question with a set of its own per size, then the
    edge sets: row 0 alone, the last row alone, row 0 and the last row, only rows of the partial last 256-row tile.
    Shared and per-question sets stand in ONE call, interleaved by a fixed permutation of the questions."""
    sets, set_of = [], []
    for i, m in enumerate(SET_SIZES):
        sets.append(pick(n, m, 100 + i))
        set_of += [len(sets) - 1] * QUESTIONS_PER_SET[i % len(QUESTIONS_PER_SET)]
    sets.append(pick(n, 300, 150))                  # three row chunks x two question groups
    set_of += [len(sets) - 1] * 130
    for i, m in enumerate(SET_SIZES):
        sets.append(pick(n, m, 200 + i))
        set_of.append(len(sets) - 1)
    tail0 = n - n % 256
    edges = [np.asarray([0]), np.asarray([n - 1]), np.asarray([0, n - 1]), np.arange(tail0, n), pick(n - tail0, 9, 7) + tail0]
    for e in edges:
        sets.append(e.astype(np.int64))
        set_of += [len(sets) - 1] * 2
    set_of = np.asarray(set_of, dtype=np.int32)
    return sets, set_of[np.random.default_rng(5).permutation(len(set_of))]


def oracle(q, c, sets, set_of, k, id_base=0):
    """fp64 top-k of every question over c[its set], (score desc, row asc), ids = id_base + row, (-inf, -1) tails"""
    nq = len(set_of)
    rv, ri = np.full((nq, k), -np.inf), np.full((nq, k), -1, dtype=np.int64)
    for s, rows in enumerate(sets):
        qs = np.flatnonzero(np.asarray(set_of) == s)
        if rows.size == 0 or qs.size == 0:
            continue
        v, i = ds.brute_force_topk(q[qs], c[rows], k)
        rv[qs], ri[qs] = v, np.where(i >= 0, rows[np.maximum(i, 0)] + id_base, -1)
    return rv, ri


# ------------------------------------------------------------------------------------------------ ties
N_TIES, DIM_TIES = 6000, 64


def identical_rows_case():
    """rows 1000 .. 3999 of the corpus are one and the same row; the set takes 2 000 of them: every score ties"""
    c = gaussian_rows(N_TIES, DIM_TIES, 31)
    c[1000:4000] = c[1000]
    q = gaussian_rows(3, DIM_TIES, 32)
    return c, q, [pick(3000, 2000, 33) + 1000], np.zeros(3, dtype=np.int32)


def integer_rows_case():
    """integer-valued rows whose score against the questions takes two values: column 0 is 2 on every third row and 1
    elsewhere, the other columns are small integers the questions do not look at.  The set of 4 000 rows holds ~1 333 rows
    of the higher score: k = 200 and 256 cut inside that tie, which the row order must resolve"""
    rng = np.random.default_rng(41)
    c = rng.integers(-2, 3, size=(N_TIES, DIM_TIES)).astype(np.float16)
    c[:, 0] = np.where(np.arange(N_TIES) % 3 == 0, 2, 1)
    q = np.zeros((2, DIM_TIES), dtype=np.float16)
    q[0, 0], q[1, 0] = 3, 1
    return c, q, [pick(N_TIES, 4000, 42)], np.zeros(2, dtype=np.int32)


def ties_on_kth(q, c, rows, k):
    """exact ties on the k-th fp64 score of every question over c[rows]"""
    s = np.asarray(q, dtype=np.float64) @ np.asarray(c[rows], dtype=np.float64).T
    kth = -np.sort(-s, axis=1)[:, k - 1]
    return (s == kth[:, None]).sum(axis=1)


# ------------------------------------------------------------------------------------------------ k above the set size
def k_above_m_cases():
    """(set size, k) with fewer rows than k, for every size of the grid below the largest k"""
    return [(m, k) for m in SET_SIZES for k in KS if m < k]


# ------------------------------------------------------------------------------------------------ position independence
N_POS, DIM_POS, B_POS = 4000, 96, 300


def position_case():
    """a probe question with a 300-row set of its own and 299 filler questions: every third filler has a 40-row set of its
    own, the others share three sets of 300, 129 and 7 rows -> (c, probe query, probe set, filler queries, filler sets,
    filler set_of)"""
    c = gaussian_rows(N_POS, DIM_POS, 51)
    q = gaussian_rows(B_POS, DIM_POS, 52)
    shared = [pick(N_POS, 300, 53), pick(N_POS, 129, 54), pick(N_POS, 7, 55)]
    sets, set_of = list(shared), []
    for g in range(B_POS - 1):
        if g % 3 == 0:
            sets.append(pick(N_POS, 40, 1000 + g))
            set_of.append(len(sets) - 1)
        else:
            set_of.append(g % 3 - 1 if g % 2 else 2)
    return c, q[:1], pick(N_POS, 300, 56), q[1:], sets, np.asarray(set_of, dtype=np.int32)


def place(probe_q, probe_set, fill_q, fill_sets, fill_of, at):
    """the batch with the probe at position ``at`` -> (queries, sets, set_of)"""
    q = np.concatenate([fill_q[:at], probe_q, fill_q[at:]])
    set_of = np.concatenate([fill_of[:at], [len(fill_sets)], fill_of[at:]]).astype(np.int32)
    return q, list(fill_sets) + [probe_set], set_of


# ------------------------------------------------------------------------------------------------ exact rows
def pm1_rows(n, dim, seed):
    """+-1 entries: every score is an integer that fp32 sums exactly in any order"""
    return np.random.default_rng(seed).choice([-1.0, 1.0], size=(n, dim)).astype(np.float16)


def small_int_rows(n, dim, seed):
    return np.random.default_rng(seed).integers(-3, 4, size=(n, dim)).astype(np.float16)


# ------------------------------------------------------------------------------------------------ the backend's corpus
WORDS = ["alpha", "beta", "gamma", "delta", "river", "city", "born", "film", "band", "album", "war", "king"]


def pm1_vec(text, dim=64):
    """exactly 16 entries of +-1: every cosine is a multiple of 1/16 that fp32 sums exactly in any order, so the scan, the
    batch kernel and the one-query kernel agree bit for bit, with many exact ties"""
    rng = np.random.default_rng(zlib.crc32(text.encode("utf-8")))
    v = np.zeros(dim, dtype=np.float32)
    v[rng.choice(dim, size=16, replace=False)] = rng.choice([-1.0, 1.0], size=16)
    return v.tolist()


def doc_rows(n=800):
    rng = np.random.default_rng(3)
    return [{"doc_id": f"Title {i // 4}#{i % 4}", "title": f"Title {i // 4}", "sent_id": i % 4,
             "text": " ".join(rng.choice(WORDS, size=int(rng.integers(4, 12))))} for i in range(n)]


def doc_queries(n=33):
    rng = np.random.default_rng(17)
    return [" ".join(rng.choice(WORDS, size=int(rng.integers(2, 5)))) for _ in range(n)]


def three_sets_or_none(req, rows):
    """the backend's ``dense_row_filter`` of the tests: by the query's length, no filter, the even rows (a mask), the first
    300 rows (positions, unsorted and with a duplicate) or the rows of every fourth title (a mask)"""
    n, kind = len(rows), len(req.query) % 4
    if kind == 0:
        return None
    if kind == 1:
        return np.arange(n) % 2 == 0
    if kind == 2:
        return np.concatenate([np.arange(299, -1, -1), [5]])
    return (np.arange(n) // 4) % 4 == 0
