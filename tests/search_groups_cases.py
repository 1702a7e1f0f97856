"""Case builders and the host restatement shared by tests/test_search_groups_host.py (which checks, without a GPU, the
restatement and what the cases hold) and tests/test_gpu_search_groups.py (which runs them through
``DenseIndex.search_groups``).  numpy only.

A case is ``(queries, sizes)``: question g owns ``sizes[g]`` consecutive query rows."""
import zlib

import numpy as np

from filter_sets_cases import gaussian_rows, pick, pm1_rows, pm1_vec, small_int_rows  # noqa: F401  (re-exported builders)
from oracle import dense_search as ds

DIMS = (64, 96, 768)
KS = (1, 10, 64, 65, 200, 256)
MAX_ENTRIES = 4096                # queries x k of one question
TOL = 1e-5                        # the oracle yardstick of tests/test_gpu_filter_sets.py
N_EXACT = 2003                    # 7 whole 256-row tiles + 211 rows
# totals on both sides of the 16-query boundary between the streaming and the batch kernel, every group size the issue
# names (1, 2, 5, 16), empty groups at the front, in the middle and at the end, a group of one between larger ones
LAYOUTS = {
    "below16": [2, 5, 1],                           # 8 queries
    "at16": [16],
    "above16": [5, 0, 1, 2, 0, 5, 4],               # 17
    "mixed": [0, 1, 2, 5, 16, 0, 1, 16, 3, 0],      # 44
}


def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def merge_groups(scores, ids, group_ptr, k):
    """The rule of ``mrag_index_search_groups`` over per-query result lists ``scores`` / ``ids`` [nq, k'], written with a
    dict per question and Python's sort, not with the kernel's sorts: per question drop the id -1, keep per id the
    largest score (float comparison: -0.0 == +0.0) and among equal scores the lowest query position, order by
    (score desc, id asc), cut at k -> (scores [G, k] fp32, ids [G, k] int64, which [G, k] int32), (-inf, -1, -1) tails."""
    scores, ids = np.asarray(scores, dtype=np.float32), np.asarray(ids, dtype=np.int64)
    ptr = np.asarray(group_ptr, dtype=np.int64)
    G = len(ptr) - 1
    out_sc = np.full((G, k), -np.inf, dtype=np.float32)
    out_id = np.full((G, k), -1, dtype=np.int64)
    out_wh = np.full((G, k), -1, dtype=np.int32)
    for g in range(G):
        best = {}
        for j, qi in enumerate(range(int(ptr[g]), int(ptr[g + 1]))):
            for s, i in zip(scores[qi], ids[qi].tolist()):
                if i == -1:
                    continue
                if i not in best or s > best[i][0]:
                    best[i] = (s, j)
        order = sorted(best.items(), key=lambda kv: (-float(kv[1][0]), kv[0]))[:k]
        for r, (i, (s, j)) in enumerate(order):
            out_sc[g, r], out_id[g, r], out_wh[g, r] = s, i, j
    return out_sc, out_id, out_wh


def topk_lists(score_matrix, k):
    """per query (row of ``score_matrix`` [q, n]) the top-k by (score desc, column asc), padded with (-inf, -1)"""
    s = np.asarray(score_matrix, dtype=np.float32)
    v, i = ds.topk_desc_rowasc(s.astype(np.float64), min(k, s.shape[1]))
    v = np.take_along_axis(s, i, axis=1)                  # the fp32 values themselves
    pad = k - v.shape[1]
    if pad > 0:
        v = np.concatenate([v, np.full((s.shape[0], pad), -np.inf, dtype=np.float32)], axis=1)
        i = np.concatenate([i, np.full((s.shape[0], pad), -1, dtype=np.int64)], axis=1)
    return v, i.astype(np.int64)


def rowwise_max_topk(score_matrix, k):
    """top-k of the row-wise maximum over the queries, (score desc, column asc), with the FIRST query that reaches it"""
    s = np.asarray(score_matrix, dtype=np.float32)
    m, w = s.max(axis=0), s.argmax(axis=0)
    order = np.lexsort((np.arange(s.shape[1]), -m.astype(np.float64)))[:k]
    return m[order], order.astype(np.int64), w[order].astype(np.int32)


def oracle_groups(q, c, sizes, k, id_base=0):
    """fp64: per question ``brute_force_topk`` over the row-wise max of the fp64 score matrix of its queries (the max as
    a one-column corpus against the query [1.0], so that the oracle's own ordering and padding apply)"""
    ptr = ptr_of(sizes)
    rv, ri = np.full((len(sizes), k), -np.inf), np.full((len(sizes), k), -1, dtype=np.int64)
    c64 = np.asarray(c, dtype=np.float64)
    for g in range(len(sizes)):
        if ptr[g + 1] == ptr[g] or len(c) == 0:
            continue
        m = (np.asarray(q[ptr[g]:ptr[g + 1]], dtype=np.float64) @ c64.T).max(axis=0)
        v, i = ds.brute_force_topk(np.ones((1, 1)), m[:, None], k)
        rv[g], ri[g] = v[0], np.where(i[0] >= 0, i[0] + id_base, -1)
    return rv, ri


# ------------------------------------------------------------------------------------------------ exact rows
def exact_case(dim, layout, seed=0):
    """rows and queries whose products sum exactly in fp32 in any order (+-1 entries for dims 96 / 768, small integers for
    dim 64), exact in f16 and in bf16 -> (rows, queries, sizes)"""
    sizes = LAYOUTS[layout]
    nq = int(np.sum(sizes))
    if dim == 64:
        return small_int_rows(N_EXACT, dim, 300 + seed), small_int_rows(nq, dim, 400 + seed), sizes
    return pm1_rows(N_EXACT, dim, 300 + seed), pm1_rows(nq, dim, 400 + seed), sizes


def duplicates_case(dim=96):
    """rows 100 .. 199 are copies of query a0, rows 300 .. 349 of a and rows 50 .. 54 of b: copies score the maximum, dim,
    and tie among themselves (ids ascending).  The groups repeat queries: group 0 is a0 four times (every id occurs four
    times with equal scores -> which = 0 everywhere), group 1 is (a, b, a): an id whose best score comes from a must name
    position 0, never 2 -> (rows, queries, sizes)"""
    c = pm1_rows(N_EXACT, dim, 501)
    q = pm1_rows(3, dim, 502)
    c[100:200], c[300:350], c[50:55] = q[0], q[1], q[2]
    return c, np.stack([q[0]] * 4 + [q[1], q[2], q[1]]), [4, 3]


def signed_zero_case(dim=64):
    """bf16 rows and two queries whose only products underflow fp32 with opposite signs: row r has 2^-100 in column 0
    (rows 0 .. 9) and is zero elsewhere, the queries are +-2^-100 in column 0.  Every score is a zero; whichever signs the
    search gives them, one id meets the zeros of both queries -> (rows, queries, sizes)"""
    c = np.zeros((300, dim), dtype=np.float32)
    c[:10, 0] = 2.0 ** -100
    q = np.zeros((2, dim), dtype=np.float32)
    q[0, 0], q[1, 0] = -(2.0 ** -100), 2.0 ** -100
    return c, q, [2]


# ------------------------------------------------------------------------------------------------ position independence
N_POS, DIM_POS, B_POS = 4000, 96, 130


def position_case():
    """a probe question of 3 Gaussian queries and 129 filler questions of 0 .. 6 queries each -> (rows, probe queries,
    filler queries, filler sizes)"""
    c = gaussian_rows(N_POS, DIM_POS, 61)
    sizes = [(g * 5) % 7 for g in range(B_POS - 1)]
    return c, gaussian_rows(3, DIM_POS, 62), gaussian_rows(int(np.sum(sizes)), DIM_POS, 63), sizes


def place(probe_q, fill_q, fill_sizes, at):
    """the batch with the probe at question ``at`` -> (queries, sizes)"""
    cut = int(np.sum(fill_sizes[:at]))
    return np.concatenate([fill_q[:cut], probe_q, fill_q[cut:]]), list(fill_sizes[:at]) + [len(probe_q)] + list(fill_sizes[at:])


# ------------------------------------------------------------------------------------------------ the backend's corpus
def expander(*, query, trace_id):
    """deterministic expansion: the query's words in two other orders, plus one unrelated sentence"""
    w = query.split()
    return [" ".join(reversed(w)), " ".join(w[1:] + w[:1]), "king of the river city"]


def failing_expander(*, query, trace_id):
    raise RuntimeError("the expander is down")


def long_expander(*, query, trace_id):
    """25 queries in all: more than 4096 // 200 = 20"""
    return [f"{query} {zlib.crc32(query.encode()) % 97} {i}" for i in range(24)]
