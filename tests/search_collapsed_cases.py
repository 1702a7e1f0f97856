"""Case builders, the host restatement and the fp64 oracle shared by tests/test_search_collapsed_host.py (which checks,
without a GPU, the exactness argument and what the cases hold) and tests/test_gpu_search_collapsed.py (which runs them
through ``DenseIndex.search_collapsed``).  numpy only.

A key layout is a function ``n -> int32 keys [n]``: the key of every stored row."""
import numpy as np

from filter_sets_cases import gaussian_rows, pm1_rows, pm1_vec, small_int_rows  # noqa: F401  (re-exported builders)
from oracle import dense_search as ds

DIMS = (64, 96, 768)
TOL = 1e-5                        # the oracle yardstick of tests/test_gpu_filter_sets.py
N_EXACT = 2003                    # 7 whole 256-row tiles + 211 rows
NQS = (8, 16, 17, 44)             # both sides of the 16-query boundary between the streaming and the batch kernel
# (k, scan_k): the list ends before, at and behind the wave boundary (entries 63 / 64), k = scan_k, the widest lists
K_SCAN = ((1, 1), (1, 64), (10, 63), (10, 64), (10, 65), (64, 64), (65, 255), (200, 256), (256, 256))
BIG = 2 ** 31 - 1


def runs(m):
    return lambda n: (np.arange(n) // m).astype(np.int32)


def interleaved(G):
    return lambda n: (np.arange(n) % G).astype(np.int32)


LAYOUTS = {
    "distinct": lambda n: np.arange(n, dtype=np.int32),
    "one_key": lambda n: np.full(n, 5, dtype=np.int32),
    "runs3": runs(3), "runs7": runs(7), "runs300": runs(300),           # runs cross the 256-row tile boundaries
    "interleaved5": interleaved(5), "interleaved257": interleaved(257),
    # sparse keys down from 2^31 - 1, three rows each
    "big_values": lambda n: (BIG - (np.arange(n, dtype=np.int64) // 3) * 1_000_003).astype(np.int32),
}


def collapse_rounds(search_fn, nq, keys, k, scan_k, id_base=0):
    """The rounds of ``mrag_index_search_collapsed`` over any search callable, written with Python sets and lists, not like
    the kernel.  ``search_fn(query_indexes, allow)`` returns the top-``scan_k`` lists (scores, ids) [len(query_indexes),
    scan_k] of those queries in (score desc, row asc) order over all rows (``allow`` None) or over the rows of the bool mask
    ``allow``, padded with (-inf, -1).  Round 0 searches every query; a query that has fewer than k keys after a full list
    is searched again alone over the rows whose key it has not met, and what it meets is appended.
    -> (scores [nq, k] fp32, ids [nq, k] int64, keys [nq, k] int32, rounds [nq]): (-inf, -1, -1) tails, rounds >= 1."""
    keys = np.asarray(keys)
    out_sc = np.full((nq, k), -np.inf, dtype=np.float32)
    out_id = np.full((nq, k), -1, dtype=np.int64)
    out_key = np.full((nq, k), -1, dtype=np.int32)
    rounds = np.zeros(nq, dtype=np.int64)
    if nq == 0:
        return out_sc, out_id, out_key, rounds
    sc0, id0 = search_fn(list(range(nq)), None)
    for q in range(nq):
        seen, found = set(), []
        sc, ids = sc0[q], id0[q]
        while True:
            rounds[q] += 1
            valid = 0
            for s, i in zip(sc, ids.tolist()):
                if i == -1 and np.isneginf(s):
                    continue
                valid += 1
                key = int(keys[i - id_base])
                if key not in seen:
                    seen.add(key)
                    found.append((s, i, key))
            if len(found) >= k or valid < scan_k:
                break
            sc, ids = (x[0] for x in search_fn([q], ~np.isin(keys, list(seen))))
        for r, (s, i, key) in enumerate(found[:k]):
            out_sc[q, r], out_id[q, r], out_key[q, r] = s, i, key
    return out_sc, out_id, out_key, rounds


def exact_search_fn(score_matrix, scan_k, id_base=0):
    """a ``search_fn`` for :func:`collapse_rounds`: the exact top-``scan_k`` of the rows of ``score_matrix`` [nq, n] by
    (score desc, column asc), over the allowed columns"""
    s = np.asarray(score_matrix, dtype=np.float32)

    def fn(qidx, allow):
        cols = np.arange(s.shape[1]) if allow is None else np.flatnonzero(allow)
        sc = np.full((len(qidx), scan_k), -np.inf, dtype=np.float32)
        ids = np.full((len(qidx), scan_k), -1, dtype=np.int64)
        for j, q in enumerate(qidx):
            order = cols[np.lexsort((cols, -s[q, cols].astype(np.float64)))][:scan_k]
            sc[j, :len(order)], ids[j, :len(order)] = s[q, order], order + id_base
        return sc, ids
    return fn


def index_search_fn(ix, q, scan_k):
    """a ``search_fn`` over a ``DenseIndex``: its own ``search`` and ``search(allow=)`` at depth ``scan_k``"""
    def fn(qidx, allow):
        sub = np.ascontiguousarray(q[qidx])
        if allow is None:
            return ix.search(sub, scan_k, normalize=False)
        return ix.search(sub, scan_k, normalize=False, allow=allow)
    return fn


def oracle_collapsed(q, c, keys, k, id_base=0):
    """fp64 brute force over all rows: per query every row scored, ordered by (score desc, row asc), the first row of every
    key kept, cut at k -> (scores [nq, k] fp64, ids [nq, k] int64, keys [nq, k] int32) with (-inf, -1, -1) tails"""
    q, c, keys = np.asarray(q, dtype=np.float64), np.asarray(c, dtype=np.float64), np.asarray(keys)
    rv = np.full((len(q), k), -np.inf)
    ri = np.full((len(q), k), -1, dtype=np.int64)
    rk = np.full((len(q), k), -1, dtype=np.int32)
    if len(c) == 0:
        return rv, ri, rk
    s = q @ c.T
    for g in range(len(q)):
        order = np.lexsort((np.arange(len(c)), -s[g]))
        first = np.sort(np.unique(keys[order], return_index=True)[1])[:k]      # positions in `order` of every key's first row
        rows = order[first]
        rv[g, :len(rows)], ri[g, :len(rows)], rk[g, :len(rows)] = s[g, rows], rows + id_base, keys[rows]
    return rv, ri, rk


# ------------------------------------------------------------------------------------------------ exact rows
def exact_case(dim, nq, seed=0):
    """rows and queries whose products sum exactly in fp32 in any order (+-1 entries for dims 96 / 768, small integers for
    dim 64: many exact ties), exact in f16 and in bf16 -> (rows, queries)"""
    if dim == 64:
        return small_int_rows(N_EXACT, dim, 1300 + seed), small_int_rows(nq, dim, 1400 + seed)
    return pm1_rows(N_EXACT, dim, 1300 + seed), pm1_rows(nq, dim, 1400 + seed)


# ------------------------------------------------------------------------------------------------ the redo case
REDO_BLOCK = (600, 900)           # 300 identical rows under ONE key: more than the deepest list (256)
REDO_KEY = 100_000
REDO_PROBES = (700, 650, 880)
REDO_K_SCAN = ((10, 64), (10, 256), (200, 256))


def redo_case(n_fill=13, dim=64):
    """+-1 rows; rows 600 .. 899 are copies of row 700 and share one key, every other key is a run of 3 rows.  A probe (a
    row of the block) scores the maximum, ``dim``, on all 300 rows of the block: whatever the depth, round 0 meets one key
    and the query must be redone.  The filler queries score at most 0 on the block, which then stands far behind their
    lists -> (rows, keys, probe queries, filler queries)"""
    c = pm1_rows(N_EXACT, dim, 1501)
    c[REDO_BLOCK[0]:REDO_BLOCK[1]] = c[700]
    keys = runs(3)(N_EXACT)
    keys[REDO_BLOCK[0]:REDO_BLOCK[1]] = REDO_KEY
    fill = pm1_rows(n_fill, dim, 1502)
    against = fill.astype(np.float32) @ c[700].astype(np.float32)
    fill[against > 0] *= -1
    return c, keys, np.ascontiguousarray(c[list(REDO_PROBES)]), fill


def place(probe_q, fill_q, at):
    """the batch with the one probe query at position ``at``"""
    return np.concatenate([fill_q[:at], probe_q, fill_q[at:]])


# ------------------------------------------------------------------------------------------------ Gaussian rows
GAUSS_K, GAUSS_M = 10, 3


def gaussian_case(dim, nq=44):
    """normalised Gaussian rows under runs of 3 -> (rows, keys, queries)"""
    return gaussian_rows(N_EXACT, dim, 1700 + dim), runs(GAUSS_M)(N_EXACT), gaussian_rows(nq, dim, 1800 + dim)


# ------------------------------------------------------------------------------------------------ the backend's corpus
def title_of(row):
    """the backend's ``dense_collapse`` callable of the tests: the document of a sentence row"""
    return row.get("title")
