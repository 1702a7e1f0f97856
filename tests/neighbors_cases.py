"""Neighbour expansion of search hits (``DenseIndex.expand_neighbors``, ``mrag_index_expand_neighbors``): the host
restatement of its semantics and the cases of tests/test_neighbors_host.py and tests/test_gpu_neighbors.py.  No GPU here.

The restatement keeps, per reached row, the smallest (distance, seed position) in a dict and sorts once -- not the
kernel's two sorts over padded entries."""
import json
from pathlib import Path

import numpy as np

from mrag_amd.index import reference_decay

GOLDEN = Path(__file__).resolve().parent / "golden" / "f11_graph_neighbors.json"
WINDOWS = (0, 1, 2, 5, 16)
N_ROWS = 1801                     # 7 whole 256-row tiles + 9 rows
DIM = 64


# ------------------------------------------------------------------------------------------------ the restatement
def reached(seed_row, keys, window, id_base=0):
    """``{local row: (dist, seed position)}`` of one question's seed ids"""
    n = len(keys)
    best = {}
    for j, sid in enumerate(np.asarray(seed_row).tolist()):
        r = sid - id_base
        if sid == -1 or r < 0 or r >= n:
            continue
        lo = hi = r
        while lo - 1 >= 0 and r - (lo - 1) <= window and keys[lo - 1] == keys[r]:
            lo -= 1
        while hi + 1 < n and (hi + 1) - r <= window and keys[hi + 1] == keys[r]:
            hi += 1
        for c in range(lo, hi + 1):
            cand = (abs(c - r), j)
            if c not in best or cand < best[c]:
                best[c] = cand
    return best


def expand(seeds, keys, window, m=None, decay=None, id_base=0):
    """the four outputs of the call: (scores fp32, ids int64, dist int32, seed int32), each [nq, m]"""
    seeds = np.asarray(seeds, dtype=np.int64)
    nq, s = seeds.shape
    if m is None:
        m = max(1, min(4096, s * (2 * window + 1)))
    dk = (reference_decay(window) if decay is None else np.asarray(decay)).astype(np.float32)
    sc = np.full((nq, m), -np.inf, dtype=np.float32)
    ids = np.full((nq, m), -1, dtype=np.int64)
    dist = np.full((nq, m), -1, dtype=np.int32)
    seed = np.full((nq, m), -1, dtype=np.int32)
    for q in range(nq):
        order = sorted((d, j, c) for c, (d, j) in reached(seeds[q], keys, window, id_base).items())
        for slot, (d, j, c) in enumerate(order[:m]):
            sc[q, slot], ids[q, slot], dist[q, slot], seed[q, slot] = dk[d], id_base + c, d, j
    return sc, ids, dist, seed


def graph_hits(rows, dense_ids, keys, window, seed_k, pool):
    """the graph channel's hit list of one request, from its dense id list, as ``DenseRetrievalBackend`` builds it: the
    leading ``seed_k`` dense ids (inside the call's limits) are the seeds, ``pool`` is m, the score is the reference's fp64
    decay value of the distance"""
    from mrag_amd import fusion
    seed_k = max(0, min(seed_k, 256, 4096 // (2 * window + 1), len(dense_ids)))
    if seed_k == 0:
        return []
    _, ids, dist, _ = expand(np.asarray(dense_ids[:seed_k], dtype=np.int64)[None, :], keys, window, m=min(pool, 4096))
    decay = reference_decay(window)
    return [{"id": fusion.raw_hit_id(rows[i]), "score": float(decay[d]), "meta": dict(fusion.row_meta(rows[i], "graph"), distance=int(d))}
            for i, d in zip(ids[0].tolist(), dist[0].tolist()) if i >= 0]


# ------------------------------------------------------------------------------------------------ the fixture
def golden_cases():
    """the F11 cases as ``(keys, seeds [1, s], window, {row: (score, distance)})``"""
    out = []
    for case in json.loads(GOLDEN.read_text())["cases"]:
        keys = np.repeat(np.arange(len(case["doc_lens"]), dtype=np.int32), case["doc_lens"])
        want = {int(r): (float(v[0]), int(v[1])) for r, v in case["expanded"].items()}
        out.append((keys, np.asarray([case["seeds"]], dtype=np.int64), int(case["window"]), want))
    return out


# ------------------------------------------------------------------------------------------------ key layouts
def one_run(n):
    return np.full(n, 3, dtype=np.int32)


def own_runs(n):
    return np.arange(n, dtype=np.int32)


def runs_1_to_7(n):
    """runs of lengths 1, 2, .. 7, 1, 2, .. : every run its own key"""
    lens, total = [], 0
    while total < n:
        lens.append(len(lens) % 7 + 1)
        total += lens[-1]
    return np.repeat(np.arange(len(lens), dtype=np.int32), lens)[:n]


def recurring(n):
    """runs of length 3 whose keys cycle through 0 1 2: every key recurs, never contiguously"""
    return ((np.arange(n) // 3) % 3).astype(np.int32)


LAYOUTS = {"one_run": one_run, "own_runs": own_runs, "runs_1_to_7": runs_1_to_7, "recurring": recurring}


def run_bounds(keys):
    """(lo, hi) of every row's run"""
    n = len(keys)
    change = np.flatnonzero(np.diff(keys) != 0) + 1
    starts = np.concatenate([[0], change])
    ends = np.concatenate([change, [n]]) - 1
    which = np.searchsorted(starts, np.arange(n), side="right") - 1
    return starts[which], ends[which]


def edge_seeds(keys, id_base=0):
    """seed ids at row 0 and row n - 1, at the first and the last row of runs in the middle, and inside a run of length 1
    and 2 (shorter than every window >= 2)"""
    n = len(keys)
    lo, hi = run_bounds(keys)
    mid = n // 2
    rows = [0, n - 1, int(lo[mid]), int(hi[mid]), int(lo[n // 3]), int(hi[2 * n // 3])]
    length = hi - lo + 1
    for want in (1, 2):
        at = np.flatnonzero(length == want)
        if len(at):
            rows.append(int(at[len(at) // 2]))
    return np.asarray(rows, dtype=np.int64) + id_base


def random_seeds(n, nq, s, seed, id_base=0, invalid=True):
    """[nq, s] seed ids over n rows: clustered (reaches overlap), with duplicates, and -- with ``invalid`` -- some -1, ids
    below id_base and ids at or above id_base + n"""
    rng = np.random.default_rng(seed)
    centre = rng.integers(0, n, size=(nq, 1))
    out = np.clip(centre + rng.integers(-12, 13, size=(nq, s)), 0, n - 1).astype(np.int64)
    far = rng.random((nq, s)) < 0.3
    out[far] = rng.integers(0, n, size=int(far.sum()))
    out += id_base
    first = out[:, 0].copy()
    if invalid:
        kind = rng.random((nq, s))
        out[kind < 0.08] = -1
        out[(kind >= 0.08) & (kind < 0.12)] = id_base - 1 - rng.integers(0, 5)
        out[(kind >= 0.12) & (kind < 0.16)] = id_base + n + rng.integers(0, 5)
    if s > 2:
        out[:, 0] = out[:, -1] = first                                       # a valid seed, and its duplicate at the last position
    return out


# entries = seed_stride * (2 * window + 1) -> (seed_stride, window): both sides of a wave (64) and of the padded size (2047
# sorts in P = 2048, 2050 in P = 4096) and the largest count the limits allow.  2048, 2049 and 4096 themselves have no
# factorisation with seed_stride <= 256 and an odd 2 * window + 1 <= 33 (2048 and 4096 are powers of two, 2049 = 3 * 683),
# so no call can have them: their nearest neighbours stand in, and 4097 = 241 * 17 is the smallest count refused as too large
ENTRY_SHAPES = {63: (21, 1), 64: (64, 0), 65: (13, 2), 2047: (89, 11), 2050: (82, 12), 4095: (195, 10)}
ENTRIES_REFUSED = (241, 8)        # 4097 entries


def pm1_rows(n, dim, seed):
    return np.random.default_rng(seed).choice([-1.0, 1.0], size=(n, dim)).astype(np.float16)


def title_of(row):
    return row.get("title")
