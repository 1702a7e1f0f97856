#!/usr/bin/env python3
"""Development timing of the collapsed dense search against the same build's plain search followed by the host
restatement of the rounds -- not the graded bench.

One dense index of ``--rows`` x 768 f16 rows (default 200 000), Gaussian, with keys in contiguous runs of 1 / 4 / 16 rows.
Queries: 1 / 1 000 / 10 000; k: 10 and 200; ``scan_k``: the default (``collapse_scan_k``) and ``min(256, 4 k)``.  Each
shape runs ``DenseIndex.search_collapsed`` against ``DenseIndex.search`` at the same ``scan_k`` followed by
``collapse_rounds`` of tests/search_collapsed_cases.py (a set and a list per query, and ``search(allow=)`` for a query
that must be redone: what a caller without the collapsed search writes).  The host side is timed in its two parts; its
collapse may be cut to the first ``--host-queries`` queries (default 1 000) and is then scaled to the whole batch, which
the record says.  Then one clustered case in which EVERY query needs redo rounds: blocks of 1 000 near-identical rows under
one key each, 100 queries (at most one per block) next to block centres, k = 10 at depth 256, so a round meets few keys.
The two sides alternate over three rounds after one warm-up each; the figures are the medians of the rounds.  Every
result is also printed as one JSON line (prefix "JSON ").
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np

DIM, ROUNDS = 768, 3
QUERIES, RUNS, KS = (1, 1000, 10000), (1, 4, 16), (10, 200)


def unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def measure(ix, q, keys, k, scan_k, n_h):
    """both sides at one shape -> the record (without the shape)"""
    from search_collapsed_cases import collapse_rounds

    def run_collapsed():
        return ix.search_collapsed(q, k, scan_k=scan_k, normalize=False)

    def run_host(depth):
        t0 = time.perf_counter()
        sc0, id0 = ix.search(q, depth, normalize=False)
        t1 = time.perf_counter()

        def fn(qidx, allow):
            if allow is None:
                return sc0[:n_h], id0[:n_h]
            return ix.search(np.ascontiguousarray(q[qidx]), depth, normalize=False, allow=allow)
        out = collapse_rounds(fn, n_h, keys, k, depth)
        return out, t1 - t0, time.perf_counter() - t1

    got = run_collapsed()                                       # warm-up at the full shape: the work buffers grow here
    lc = ix.last_collapsed()
    host, _, _ = run_host(lc["scan_k"])
    same = all(x[:n_h].tobytes() == y.tobytes() for x, y in zip(got, host[:3]))
    tc, ts, tm = [], [], []
    for _ in range(ROUNDS):
        t0 = time.perf_counter(); run_collapsed(); tc.append(time.perf_counter() - t0)
        _, s, m = run_host(lc["scan_k"]); ts.append(s); tm.append(m * len(q) / n_h)
    c_med, s_med, m_med = float(np.median(tc)), float(np.median(ts)), float(np.median(tm))
    return {"k": k, "rounds": ROUNDS, "collapsed_ms": 1e3 * c_med, "collapsed_ms_min": 1e3 * min(tc), "collapsed_ms_max": 1e3 * max(tc),
            "search_ms": 1e3 * s_med, "host_collapse_ms": 1e3 * m_med, "host_queries_timed": n_h,
            "host_over_collapsed": (s_med + m_med) / c_med, "same_bits": bool(same), **lc}


def show(tag, rec):
    print(f"  {tag}: search_collapsed {rec['collapsed_ms']:10.3f} ms (min {rec['collapsed_ms_min']:.3f} max {rec['collapsed_ms_max']:.3f}); "
          f"search({rec['scan_k']}) {rec['search_ms']:10.3f} ms + host collapse {rec['host_collapse_ms']:11.3f} ms (timed on "
          f"{rec['host_queries_timed']} queries); x{rec['host_over_collapsed']:.1f}; redone {rec['redone_queries']} queries in "
          f"{rec['redo_rounds']} searches; same bits: {rec['same_bits']}", flush=True)
    print("JSON " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--host-queries", type=int, default=1000)
    a = ap.parse_args()
    from mrag_amd import _native as N
    from mrag_amd.index import DenseIndex
    rng = np.random.default_rng(1)
    ix = DenseIndex(DIM, dtype="f16")
    for lo in range(0, a.rows, 100_000):
        ix.add(rng.standard_normal((min(100_000, a.rows - lo), DIM)).astype(np.float32))
    print(f"dense index {a.rows} x {DIM} f16; library {N.lib_path()}", flush=True)
    for run in RUNS:
        keys = (np.arange(a.rows) // run).astype(np.int32)
        ix.set_row_keys(keys)
        for nq in QUERIES:
            q = unit(rng.standard_normal((nq, DIM)))
            n_h = min(nq, a.host_queries) if a.host_queries else nq
            for k in KS:
                for scan_k in (None, min(256, 4 * k)):
                    rec = {"rows": a.rows, "rows_per_key": run, "queries": nq, "scan": "default" if scan_k is None else "4k",
                           **measure(ix, q, keys, k, scan_k, n_h)}
                    show(f"runs of {run:2d}, {nq:6d} queries, k = {k:3d}, scan_k {rec['scan']:>7s} = {rec['scan_k']:3d}", rec)
    ix.close()

    # every query is redone: blocks of 1 000 rows around one centre each, one key per block
    block, k = 1000, 10
    n_blocks = a.rows // block
    nq = min(100, n_blocks)
    centres = unit(rng.standard_normal((n_blocks, DIM)))
    ix = DenseIndex(DIM, dtype="f16")
    for lo in range(0, n_blocks, 100):
        cen = np.repeat(centres[lo:lo + 100], block, axis=0)
        ix.add(cen + 0.01 * rng.standard_normal(cen.shape).astype(np.float32))
    keys = (np.arange(n_blocks * block) // block).astype(np.int32)
    ix.set_row_keys(keys)
    q = unit(centres[rng.choice(n_blocks, size=nq, replace=False)] + 0.01 * rng.standard_normal((nq, DIM)).astype(np.float32))
    rec = {"rows": n_blocks * block, "rows_per_key": block, "queries": nq, "scan": "256", "clustered": True,
           **measure(ix, q, keys, k, 256, nq)}
    show(f"clustered blocks of {block}, {nq} queries, k = {k}, scan_k 256", rec)
    ix.close()


if __name__ == "__main__":
    main()
