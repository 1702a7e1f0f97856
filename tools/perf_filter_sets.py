#!/usr/bin/env python3
"""Development timing of the dense search over per-question allow-sets against the loop of single filtered searches --
not the graded bench.

200 000 and 1 000 000 x 768 f16 rows (``--rows``), k = 10, three regimes:
    own40      1 000 questions, each with its own 40-row set (HotpotQA's distractor setting)
    shared5k   1 000 questions over 10 shared sets of 5 000 rows
    routed100k one 100 000-row set shared by 500 questions (above the scan route: one filtered search)
Each regime runs ``DenseIndex.search_sets`` against the loop of ``search(Q[g:g+1], k, allow=set_g)`` over the same
questions -- that loop is the parent's behaviour and is unchanged in this build.  The two sides alternate over three rounds
in one process order (sets, loop, sets, loop, ...) after one warm-up each; the figures are the medians of the rounds: ms per
call, us per question, and the ratio of the two whole-call times.  The loop side may be cut to the first ``--loop-questions``
questions (default: all); its per-question time is what is compared.
Every result is also printed as one JSON line (prefix "JSON ").
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

DIM, K, ROUNDS = 768, 10, 3


def regimes(n, rng):
    own = [np.sort(rng.choice(n, size=40, replace=False)) for _ in range(1000)]
    shared = [np.sort(rng.choice(n, size=5000, replace=False)) for _ in range(10)]
    big = [np.sort(rng.choice(n, size=100_000, replace=False))]
    return [("own40", own, np.arange(1000, dtype=np.int32)),
            ("shared5k", shared, (np.arange(1000) % 10).astype(np.int32)),
            ("routed100k", big, np.zeros(500, dtype=np.int32))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="200000,1000000")
    ap.add_argument("--loop-questions", type=int, default=0)
    a = ap.parse_args()
    from mrag_amd import _native as N
    from mrag_amd.index import DenseIndex
    for n in [int(x) for x in a.rows.split(",")]:
        rng = np.random.default_rng(1)
        ix = DenseIndex(DIM, dtype="f16")
        for lo in range(0, n, 100_000):
            ix.add(rng.standard_normal((min(100_000, n - lo), DIM)).astype(np.float32))
        print(f"dense index {n} x {DIM} f16, k = {K}; library {N.lib_path()}", flush=True)
        for name, sets, set_of in regimes(n, rng):
            nq = len(set_of)
            q = rng.standard_normal((nq, DIM)).astype(np.float32)
            n_loop = min(nq, a.loop_questions) if a.loop_questions else nq

            def run_sets():
                return ix.search_sets(q, K, sets, set_of=set_of)

            def run_loop():
                return [ix.search(q[g:g + 1], K, allow=sets[set_of[g]]) for g in range(n_loop)]

            got, loop = run_sets(), run_loop()                         # warm-up at the full shape: the work buffers grow here
            same = all(got[1][g].tolist() == loop[g][1][0].tolist() for g in range(n_loop))
            ts, tl = [], []
            for _ in range(ROUNDS):
                t0 = time.perf_counter(); run_sets(); ts.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); run_loop(); tl.append(time.perf_counter() - t0)
            s_med, l_med = float(np.median(ts)), float(np.median(tl))
            rec = {"rows": n, "regime": name, "questions": nq, "loop_questions": n_loop, "k": K, "rounds": ROUNDS,
                   "sets_ms": 1e3 * s_med, "sets_ms_min": 1e3 * min(ts), "sets_ms_max": 1e3 * max(ts),
                   "sets_us_per_question": 1e6 * s_med / nq,
                   "loop_ms": 1e3 * l_med, "loop_ms_min": 1e3 * min(tl), "loop_ms_max": 1e3 * max(tl),
                   "loop_us_per_question": 1e6 * l_med / n_loop,
                   "loop_over_sets_per_question": (l_med / n_loop) / (s_med / nq), "same_ids": bool(same), **ix.last_sets()}
            print(f"  {name:10s}: search_sets {rec['sets_ms']:9.3f} ms ({rec['sets_us_per_question']:8.1f} us/question, min {rec['sets_ms_min']:.3f} "
                  f"max {rec['sets_ms_max']:.3f}); loop {rec['loop_ms']:10.3f} ms ({rec['loop_us_per_question']:8.1f} us/question, min "
                  f"{rec['loop_ms_min']:.3f} max {rec['loop_ms_max']:.3f}); x{rec['loop_over_sets_per_question']:.1f}; same ids: {same}", flush=True)
            print("JSON " + json.dumps(rec), flush=True)
        ix.close()


if __name__ == "__main__":
    main()
