#!/usr/bin/env python3
"""Development timing of the grouped dense search against the same build's plain search followed by the host merge --
not the graded bench.

One dense index of ``--rows`` x 768 f16 rows (default 200 000).  Questions: 1 / 1 000 / 10 000; query vectors per question
(the question and its expansions): 1 / 4 / 8; k: 10 and 200.  Each shape runs ``DenseIndex.search_groups`` against
``DenseIndex.search`` of all the query vectors followed by ``merge_groups`` of tests/search_groups_cases.py, the host
restatement of the merge (a dict per question and a sort: what a caller without the grouped search writes).  The host
side is timed in its two parts; its merge may be cut to the first ``--merge-questions`` questions (default 1 000) and is
then scaled to the whole batch, which the record says.  The two sides alternate over three rounds after one warm-up each;
the figures are the medians of the rounds.  Every result is also printed as one JSON line (prefix "JSON ").
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
QUESTIONS, EXPANSIONS, KS = (1, 1000, 10000), (1, 4, 8), (10, 200)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--merge-questions", type=int, default=1000)
    a = ap.parse_args()
    from mrag_amd import _native as N
    from mrag_amd.index import DenseIndex
    from search_groups_cases import merge_groups
    rng = np.random.default_rng(1)
    ix = DenseIndex(DIM, dtype="f16")
    for lo in range(0, a.rows, 100_000):
        ix.add(rng.standard_normal((min(100_000, a.rows - lo), DIM)).astype(np.float32))
    print(f"dense index {a.rows} x {DIM} f16; library {N.lib_path()}", flush=True)
    for n_q in QUESTIONS:
        for e in EXPANSIONS:
            q = rng.standard_normal((n_q * e, DIM)).astype(np.float32)
            ptr = np.arange(0, n_q * e + 1, e, dtype=np.int64)
            n_m = min(n_q, a.merge_questions) if a.merge_questions else n_q
            for k in KS:
                def run_groups():
                    return ix.search_groups(q, k, group_ptr=ptr, return_which=True)

                def run_host():
                    t0 = time.perf_counter()
                    sc, ids = ix.search(q, k)
                    t1 = time.perf_counter()
                    out = merge_groups(sc[:n_m * e], ids[:n_m * e], ptr[:n_m + 1], k)
                    return out, t1 - t0, time.perf_counter() - t1

                got, (host, _, _) = run_groups(), run_host()                # warm-up at the full shape: the work buffers grow here
                same = all(x[:n_m].tobytes() == y.tobytes() for x, y in zip(got, host))
                tg, ts, tm = [], [], []
                for _ in range(ROUNDS):
                    t0 = time.perf_counter(); run_groups(); tg.append(time.perf_counter() - t0)
                    _, s, m = run_host(); ts.append(s); tm.append(m * n_q / n_m)
                g_med, s_med, m_med = float(np.median(tg)), float(np.median(ts)), float(np.median(tm))
                rec = {"rows": a.rows, "questions": n_q, "queries_per_question": e, "k": k, "rounds": ROUNDS,
                       "groups_ms": 1e3 * g_med, "groups_ms_min": 1e3 * min(tg), "groups_ms_max": 1e3 * max(tg),
                       "search_ms": 1e3 * s_med, "host_merge_ms": 1e3 * m_med, "host_merge_questions_timed": n_m,
                       "host_over_groups": (s_med + m_med) / g_med, "same_bits": bool(same), **ix.last_groups()}
                print(f"  {n_q:6d} questions x {e} queries, k = {k:3d}: search_groups {rec['groups_ms']:10.3f} ms (min {rec['groups_ms_min']:.3f} "
                      f"max {rec['groups_ms_max']:.3f}); search {rec['search_ms']:10.3f} ms + host merge {rec['host_merge_ms']:11.3f} ms "
                      f"(timed on {n_m} questions); x{rec['host_over_groups']:.1f}; same bits: {same}", flush=True)
                print("JSON " + json.dumps(rec), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
