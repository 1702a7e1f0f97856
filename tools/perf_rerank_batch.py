#!/usr/bin/env python3
"""Development timing of the batched dense re-rank against a loop of single lookups -- not the graded bench.

1 M x 768 f16 rows; batches of 1, 32, 1 000 and 10 000 questions with 200 random candidate rows each, and one skewed
batch: one question of 100 000 candidates among 999 of 20.  Per shape: ms per call and us per question of
``DenseIndex.score_rows_batch``, the same questions as a loop of ``score_rows``, bytes/s against entries * ld * 2 (the
stored rows the call has to read), and whether both give identical bits.

The baseline of a comparison is the PARENT build's loop, not this build's: build the parent's library (say into
build_ab/base.so), then run, on one box and alternating over three rounds,
    MRAG_HIP_LIB=build_ab/base.so python tools/perf_rerank_batch.py --loop-only
    python tools/perf_rerank_batch.py
``--loop-only`` times only the loop; a library without the batch entry point is accepted there.
Every result is also printed as one JSON line (prefix "JSON ").
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

DIM = 768
POOL = 200


def shapes(n_rows, sizes):
    rng = np.random.default_rng(7)
    out = [(f"{nq} x {POOL}", [rng.integers(0, n_rows, size=POOL) for _ in range(nq)]) for nq in sizes]
    skew = [rng.integers(0, n_rows, size=20) for _ in range(1000)]
    skew[500] = rng.integers(0, n_rows, size=100_000)
    out.append(("skew: 100000 among 999 x 20", skew))
    return out


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_rows", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--sizes", default="1,32,1000,10000")
    a = ap.parse_args()
    from mrag_amd import _native as N
    if a.loop_only:
        import ctypes
        if not hasattr(ctypes.CDLL(str(N.lib_path())), "mrag_index_score_rows_batch"):
            N.RERANK_BATCH_SIGNATURES.clear()
    from mrag_amd.index import DenseIndex
    rng = np.random.default_rng(1)
    ix = DenseIndex(DIM, dtype="f16")
    step = 100_000
    for lo in range(0, a.n_rows, step):
        ix.add(rng.standard_normal((min(step, a.n_rows - lo), DIM)).astype(np.float32))
    ld = (DIM + 63) // 64 * 64
    print(f"dense index {a.n_rows} x {DIM} f16; library {N.lib_path()}", flush=True)
    for name, lists in shapes(a.n_rows, [int(s) for s in a.sizes.split(",")]):
        nq, entries = len(lists), int(sum(len(x) for x in lists))
        q = rng.standard_normal((nq, DIM)).astype(np.float32)
        ptr = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum([len(x) for x in lists], out=ptr[1:])
        flat = np.concatenate(lists).astype(np.int64)
        reps = 50 if nq == 1 else (10 if nq <= 32 else 3)
        ix.score_rows(q[0], lists[0])
        rec = {"shape": name, "questions": nq, "entries": entries, "row_bytes": entries * ld * 2, "reps": reps}
        loop, lt = timed(lambda: [ix.score_rows(q[g], lists[g]) for g in range(nq)], reps)
        rec.update(loop_ms=1e3 * float(np.median(lt)), loop_ms_min=1e3 * min(lt), loop_ms_max=1e3 * max(lt),
                   loop_us_per_question=1e6 * float(np.median(lt)) / nq, loop_gb_s=rec["row_bytes"] / float(np.median(lt)) / 1e9)
        line = f"  {name:28s}: loop of score_rows {rec['loop_ms']:10.3f} ms ({rec['loop_us_per_question']:8.1f} us/question, " \
               f"min {rec['loop_ms_min']:.3f} max {rec['loop_ms_max']:.3f}, {rec['loop_gb_s']:.1f} GB/s)"
        if not a.loop_only:
            ix.score_rows_batch(q, (ptr, flat))          # warm-up at the full shape: the staging buffers grow here, not in a timed call
            got, bt = timed(lambda: ix.score_rows_batch(q, (ptr, flat))[1], reps)
            same = bool((got.view(np.uint32) == np.concatenate(loop).view(np.uint32)).all())
            rec.update(batch_ms=1e3 * float(np.median(bt)), batch_ms_min=1e3 * min(bt), batch_ms_max=1e3 * max(bt),
                       batch_us_per_question=1e6 * float(np.median(bt)) / nq, batch_gb_s=rec["row_bytes"] / float(np.median(bt)) / 1e9,
                       identical=same)
            line += f"; score_rows_batch {rec['batch_ms']:10.3f} ms ({rec['batch_us_per_question']:8.1f} us/question, min {rec['batch_ms_min']:.3f} " \
                    f"max {rec['batch_ms_max']:.3f}, {rec['batch_gb_s']:.1f} GB/s), identical: {same}"
        print(line, flush=True)
        print("JSON " + json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
