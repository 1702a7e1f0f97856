#!/usr/bin/env python3
"""Development timing of the BM25 search at batches of 1 ... 10 000 questions -- not the graded bench.

The corpus of tools/perf_bm25.py (Zipf, 1 M documents, vocabulary of 30 000), top_k = 200, questions of 1 and of 3
expanded queries with 4-5 tokens each, batches of 1, 32, 1 000 and 10 000 questions.  Per shape: ms per call and us per
question of ``search_batch``, the same questions as a loop of ``search`` (a batch of one question per call: the same
kernels, so the loop shows what one call per question costs, not another implementation), the number of chunks, and
whether both give identical lists.

First leg, ``mrag_bm25_search`` through ctypes: us per call of the C entry point for one question, median of 200 calls
after 20 warm-ups.  It is the leg to compare two builds of the library with: build the other commit's library (say into
build_ab/base.so) and run, on one box and alternating as tools/ab.sh does,
    MRAG_HIP_LIB=build_ab/base.so python tools/perf_bm25_batch.py --loop-only --sizes 1
    python tools/perf_bm25_batch.py --loop-only --sizes 1
A build from before the single search became a batch of one runs its own single-question kernels there; the Python
classes of this tree reach every build through ``mrag_bm25_search_batch``.  ``--loop-only`` leaves ``search_batch`` out.
Every result is also printed as one JSON line (prefix "JSON ").
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

V = 30000
TOP_K = 200
DEFAULT_LIMIT = 1 << 30


def corpus(n):
    rng = np.random.default_rng(7)
    p = 1.0 / np.arange(1, V + 1) ** 1.07
    p /= p.sum()
    lens = rng.integers(5, 40, size=n)
    words = rng.choice(V, size=int(lens.sum()), p=p)
    rows, at = [], 0
    for i, L in enumerate(lens):
        rows.append({"doc_id": f"T{i // 5}#{i % 5}", "title": f"T{i // 5}", "sent_id": i % 5, "text": " ".join(f"w{w}" for w in words[at:at + L])})
        at += L
    return rows, p


def questions(n, per_question, p):
    rng = np.random.default_rng(1000 + per_question)
    out = []
    for _ in range(n):
        out.append([" ".join(f"w{w}" for w in rng.choice(V, size=int(rng.integers(4, 6)), p=p)) for _ in range(per_question)])
    return out


def n_chunks(sizes, n_docs, limit):
    """The chunking rule of csrc/bm25.hip: whole questions in order while their rows fit, at most 1024 per chunk."""
    cap = min(max(limit // (8 * n_docs), 1), 65535)
    chunks = rows = held = 0
    for s in sizes:
        if s == 0:
            continue
        if not chunks or rows + s > cap or held == 1024:
            chunks, rows, held = chunks + 1, 0, 0
        rows, held = rows + s, held + 1
    return chunks


def abi_single_us(ix, question, reps=200):
    """median us per call of ``mrag_bm25_search`` for the expanded queries of one question"""
    import ctypes as C
    from mrag_amd import _native as N
    from mrag_amd.text_index import tokenize
    q_ptr, terms, idf = [0], [], []
    for q in question:
        for t in tokenize(q):
            terms.append(ix._term_id.get(t, -1))
            idf.append(ix._idf(t))
        q_ptr.append(len(terms))
    qp, qt, qi = np.asarray(q_ptr, dtype=np.int32), np.asarray(terms or [0], dtype=np.int32), np.asarray(idf or [0.0])
    k = min(TOP_K, ix.N)
    docs, scores, n = np.empty(k, dtype=np.int64), np.empty(k), C.c_int(0)

    def call():
        N.check(ix._lib.mrag_bm25_search(ix._h, len(question), qp.ctypes.data, qt.ctypes.data, qi.ctypes.data, 0, k,
                                         docs.ctypes.data, scores.ctypes.data, C.byref(n), None))
    timed(call, 20)
    return 1e6 * float(np.median(timed(call, reps)[1]))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_docs", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--sizes", default="1,32,1000,10000")
    ap.add_argument("--limit", type=int, default=0, help="scratch limit in bytes (0 = the default)")
    a = ap.parse_args()
    from mrag_amd import _native as N
    from mrag_amd.text_index import HipBM25Index
    rows, p = corpus(a.n_docs)
    t0 = time.perf_counter()
    ix = HipBM25Index(rows=rows)
    print(f"BM25 n={a.n_docs} docs, vocab {len(ix.df)}: build {time.perf_counter() - t0:.1f} s; library {N.lib_path()}", flush=True)
    if a.limit and not a.loop_only:
        ix.set_scratch_limit(a.limit)
    sizes = [int(s) for s in a.sizes.split(",")]
    for per_question in (1, 3):
        pool = questions(max(sizes), per_question, p)
        us = abi_single_us(ix, pool[0])
        print(f"  {per_question} q/question: mrag_bm25_search through ctypes {us:7.1f} us/call", flush=True)
        print("JSON " + json.dumps({"n_docs": a.n_docs, "queries_per_question": per_question, "abi_single_us": us}), flush=True)
        ix.search(pool[0], top_k=TOP_K)
        if not a.loop_only:
            ix.search_batch(pool[:2], top_k=TOP_K)
        for nq in sizes:
            qs = pool[:nq]
            reps = 30 if nq == 1 else (10 if nq <= 32 else 3)
            rec = {"n_docs": a.n_docs, "queries_per_question": per_question, "questions": nq, "reps": reps}
            loop, lt = timed(lambda: [ix.search(q, top_k=TOP_K) for q in qs], reps)
            rec.update(loop_ms=1e3 * float(np.median(lt)), loop_ms_min=1e3 * min(lt), loop_ms_max=1e3 * max(lt),
                       loop_us_per_question=1e6 * float(np.median(lt)) / nq)
            line = f"  {per_question} q/question x {nq:5d}: loop of search {rec['loop_ms']:9.3f} ms ({rec['loop_us_per_question']:7.1f} us/question, " \
                   f"min {rec['loop_ms_min']:.3f} max {rec['loop_ms_max']:.3f})"
            if not a.loop_only:
                got, bt = timed(lambda: ix.search_batch(qs, top_k=TOP_K), reps)
                rec.update(batch_ms=1e3 * float(np.median(bt)), batch_ms_min=1e3 * min(bt), batch_ms_max=1e3 * max(bt),
                           batch_us_per_question=1e6 * float(np.median(bt)) / nq,
                           chunks=n_chunks([per_question] * nq, a.n_docs, a.limit or DEFAULT_LIMIT), identical=got == loop)
                line += f"; search_batch {rec['batch_ms']:9.3f} ms ({rec['batch_us_per_question']:7.1f} us/question, min {rec['batch_ms_min']:.3f} " \
                        f"max {rec['batch_ms_max']:.3f}), {rec['chunks']} chunk(s), identical: {rec['identical']}"
            print(line, flush=True)
            print("JSON " + json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
