#!/usr/bin/env python3
"""Development timing of the batched hybrid retrieval against its one-question forms -- not the graded bench.

Part 1, fusion: questions of 200 text + 0 graph + 200 dense hits (the reference's pools), batches of 1, 32, 1 000 and
10 000 questions.  Per size: ms per call and us per question of ``fusion.fuse_channels_device_batch``, the same
questions as a loop of ``fusion.fuse_channels_device``, and whether both give identical lists.

Part 2, backend: ``DenseRetrievalBackend.run_batch`` on 1 000 requests over a 200 000-row corpus (``text_channel="bm25"``,
``fuse_on_device=True``, a stub router with 64-dimensional embeddings) against the loop of ``run``.

The baseline of a comparison is the PARENT build's loop, not this build's: build the parent's library (say into
build_ab/base.so), then run, on one box, three rounds of
    MRAG_HIP_LIB=build_ab/base.so python tools/perf_hybrid_batch.py --loop-only
    python tools/perf_hybrid_batch.py
alternating as tools/ab.sh does; the spread of the parent's three rounds is the noise a difference has to exceed.
``--loop-only`` times only the loops; a library without the batch entry point is accepted there.
Every result is also printed as one JSON line (prefix "JSON ").
"""
import argparse
import json
import sys
import tempfile
import time
import zlib
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

POOL = 200
ALPHAS = dict(alpha_text=0.4, alpha_graph=0.2, alpha_dense=0.4)
WORDS = [f"w{i}" for i in range(3000)]


def fusion_questions(n):
    """n questions: 200 text hits and 200 dense scores over 300 ids, so a third of the ids sit in both channels"""
    rng = np.random.default_rng(5)
    out = []
    for g in range(n):
        ids = [f"sent::T{g % 97}-{j}::{j % 4}" for j in range(300)]
        t_pick, d_pick = rng.permutation(300)[:POOL], rng.permutation(300)[:POOL]
        t_sc, d_sc = np.sort(rng.random(POOL) * 20)[::-1], np.sort(rng.random(POOL).astype(np.float32))[::-1]
        text = [{"id": ids[i], "score": float(s), "meta": {"doc": f"T{g % 97}-{i}", "sent_id": i % 4, "text": "x"}} for i, s in zip(t_pick, t_sc)]
        out.append((text, [], {ids[i]: float(s) for i, s in zip(d_pick, d_sc)}))
    return out


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, ts


def stats(prefix, ts, n):
    return {f"{prefix}_ms": 1e3 * float(np.median(ts)), f"{prefix}_ms_min": 1e3 * min(ts), f"{prefix}_ms_max": 1e3 * max(ts),
            f"{prefix}_us_per_question": 1e6 * float(np.median(ts)) / n}


class Router:
    """64-dimensional embeddings from the text's CRC: deterministic, cheap, no model"""

    def embed(self, *, model_hint, texts, require=None):
        out = np.empty((len(texts), 64), dtype=np.float32)
        for i, t in enumerate(texts):
            out[i] = np.random.default_rng(zlib.crc32(t.encode("utf-8"))).standard_normal(64)
        return {"vectors": out}


def backend_part(a):
    from mrag_amd import corpus
    from mrag_amd.backend import DenseRetrievalBackend
    from mrag_amd.dto import RetrievalIn
    rng = np.random.default_rng(9)
    p = 1.0 / np.arange(1, len(WORDS) + 1) ** 1.07
    p /= p.sum()
    lens = rng.integers(5, 30, size=a.rows)
    words = rng.choice(len(WORDS), size=int(lens.sum()), p=p)
    rows, at = [], 0
    for i, L in enumerate(lens):
        rows.append({"doc_id": f"T{i // 5}#{i % 5}", "title": f"T{i // 5}", "sent_id": i % 5, "text": " ".join(WORDS[w] for w in words[at:at + L])})
        at += L
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "docs.jsonl"
        corpus.write_docs_jsonl(path, rows)
        be = DenseRetrievalBackend(Router(), index_path=str(path), text_channel="bm25", fuse_on_device=True, embed_batch=4096)
        reqs = [RetrievalIn(query=" ".join(WORDS[w] for w in rng.choice(len(WORDS), size=5, p=p)), graph_id="", top_k=20, trace_id=f"t{g}")
                for g in range(a.requests)]
        t0 = time.perf_counter()
        be.run(reqs[0])
        print(f"backend over {a.rows} rows: first run (builds both indexes) {time.perf_counter() - t0:.1f} s", flush=True)
        rec = {"part": "backend", "rows": a.rows, "requests": a.requests}
        loop, lt = timed(lambda: [be.run(r) for r in reqs], 1)
        rec.update(stats("loop", lt, a.requests))
        line = f"  {a.requests} requests: loop of run {rec['loop_ms']:9.1f} ms ({rec['loop_us_per_question']:7.1f} us/request)"
        if not a.loop_only:
            be.run_batch(reqs[:2])
            got, bt = timed(lambda: be.run_batch(reqs), 3)
            rec.update(stats("batch", bt, a.requests))
            rec["same_ids"] = sum([h["id"] for h in x["hits"]] == [h["id"] for h in y["hits"]] for x, y in zip(got, loop))
            line += f"; run_batch {rec['batch_ms']:9.1f} ms ({rec['batch_us_per_question']:7.1f} us/request); same id lists: {rec['same_ids']}/{a.requests}"
        print(line, flush=True)
        print("JSON " + json.dumps(rec), flush=True)
        corpus.drop_shared("dense-index|")
        corpus.drop_shared("bm25-index|")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--sizes", default="1,32,1000,10000")
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--requests", type=int, default=1000)
    ap.add_argument("--skip-backend", action="store_true")
    a = ap.parse_args()
    from mrag_amd import _native as N
    if a.loop_only:
        import ctypes
        lib = ctypes.CDLL(str(N.lib_path()))
        for name in list(getattr(N, "FUSE_BATCH_SIGNATURES", {})):
            if not hasattr(lib, name):
                N.FUSE_BATCH_SIGNATURES.pop(name)
    from mrag_amd import fusion
    print(f"library {N.lib_path()}", flush=True)
    sizes = [int(s) for s in a.sizes.split(",")]
    pool = fusion_questions(max(sizes))
    fusion.fuse_channels_device(*pool[0], top_k=20, **ALPHAS)
    if not a.loop_only:
        fusion.fuse_channels_device_batch(pool[:2], top_k=20, **ALPHAS)
    for nq in sizes:
        qs = pool[:nq]
        reps = 30 if nq == 1 else (10 if nq <= 32 else 3)
        rec = {"part": "fusion", "questions": nq, "entries": 2 * POOL, "reps": reps}
        loop, lt = timed(lambda: [fusion.fuse_channels_device(*q, top_k=20, **ALPHAS) for q in qs], reps)
        rec.update(stats("loop", lt, nq))
        line = f"  {nq:5d} questions: loop of fuse_channels_device {rec['loop_ms']:9.3f} ms ({rec['loop_us_per_question']:7.1f} us/question, " \
               f"min {rec['loop_ms_min']:.3f} max {rec['loop_ms_max']:.3f})"
        if not a.loop_only:
            got, bt = timed(lambda: fusion.fuse_channels_device_batch(qs, top_k=20, **ALPHAS), reps)
            rec.update(stats("batch", bt, nq))
            rec["identical"] = got == loop
            line += f"; batch {rec['batch_ms']:9.3f} ms ({rec['batch_us_per_question']:7.1f} us/question, min {rec['batch_ms_min']:.3f} " \
                    f"max {rec['batch_ms_max']:.3f}), identical: {rec['identical']}"
        print(line, flush=True)
        print("JSON " + json.dumps(rec), flush=True)
    if not a.skip_backend:
        backend_part(a)


if __name__ == "__main__":
    main()
