#!/usr/bin/env python3
"""Development timing of the hybrid retrieval at batches of 1 ... 10 000 questions -- not the graded bench.

Part 1, fusion: questions of 200 text + 0 graph + 200 dense hits (the reference's pools), batches of 1, 32, 1 000 and
10 000 questions.  First ``mrag_fuse_topk`` through ctypes: us per call of the C entry point for one question, median
of 200 calls after 20 warm-ups.  Then per size: ms per call and us per question of ``fusion.fuse_channels_device_batch``,
the same questions as a loop of ``fusion.fuse_channels_device`` (a batch of one question per call: the same kernel),
and whether both give identical lists.

Part 2, backend: ``DenseRetrievalBackend.run_batch`` on 1 000 requests over a 200 000-row corpus (``text_channel="bm25"``,
``fuse_on_device=True``, a stub router with 64-dimensional embeddings) against the loop of ``run``.

To compare two builds of the library, build the other commit's (say into build_ab/base.so), then run, on one box, three
rounds of
    MRAG_HIP_LIB=build_ab/base.so python tools/perf_hybrid_batch.py --loop-only
    python tools/perf_hybrid_batch.py --loop-only
alternating as tools/ab.sh does; the spread of one build's three rounds is the noise a difference has to exceed.  The
ctypes leg is the one that reaches a build's own single-question kernel, where it has one (builds from before
``mrag_fuse_topk`` became a batch of one); the Python functions of this tree reach every build through
``mrag_fuse_topk_batch``.  ``--loop-only`` leaves the batch calls out.
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


def abi_single_us(question, reps=200):
    """median us per call of ``mrag_fuse_topk`` for one question's entries (keys = ranks of the sorted ids, as
    ``fusion.fuse_channels_device`` builds them)"""
    import ctypes as C
    from mrag_amd import _native as N, fusion
    text, graph, dense = question
    chans = [[(fusion.normalize_id(h)[0], float(h["score"])) for h in hits] for hits in (text, graph)] + [list(dense.items())]
    key_of = {nid: i for i, nid in enumerate(sorted({nid for ent in chans for nid, _ in ent}))}
    keys = np.asarray([key_of[nid] for ent in chans for nid, _ in ent], dtype=np.int32)
    scores = np.asarray([v for ent in chans for _, v in ent], dtype=np.float64)
    kk = min(20, len(key_of))
    ok, vals, n = np.empty(kk, dtype=np.int32), [np.empty(kk) for _ in range(4)], C.c_int(0)
    lib = N.load()

    def call():
        N.check(lib.mrag_fuse_topk(0, keys.ctypes.data, scores.ctypes.data, *[len(ent) for ent in chans], ALPHAS["alpha_text"],
                                   ALPHAS["alpha_graph"], ALPHAS["alpha_dense"], kk, ok.ctypes.data, *[v.ctypes.data for v in vals],
                                   C.byref(n), None))
    timed(call, 20)
    return 1e6 * float(np.median(timed(call, reps)[1]))


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
    from mrag_amd import fusion
    print(f"library {N.lib_path()}", flush=True)
    sizes = [int(s) for s in a.sizes.split(",")]
    pool = fusion_questions(max(sizes))
    us = abi_single_us(pool[0])
    print(f"  mrag_fuse_topk through ctypes, {2 * POOL} entries: {us:7.1f} us/call", flush=True)
    print("JSON " + json.dumps({"part": "fusion", "entries": 2 * POOL, "abi_single_us": us}), flush=True)
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
