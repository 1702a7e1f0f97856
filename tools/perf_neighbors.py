#!/usr/bin/env python3
"""Development timing of the neighbour expansion (the device graph channel) against the same expansion in plain Python
on the same seeds -- not the graded bench.

One dense index of ``--rows`` x 64 f16 rows (default 200 000; the expansion never reads the rows, only their keys) with
keys in contiguous runs of 4 rows (a HotpotQA paragraph).  Seeds are the reference's pool of 200 ids per question, drawn
at random.  Three parts:
  1. one question at the pool of 200 with windows 1 / 2;
  2. 1 000 and 10 000 questions, same pool and windows;
  3. ``DenseRetrievalBackend.run_batch`` of ``--requests`` requests over a synthetic ``docs.jsonl`` of ``--docs`` rows with
     the BM25 channel, with and without ``graph_channel="neighbors"``.
Parts 1 and 2 run ``DenseIndex.expand_neighbors`` with host buffers (the call ends in a synchronisation), and with device
seeds and outputs followed by a stream synchronisation, against ``neighbors_cases.expand`` of tests/ -- a dict per question
in plain Python, what a caller without the call writes; the Python side may be cut to the first ``--host-questions``
questions (default 1 000) and is then scaled to the whole batch, which the record says.  The sides alternate over three
rounds after one warm-up each; the figures are the medians.  Every result is also printed as one JSON line (prefix "JSON ").
"""
import argparse
import json
import sys
import tempfile
import time
import zlib
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np

DIM, ROUNDS, POOL = 64, 3, 200
WORDS = ["alpha", "beta", "gamma", "delta", "river", "city", "born", "film", "band", "album", "war", "king"]


def med(fn):
    fn()
    t = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter(); fn(); t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def measure(ix, keys, seeds, window, n_h):
    import torch
    from neighbors_cases import expand
    got = ix.expand_neighbors(seeds, window, m=POOL, return_from=True)
    want = expand(seeds[:n_h], keys, window, m=POOL)
    same = all(a[:n_h].tobytes() == b.tobytes() for a, b in zip(got, want))
    ds = torch.from_numpy(seeds).cuda()
    out = ix.expand_neighbors(ds, window, m=POOL, return_from=True)

    def device():
        ix.expand_neighbors(ds, window, m=POOL, return_from=True, out=out)
        torch.cuda.synchronize()
    host_ms = med(lambda: ix.expand_neighbors(seeds, window, m=POOL, return_from=True))
    dev_ms = med(device)
    py_ms = med(lambda: expand(seeds[:n_h], keys, window, m=POOL)) * len(seeds) / n_h
    return {"window": window, "questions": len(seeds), "seeds": seeds.shape[1], "m": POOL, "host_buffers_ms": host_ms,
            "device_buffers_ms": dev_ms, "python_ms": py_ms, "python_questions_timed": n_h, "same_bits": bool(same),
            **ix.last_neighbors()}


class Router:
    def embed(self, *, model_hint, texts, require=None):
        out = []
        for t in texts:
            rng = np.random.default_rng(zlib.crc32(t.encode("utf-8")))
            out.append(rng.standard_normal(DIM).astype(np.float32).tolist())
        return {"vectors": out}


def backend_part(n_docs, n_req):
    from mrag_amd import corpus
    from mrag_amd.backend import DenseRetrievalBackend
    from mrag_amd.dto import RetrievalIn
    rng = np.random.default_rng(3)
    rows = [{"doc_id": f"Title {i // 4}#{i % 4}", "title": f"Title {i // 4}", "sent_id": i % 4,
             "text": " ".join(rng.choice(WORDS, size=int(rng.integers(4, 12))))} for i in range(n_docs)]
    reqs = [RetrievalIn(query=" ".join(rng.choice(WORDS, size=int(rng.integers(2, 5)))), graph_id="", top_k=20, trace_id=f"t{g}")
            for g in range(n_req)]
    with tempfile.TemporaryDirectory() as td:
        path = Path(td) / "docs.jsonl"
        corpus.write_docs_jsonl(path, rows)
        rec = {"docs": n_docs, "requests": n_req}
        for name, kw in (("without_graph_ms", {}), ("with_graph_ms", {"graph_channel": "neighbors"})):
            b = DenseRetrievalBackend(Router(), index_path=str(path), text_channel="bm25", bulk_ingest=False, **kw)
            rec[name] = med(lambda: b.run_batch(reqs))
            if kw:
                rec["graph_candidates"] = int(np.mean([o["diagnostics"]["graph_candidates"] for o in b.run_batch(reqs)]))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--host-questions", type=int, default=1000)
    ap.add_argument("--docs", type=int, default=20_000)
    ap.add_argument("--requests", type=int, default=256)
    a = ap.parse_args()
    from mrag_amd import _native as N
    from mrag_amd.index import DenseIndex
    rng = np.random.default_rng(1)
    ix = DenseIndex(DIM, dtype="f16")
    for lo in range(0, a.rows, 100_000):
        ix.add(rng.standard_normal((min(100_000, a.rows - lo), DIM)).astype(np.float32))
    keys = (np.arange(a.rows) // 4).astype(np.int32)
    ix.set_row_keys(keys)
    print(f"dense index {a.rows} x {DIM} f16, runs of 4; library {N.lib_path()}", flush=True)
    for nq in (1, 1000, 10000):
        seeds = rng.integers(0, a.rows, size=(nq, POOL)).astype(np.int64)
        for window in (1, 2):
            rec = {"rows": a.rows, **measure(ix, keys, seeds, window, min(nq, a.host_questions))}
            print(f"  {nq:6d} questions x {POOL} seeds, window {window}: host buffers {rec['host_buffers_ms']:9.3f} ms, device buffers "
                  f"{rec['device_buffers_ms']:9.3f} ms, plain Python {rec['python_ms']:11.3f} ms (timed on {rec['python_questions_timed']}); "
                  f"same bits: {rec['same_bits']}", flush=True)
            print("JSON " + json.dumps(rec), flush=True)
    ix.close()
    rec = backend_part(a.docs, a.requests)
    print(f"  run_batch of {rec['requests']} requests over {rec['docs']} rows, BM25 + dense: {rec['without_graph_ms']:.3f} ms without, "
          f"{rec['with_graph_ms']:.3f} ms with the graph channel ({rec['graph_candidates']} graph candidates per request)", flush=True)
    print("JSON " + json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
