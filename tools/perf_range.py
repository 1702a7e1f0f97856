#!/usr/bin/env python3
"""Range search cost against the floor (the table behind DESIGN.md "Range search").

1M x 768 fp16, Gaussian rows and the clustered recipe of oracle.dense_search.make_clustered (centroid + 0.3 N(0,1) rows,
queries = a random row + 0.1 N(0,1); generated on the device), {1, 1 000, 10 000} queries, k in {10, 200}.  Floors: from
the exact fp32 scores of a 64-query sample, the pooled quantiles at which the mean count is about 0.1, 1, 10, 100 and
10 000 rows per query, plus a floor below every score (-2).  Whole-search device ms (last_timing_ms()[1], median of 5 after
a warm-up), range search and the plain search at the same k measured in rotation.  Then a self-join of the clustered rows
at 0.9 (k = 64, batches of 16 384), wall time.  One JSON line per point (--json FILE) and a table."""
import argparse
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from mrag_amd.index import DenseIndex

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--nq", default="1,1000,10000")
ap.add_argument("--k", default="10,200")
ap.add_argument("--counts", default="0.1,1,10,100,10000")
ap.add_argument("--data", default="gaussian,clustered")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--self-join", type=float, default=0.9, help="floor of the clustered self-join (<= -3: skip)")
ap.add_argument("--json", default=None)
args = ap.parse_args()
out = open(args.json, "w") if args.json else None


def emit(r):
    if out:
        out.write(json.dumps(r) + "\n")
        out.flush()


def make(kind):
    g = torch.Generator(device="cuda").manual_seed(11)
    nq_max = max(int(x) for x in args.nq.split(","))
    if kind == "gaussian":
        rows = [torch.randn(min(250_000, args.n - lo), args.dim, device="cuda", generator=g) for lo in range(0, args.n, 250_000)]
        q = torch.randn(nq_max, args.dim, device="cuda", generator=g)
        return rows, q
    cent = torch.randn(4096, args.dim, device="cuda", generator=g)
    rows = []
    for lo in range(0, args.n, 250_000):
        m = min(250_000, args.n - lo)
        which = torch.randint(0, 4096, (m,), device="cuda", generator=g)
        rows.append(cent[which] + 0.3 * torch.randn(m, args.dim, device="cuda", generator=g))
    pick = torch.randint(0, args.n, (nq_max,), device="cuda", generator=g)
    allr = torch.cat(rows)
    q = allr[pick] + 0.1 * torch.randn(nq_max, args.dim, device="cuda", generator=g)
    return rows, q


def floors(ix, q, counts):
    """pooled quantiles of the exact fp32 scores of 64 sample queries: mean count per query ~ each target"""
    qs = torch.nn.functional.normalize(q[:64].double(), dim=1).float().half().float()   # as K1 prepares them
    S = []
    for r0 in range(0, len(ix), 250_000):
        m = min(250_000, len(ix) - r0)
        rr = torch.from_numpy(ix.rows(r0, m)).cuda()
        S.append(qs @ rr.T)
    S = torch.cat(S, 1).flatten()
    res = {}
    for c in counts:
        t = max(1, int(round(c * qs.shape[0])))
        res[c] = float(torch.topk(S, t).values[-1])
    return res


def timed_pair(q, k, floor):
    """range search and plain search in rotation; -> ((range ms, kernel ms), (plain ms, kernel ms), counts)"""
    ix.range_search(q, floor, k)
    ix.search(q, k)
    tr, tp = [], []
    for _ in range(args.reps):
        _, _, cnt = ix.range_search(q, floor, k)
        tr.append(ix.last_timing_ms())
        ix.search(q, k)
        tp.append(ix.last_timing_ms())
    torch.cuda.synchronize()
    med = lambda ts, i: float(np.median([t[i] for t in ts]))
    return (med(tr, 1), med(tr, 0)), (med(tp, 1), med(tp, 0)), cnt.cpu().numpy()


print("| data | queries | k | target count | floor | mean count | truncated | range ms | plain ms | ratio |")
print("|---|---|---|---|---|---|---|---|---|---|")
for kind in args.data.split(","):
    rows, qall = make(kind)
    ix = DenseIndex(args.dim)
    ix.reserve(args.n)
    for r in rows:
        ix.add(r)
    del rows
    torch.cuda.synchronize()
    fl = floors(ix, qall, [float(c) for c in args.counts.split(",")])
    fl["below"] = -2.0
    for nq in (int(x) for x in args.nq.split(",")):
        q = qall[:nq].contiguous()
        for k in (int(x) for x in args.k.split(",")):
            for tgt, f in fl.items():
                (rm, rg), (pm, pg), cnt = timed_pair(q, k, f)
                r = dict(data=kind, nq=nq, k=k, target=tgt, floor=f, mean_count=float(cnt.mean()),
                         truncated=float((cnt > k).mean()), range_ms=rm, range_kernel_ms=rg, plain_ms=pm, plain_kernel_ms=pg,
                         ratio=rm / pm)
                emit(r)
                print(f"| {kind} | {nq} | {k} | {tgt} | {f:.4f} | {r['mean_count']:.4g} | {100 * r['truncated']:.1f} % | "
                      f"{rm:.3f} | {pm:.3f} | {rm / pm:.3f} |", flush=True)
    if kind == "clustered" and args.self_join > -3:
        t0 = time.perf_counter()
        sc, ids, cnt = ix.self_join(args.self_join, k=64, batch=16384)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        c = cnt.cpu().numpy()
        flop = 2.0 * args.n * args.n * args.dim
        r = dict(data=kind, self_join=args.self_join, n=args.n, k=64, seconds=dt, pflops=flop / dt / 1e15,
                 mean_count=float(c.mean()), truncated=float((c > 64).mean()))
        emit(r)
        print(f"self-join {args.n} rows at {args.self_join}: {dt:.3f} s ({r['pflops']:.3f} PFLOP/s of 2 n^2 d), "
              f"mean count {r['mean_count']:.1f}, truncated {100 * r['truncated']:.1f} %", flush=True)
    ix.close()
    torch.cuda.empty_cache()
