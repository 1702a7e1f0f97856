#!/usr/bin/env python3
"""IVF range search and neighbour join: cost against the plain IVF search and the exact join (the tables behind DESIGN.md
"IVF range search").

Search part: clustered rows (4096 centres + 0.3 N(0,1), generated on the device), nlist 4096 trained on 100 000 rows,
10 000 queries, nprobe 32, k = 10.  Floors: a floor below every score (-2) and the pooled quantiles of a 64-query sample
(range search at k = 256) at which the mean count is about 0.1, 1, 10 and 100 rows per query.  Whole-search device ms
(last_timing()["total_ms"], median of --reps after a warm-up), the range search and the plain search measured in rotation.
--plain-only times the plain search alone: with MRAG_HIP_LIB pointing at another build of the library the same process
shape gives that build's figure; run the two alternately to compare builds (a build that lacks the range entry points
needs their two names dropped from _native.SIGNATURES before the library is loaded).

Join part (--join-n > 0): that many clustered rows, IVFFlatIndex.self_join at --join-floor, k = 64, for each --join-nprobe,
wall seconds, against DenseIndex.self_join on the same rows: pair recall = unordered pairs the IVF join lists / pairs the
exact join lists.  One JSON line per point (--json FILE) and tables."""
import argparse
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from mrag_amd.index import DenseIndex, IVFFlatIndex

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="625000", help="corpus sizes of the search part, comma separated (empty: skip)")
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--nprobe", type=int, default=32)
ap.add_argument("--nq", type=int, default=10000)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--counts", default="0.1,1,10,100")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--join-n", type=int, default=0)
ap.add_argument("--join-floor", type=float, default=0.9)
ap.add_argument("--join-nprobe", default="8,32")
ap.add_argument("--json", default=None)
args = ap.parse_args()
out = open(args.json, "a") if args.json else None


def emit(r):
    if out:
        out.write(json.dumps(r) + "\n")
        out.flush()


def build(n, dense=False):
    g = torch.Generator(device="cuda").manual_seed(1)
    cent = torch.randn(4096, args.dim, device="cuda", generator=g)
    draw = lambda m: cent[torch.randint(0, 4096, (m,), device="cuda", generator=g)] + 0.3 * torch.randn(m, args.dim, device="cuda", generator=g)
    ix = IVFFlatIndex(args.dim, args.nlist)
    ix.train(draw(100_000), iters=5, seed=1)
    dx = DenseIndex(args.dim) if dense else None
    for lo in range(0, n, 125_000):
        rows = draw(min(125_000, n - lo))
        ix.add(rows)
        if dx is not None:
            dx.add(rows)
    q = draw(args.nq)
    torch.cuda.synchronize()
    return ix, dx, q


def med(xs):
    return float(np.median(xs))


for n in (int(x) for x in args.n.split(",") if x):
    ix, _, q = build(n)
    k, nprobe = args.k, args.nprobe
    ix.search(q, k, nprobe)
    torch.cuda.synchronize()
    if args.plain_only:
        ts = []
        for _ in range(2 * args.reps):
            ix.search(q, k, nprobe)
            ts.append(ix.last_timing()["total_ms"])
        r = dict(part="plain_only", n=n, nq=args.nq, k=k, nprobe=nprobe, plain_ms=med(ts), plain_min=min(ts), plain_max=max(ts))
        emit(r)
        print(f"plain only, {n} rows: {r['plain_ms']:.3f} ms (min {r['plain_min']:.3f}, max {r['plain_max']:.3f})", flush=True)
        ix.close()
        continue
    sample, _, _ = ix.range_search(q[:64].contiguous(), -2.0, 256, nprobe)
    pooled = torch.sort(sample.flatten(), descending=True).values
    floors = {"below": -2.0}
    for c in (float(x) for x in args.counts.split(",")):
        floors[c] = float(pooled[max(1, int(round(c * 64))) - 1])
    print(f"| rows | target count | floor | mean count | truncated | range ms | select+scan ms | plain ms | plain select+scan ms | ratio |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for tgt, f in floors.items():
        ix.range_search(q, f, k, nprobe)
        tr, tp, sr, sp = [], [], [], []
        for _ in range(args.reps):
            _, _, cnt = ix.range_search(q, f, k, nprobe)
            t = ix.last_timing()
            tr.append(t["total_ms"]); sr.append(t["scan_ms"])
            ix.search(q, k, nprobe)
            t = ix.last_timing()
            tp.append(t["total_ms"]); sp.append(t["scan_ms"])
        c = cnt.cpu().numpy()
        r = dict(part="search", n=n, nq=args.nq, k=k, nprobe=nprobe, target=tgt, floor=f, mean_count=float(c.mean()),
                 truncated=float((c > k).mean()), range_ms=med(tr), range_scan_ms=med(sr), plain_ms=med(tp), plain_scan_ms=med(sp),
                 plain_min=min(tp), plain_max=max(tp), ratio=med(tr) / med(tp))
        emit(r)
        print(f"| {n} | {tgt} | {f:.4f} | {r['mean_count']:.4g} | {100 * r['truncated']:.1f} % | {r['range_ms']:.3f} | {r['range_scan_ms']:.3f} | "
              f"{r['plain_ms']:.3f} | {r['plain_scan_ms']:.3f} | {r['ratio']:.3f} |", flush=True)
    ix.close()
    torch.cuda.empty_cache()

if args.join_n > 0 and not args.plain_only:
    n, k = args.join_n, 64
    ix, dx, _ = build(n, dense=True)

    def pairs(ids):
        """unordered pairs (as i * n + j, i < j) listed by either side, unique"""
        src = torch.arange(n, device="cuda", dtype=torch.int64)[:, None].expand_as(ids)
        ok = ids >= 0
        a, b = src[ok], ids[ok]
        return torch.unique(torch.minimum(a, b) * n + torch.maximum(a, b))

    dx.self_join(args.join_floor, k=k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, dids, dcnt = dx.self_join(args.join_floor, k=k)
    torch.cuda.synchronize()
    dense_s = time.perf_counter() - t0
    dp = pairs(dids)
    print(f"exact join, {n} rows at {args.join_floor}: {dense_s:.3f} s, {dp.numel()} pairs, mean count {float(dcnt.float().mean()):.1f}, "
          f"truncated {100 * float((dcnt > k).float().mean()):.1f} %", flush=True)
    emit(dict(part="dense_join", n=n, floor=args.join_floor, k=k, seconds=dense_s, pairs=int(dp.numel())))
    print("| rows | nprobe | IVF join s | exact join s | pairs | exact pairs | pair recall | mean count | truncated |")
    print("|---|---|---|---|---|---|---|---|---|")
    for nprobe in (int(x) for x in args.join_nprobe.split(",")):
        ix.self_join(args.join_floor, nprobe, k=k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, ids, cnt = ix.self_join(args.join_floor, nprobe, k=k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ip = pairs(ids)
        common = int(torch.isin(ip, dp).sum())
        r = dict(part="ivf_join", n=n, floor=args.join_floor, k=k, nprobe=nprobe, seconds=dt, dense_seconds=dense_s, pairs=int(ip.numel()),
                 dense_pairs=int(dp.numel()), common=common, recall=common / max(1, int(dp.numel())),
                 mean_count=float(cnt.float().mean()), truncated=float((cnt > k).float().mean()))
        emit(r)
        print(f"| {n} | {nprobe} | {dt:.3f} | {dense_s:.3f} | {r['pairs']} | {r['dense_pairs']} | {r['recall']:.4f} | {r['mean_count']:.1f} | "
              f"{100 * r['truncated']:.1f} % |", flush=True)
    ix.close()
    dx.close()
