#!/usr/bin/env python3
"""Filtered search cost against selectivity, both paths forced and AUTO (the table behind DESIGN.md "Filtered search").

{1, 1 000, 10 000} queries x 1M x 768 fp16, k in {10, 200}, selectivity in {1e-4 .. 1.0}: whole-search device ms
(last_timing_ms()[1], median of 5 after a warm-up, the three filtered variants in rotation) of the unfiltered search, forced mask, forced compact and AUTO (with
the path it took).  Host masks, so AUTO needs no read-back.  One JSON line per point (--json FILE, with the search-kernel ms of each, last_timing_ms()[0]) and a table."""
import argparse
import json
import sys
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
ap.add_argument("--sel", default="1e-4,1e-3,1e-2,0.1,0.25,0.5,1.0")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

ix = DenseIndex(args.dim)
g = torch.Generator(device="cuda").manual_seed(1)
for lo in range(0, args.n, 250_000):
    ix.add(torch.randn(min(250_000, args.n - lo), args.dim, device="cuda", generator=g))
rng = np.random.default_rng(2)
u = rng.random(args.n)
out = open(args.json, "w") if args.json else None


def timed(q, k, **kw):
    ix.search(q, k, **kw)
    ts = []
    for _ in range(args.reps):
        ix.search(q, k, **kw)
        ts.append(ix.last_timing_ms())
    torch.cuda.synchronize()
    return float(np.median([t[1] for t in ts])), float(np.median([t[0] for t in ts]))


def timed_paths(q, k, mask):
    """mask / compact / auto measured in rotation (one of each per round), so that clock drift hits all three alike."""
    kws = {p: dict(allow=mask, filter_path=p) for p in ("mask", "compact", "auto")}
    for kw in kws.values():
        ix.search(q, k, **kw)
    ts = {p: [] for p in kws}
    for _ in range(args.reps):
        for p, kw in kws.items():
            ix.search(q, k, **kw)
            ts[p].append(ix.last_timing_ms())
    auto_path = ix.last_filter()["path"]
    torch.cuda.synchronize()
    return {p: (float(np.median([t[1] for t in v])), float(np.median([t[0] for t in v]))) for p, v in ts.items()}, auto_path


print("| queries | k | selectivity | unfiltered ms | mask ms | compact ms | auto ms (path) |")
print("|---:|---:|---:|---:|---:|---:|---|")
for nq in (int(x) for x in args.nq.split(",")):
    q = torch.randn(nq, args.dim, device="cuda", generator=g)
    for k in (int(x) for x in args.k.split(",")):
        base, base_kernel = timed(q, k)
        for sel in (float(x) for x in args.sel.split(",")):
            mask = u < sel
            r = {"nq": nq, "n": args.n, "dim": args.dim, "k": k, "sel": sel, "allowed": int(mask.sum()), "unfiltered_ms": base,
                 "unfiltered_kernel_ms": base_kernel}
            res, r["auto_path"] = timed_paths(q, k, mask)
            for path, (t_all, t_kernel) in res.items():
                r[f"{path}_ms"], r[f"{path}_kernel_ms"] = t_all, t_kernel
            best = min(r["mask_ms"], r["compact_ms"])
            r["auto_over_best"] = r["auto_ms"] / best
            print(f"| {nq} | {k} | {sel:g} | {base:.3f} | {r['mask_ms']:.3f} | {r['compact_ms']:.3f} | "
                  f"{r['auto_ms']:.3f} ({r['auto_path']}) |", flush=True)
            if out:
                out.write(json.dumps(r) + "\n")
                out.flush()
