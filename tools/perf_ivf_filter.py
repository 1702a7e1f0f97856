#!/usr/bin/env python3
"""Filtered IVF search cost against selectivity: unfiltered, forced P (probe), forced E (exact) and AUTO (the table behind
DESIGN.md "Filtered IVF search").

10 000 queries x 625 k x 768 fp16 (clustered rows, the C5 share of one GPU), nlist 4096 (k-means on the device), nprobe 32,
k = 10, selectivity in {1e-4 .. 1.0}, two kinds of allow-set: uniform random rows, and list-correlated (whole lists drawn at
random until the allowed rows reach the selectivity: tenant / title filters).  Whole-search device ms (last_timing()
["total_ms"], median of 5 after a warm-up, the filtered variants in rotation), the path AUTO took, and recall@10 of P
against E (E is exact).  Host masks, so AUTO needs no read-back.  One JSON line per point (--json FILE) and a table."""
import argparse
import json
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from mrag_amd.index import IVFFlatIndex

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=625_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--nq", default="10000")
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--nprobe", type=int, default=32)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--sel", default="1e-4,1e-3,1e-2,0.05,0.1,0.25,1.0")
ap.add_argument("--kinds", default="uniform,lists")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

g = torch.Generator(device="cuda").manual_seed(1)
topics = torch.randn(4096, args.dim, device="cuda", generator=g)


def clustered(m):
    which = torch.randint(0, topics.shape[0], (m,), device="cuda", generator=g)
    return topics[which] + 0.3 * torch.randn(m, args.dim, device="cuda", generator=g)


ix = IVFFlatIndex(args.dim, args.nlist)
ix.train(clustered(200_000), iters=4, seed=3)
for lo in range(0, args.n, 125_000):
    ix.add(clustered(min(125_000, args.n - lo)))
assign = ix.assignments()
rng = np.random.default_rng(2)
u = rng.random(args.n)
list_order = rng.permutation(args.nlist)
list_rows = [np.flatnonzero(assign == l) for l in range(args.nlist)]
out = open(args.json, "w") if args.json else None


def lists_mask(sel):
    """whole lists in a random order until sel * n rows are allowed (the last list cut)"""
    want = max(1, int(round(sel * args.n)))
    mask = np.zeros(args.n, dtype=bool)
    have = 0
    for l in list_order:
        r = list_rows[l][:want - have]
        mask[r] = True
        have += r.size
        if have >= want:
            break
    return mask


def timed(q, **kw):
    ix.search(q, args.k, args.nprobe, **kw)
    ts = []
    for _ in range(args.reps):
        ix.search(q, args.k, args.nprobe, **kw)
        ts.append(ix.last_timing()["total_ms"])
    torch.cuda.synchronize()
    return float(np.median(ts))


def timed_paths(q, mask):
    kws = {p: dict(allow=mask, filter_path=p) for p in ("probe", "exact", "auto")}
    res = {p: ix.search(q, args.k, args.nprobe, **kw) for p, kw in kws.items()}
    auto_path = ix.last_filter()["path"]
    ts = {p: [] for p in kws}
    for _ in range(args.reps):
        for p, kw in kws.items():
            ix.search(q, args.k, args.nprobe, **kw)
            ts[p].append(ix.last_timing()["total_ms"])
    torch.cuda.synchronize()
    return {p: float(np.median(v)) for p, v in ts.items()}, auto_path, res


def recall(ids_p, ids_e):
    ids_p, ids_e = ids_p.cpu().numpy(), ids_e.cpu().numpy()
    hit = tot = 0
    for a, b in zip(ids_p, ids_e):
        b = b[b >= 0]
        tot += b.size
        hit += np.isin(b, a).sum()
    return hit / tot if tot else 1.0


print(f"n {args.n} x {args.dim}, nlist {args.nlist}, nprobe {args.nprobe}, k {args.k}")
print("| queries | mask | selectivity | unfiltered ms | P ms | E ms | auto ms (path) | P recall@k vs E | P hits / k |")
print("|---:|---|---:|---:|---:|---:|---|---:|---:|")
for nq in (int(x) for x in args.nq.split(",")):
    q = clustered(nq)
    base = timed(q)
    for kind in args.kinds.split(","):
        for sel in (float(x) for x in args.sel.split(",")):
            mask = u < sel if kind == "uniform" else lists_mask(sel)
            r = {"nq": nq, "n": args.n, "dim": args.dim, "nlist": args.nlist, "nprobe": args.nprobe, "k": args.k, "mask": kind,
                 "sel": sel, "allowed": int(mask.sum()), "unfiltered_ms": base}
            t, r["auto_path"], res = timed_paths(q, mask)
            for p, v in t.items():
                r[f"{p}_ms"] = v
            r["auto_over_best"] = t["auto"] / min(t["probe"], t["exact"])
            r["probe_recall"] = recall(res["probe"][1], res["exact"][1])
            r["probe_hits"] = float((res["probe"][1] >= 0).float().mean().item())
            print(f"| {nq} | {kind} | {sel:g} | {base:.3f} | {t['probe']:.3f} | {t['exact']:.3f} | {t['auto']:.3f} ({r['auto_path']}) | "
                  f"{r['probe_recall']:.3f} | {r['probe_hits']:.3f} |", flush=True)
            if out:
                out.write(json.dumps(r) + "\n")
                out.flush()
