#!/usr/bin/env python3
"""Exact search against the fp8 scan + exact re-rank (the table behind DESIGN.md "fp8 scan + exact re-rank").

{10 000, 1} queries x 1M x 768 fp16 on a clustered corpus (rows = one of 4096 centroids + 0.3 N(0,1), queries = a random
row + 0.1 N(0,1), the oracle's make_clustered recipe drawn on the device), k = 10, default refine: candidate-kernel ms and
whole-call ms (last_timing_ms(), median of --reps after a warm-up, exact and fp8 in rotation), recall@10 of the fp8
result against the exact search on the same GPU, and the HBM the fp8 copy adds.  One JSON line per point
(--json FILE) and a table."""
import argparse
import json
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from mrag_amd.index import DenseIndex, fp8_default_refine

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--nq", default="10000,1")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--refine", default="0", help="comma list of fp8 refine pools (0 = the default)")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--json", default=None)
args = ap.parse_args()

g = torch.Generator(device="cuda").manual_seed(7)
cent = torch.randn(4096, args.dim, device="cuda", generator=g)
ix = DenseIndex(args.dim, fp8_scan=True)
ix.reserve(args.n)
rows = torch.empty(args.n, args.dim, device="cuda")
for lo in range(0, args.n, 250_000):
    m = min(250_000, args.n - lo)
    which = torch.randint(0, 4096, (m,), device="cuda", generator=g)
    rows[lo:lo + m] = cent[which] + 0.3 * torch.randn(m, args.dim, device="cuda", generator=g)
    ix.add(rows[lo:lo + m])
nq_max = max(int(x) for x in args.nq.split(","))
pick = torch.randint(0, args.n, (nq_max,), device="cuda", generator=g)
qall = rows[pick] + 0.1 * torch.randn(nq_max, args.dim, device="cuda", generator=g)
del rows
torch.cuda.synchronize()
extra_mb = len(ix) * ((args.dim + 127) // 128 * 128) / 2**20     # fp8 copy of the stored rows (capacity = rows here)
out = open(args.json, "w") if args.json else None



def run_point(nq, rf):
    q = qall[:nq].contiguous()
    kws = {"exact": {}, "fp8": {"precision": "fp8", "refine": rf or None}}
    res = {}
    for name, kw in kws.items():
        res[name] = ix.search(q, args.k, **kw)
    ts = {name: [] for name in kws}
    for _ in range(args.reps):
        for name, kw in kws.items():
            ix.search(q, args.k, **kw)
            ts[name].append(ix.last_timing_ms())
    info = ix.last_fp8()
    torch.cuda.synchronize()
    ex_ids = res["exact"][1].cpu().numpy()
    f8_ids = res["fp8"][1].cpu().numpy()
    hit = sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(ex_ids, f8_ids))
    recall = hit / ex_ids.size
    med = {name: (float(np.median([t[0] for t in v])), float(np.median([t[1] for t in v]))) for name, v in ts.items()}
    row = {"nq": nq, "n": len(ix), "dim": args.dim, "k": args.k, "refine": info["refine"], "regime": info["regime"],
           "exact_kernel_ms": med["exact"][0], "exact_total_ms": med["exact"][1],
           "fp8_kernel_ms": med["fp8"][0], "fp8_total_ms": med["fp8"][1], "recall": recall, "fp8_copy_mb": extra_mb,
           "default_refine": fp8_default_refine(args.k)}
    print(f"| {nq} | {med['exact'][0]:.3f} | {med['exact'][1]:.3f} | {med['fp8'][0]:.3f} | {med['fp8'][1]:.3f} | "
          f"{recall:.4f} | {info['refine']} | {info['regime']} | {extra_mb:.0f} |", flush=True)
    if out:
        out.write(json.dumps(row) + "\n")
        out.flush()


print(f"| queries | exact kernel ms | exact total ms | fp8 kernel ms | fp8 total ms | recall@{args.k} | refine | regime | fp8 copy MB |")
print("|---|---|---|---|---|---|---|---|---|")
for nq_ in (int(x) for x in args.nq.split(",")):
    for rf_ in (int(x) for x in args.refine.split(",")):
        run_point(nq_, rf_)
