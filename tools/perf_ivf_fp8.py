#!/usr/bin/env python3
"""Exact IVF search against the IVF fp8 scan + exact re-rank (the table behind DESIGN.md "IVF fp8 scan + exact re-rank").

C5's data (bench.ivf_leg's recipe: rows = one of 4096 centroids + 0.3 N(0,1) in 768 dimensions, nlist 4096 trained on the
device, nprobe 32, k = 10) at --n rows (625 000 = the per-GPU share, 5 000 000 = the whole corpus), for every batch size of
--nq and every refine pool of --refine: whole-call ms and scan + select ms (last_timing(), median and min-max of --reps
rounds after a warm-up, exact and fp8 in rotation), recall@k of the fp8 result against the exact IVF result of the same
index, and the HBM the fp8 copy adds.  One JSON line per point (--json FILE) and a table.
Per-kernel split: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/perf_ivf_fp8.py --n N
--nq 10000 --refine 0 --reps 3` (without --output-format csv no CSV is written).  ivfs_scan_kernel<1> / <16> are the fp16 /
fp8 scans (the <1> instance also runs once per search for the probe selection), then ivfs_select_lists_kernel,
quant_queries_fp8_kernel, fp8_rerank_kernel."""
import argparse
import json
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from mrag_amd.index import IVFFlatIndex, fp8_default_refine

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=625_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--nprobe", type=int, default=32)
ap.add_argument("--nq", default="10000,1000,1")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--refine", default="0,64", help="comma list of fp8 refine pools (0 = the default)")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--json", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(1)
cent = torch.randn(4096, args.dim, device=dev, generator=g)


def draw(m):
    return cent[torch.randint(0, 4096, (m,), device=dev, generator=g)] + 0.3 * torch.randn(m, args.dim, device=dev, generator=g)


ix = IVFFlatIndex(args.dim, args.nlist, fp8_scan=True)
ix.train(draw(100_000), iters=5, seed=1)
for lo in range(0, args.n, 125_000):
    ix.add(draw(min(125_000, args.n - lo)))
nq_max = max(int(x) for x in args.nq.split(","))
qall = draw(nq_max)
torch.cuda.synchronize()
out = open(args.json, "w") if args.json else None


def run_point(nq, rf):
    q = qall[:nq].contiguous()
    kws = {"exact": {}, "fp8": {"precision": "fp8", "refine": rf or None}}
    res = {name: ix.search(q, args.k, args.nprobe, **kw) for name, kw in kws.items()}     # warm-up (and the regroup)
    ts = {name: [] for name in kws}
    for _ in range(args.reps):
        for name, kw in kws.items():
            ix.search(q, args.k, args.nprobe, **kw)
            t = ix.last_timing()
            ts[name].append((t["scan_ms"], t["total_ms"], t["scanned_rows"]))
    refine = ix.last_fp8()["refine"]
    torch.cuda.synchronize()
    ex_ids, f8_ids = res["exact"][1].cpu().numpy(), res["fp8"][1].cpu().numpy()
    hit = sum(len(set(a.tolist()) & set(b.tolist()) - {-1}) for a, b in zip(ex_ids, f8_ids))
    recall = hit / max(int((ex_ids >= 0).sum()), 1)
    row = {"n": len(ix), "dim": args.dim, "nlist": args.nlist, "nprobe": args.nprobe, "nq": nq, "k": args.k, "refine": refine,
           "default_refine": fp8_default_refine(args.k), "recall": recall, "reps": args.reps,
           "scanned_rows": ts["exact"][-1][2],
           "fp8_copy_mb_rows": len(ix) * ((args.dim + 127) // 128 * 128) / 2**20}    # (+ each list's padding to whole 256-row tiles)
    for name, v in ts.items():
        for j, what in enumerate(("scan_ms", "total_ms")):
            x = [t[j] for t in v]
            row[f"{name}_{what}"] = float(np.median(x))
            row[f"{name}_{what}_min"], row[f"{name}_{what}_max"] = float(min(x)), float(max(x))
    print(f"| {len(ix)} | {nq} | {refine} | {row['exact_scan_ms']:.3f} | {row['exact_total_ms']:.3f} "
          f"({row['exact_total_ms_min']:.3f}-{row['exact_total_ms_max']:.3f}) | {row['fp8_scan_ms']:.3f} | {row['fp8_total_ms']:.3f} "
          f"({row['fp8_total_ms_min']:.3f}-{row['fp8_total_ms_max']:.3f}) | {recall:.4f} |", flush=True)
    if out:
        out.write(json.dumps(row) + "\n")
        out.flush()


print(f"| rows | queries | refine | exact scan+select ms | exact total ms (min-max) | fp8 scan+select ms | fp8 total ms (min-max) | recall@{args.k} |")
print("|---|---|---|---|---|---|---|---|")
for nq_ in (int(x) for x in args.nq.split(",")):
    for rf_ in (int(x) for x in args.refine.split(",")):
        run_point(nq_, rf_)
