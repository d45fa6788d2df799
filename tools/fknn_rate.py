"""Rate of the feature-space search (ops.f32_knn, csrc/neighbors_f32.hip) against the same quantities written with torch
in fp64 on the same device -- chunked q.double() @ r.double().T plus the norms and topk:
python tools/fknn_rate.py [--repeats 3] [--n 50000] [--queries 10000] [--dim 2048] [--k 5] [--mfma_bin PATH | --mfma_tflops X]

Two points: an n x n x dim self-search (exclude_self) at k, and `queries` rows against the same n references.  For each
form the median time over `repeats` runs (after one warm-up, the forms alternating) and the peak device memory above
what the inputs hold.  The library's share of the bare fp64 MFMA rate is quoted on the FLOPs it executes (whole 64 x 64
tiles and whole 32-element K steps, the norm tiles included); the bare rate comes from running the binary built from
tools/mfma_shape/mfma_f64.hip (--mfma_bin) or is given (--mfma_tflops).  The two forms are compared before they are timed:
the share of equal neighbour indices and the largest relative distance difference (the torch form rounds differently).
Prints one JSON line per point."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinyedm_amd import ops  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--repeats", type=int, default=3)
p.add_argument("--n", type=int, default=50000)
p.add_argument("--queries", type=int, default=10000)
p.add_argument("--dim", type=int, default=2048)
p.add_argument("--k", type=int, default=5)
p.add_argument("--torch_chunk", type=int, default=4096, help="queries per fp64 matmul of the torch form")
p.add_argument("--mfma_bin", type=str, default=None)
p.add_argument("--mfma_tflops", type=float, default=None)
args = p.parse_args()
dev = torch.device("cuda:0")

bare = args.mfma_tflops
if args.mfma_bin is not None:
    out = subprocess.run([args.mfma_bin], capture_output=True, text=True, timeout=300, check=True).stdout
    bare = float(json.loads(out.strip().splitlines()[-1])["tflops"])


def torch_form(q, r64, rn, k, exclude_self, chunk):
    """(dist fp64 [Q, k], idx int64 [Q, k]) by the expansion in fp64; r64 and rn are made once by the caller"""
    dist, idx = [], []
    for a in range(0, q.shape[0], chunk):
        q64 = q[a:a + chunk].double()
        d = (q64 * q64).sum(1, keepdim=True) + rn[None, :] - 2.0 * (q64 @ r64.T)
        d.clamp_(min=0.0)
        if exclude_self:
            rows = torch.arange(d.shape[0], device=d.device)
            d[rows, rows + a] = float("inf")
        v, i = torch.topk(d, k, dim=1, largest=False)
        dist.append(v)
        idx.append(i)
    return torch.cat(dist), torch.cat(idx)


def torch_whole(q, r, k, exclude_self):
    r64 = r.double()
    return torch_form(q, r64, (r64 * r64).sum(1), k, exclude_self, args.torch_chunk)


def measure(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return a.elapsed_time(b), peak


def executed_flop(Q, R, D, same):
    tiles = lambda n: (n + 63) // 64                                     # noqa: E731
    steps = (D + 31) // 32 * 32
    norm_tiles = tiles(Q) if same else tiles(Q) + tiles(R)
    return 2.0 * 64 * 64 * steps * (tiles(Q) * tiles(R) + norm_tiles)


g = torch.Generator().manual_seed(args.n + args.dim)
refs = torch.randn(args.n, args.dim, generator=g).to(dev)
queries = torch.randn(args.queries, args.dim, generator=g).to(dev)
for name, q, excl in (("self", refs, True), ("queries", queries, False)):
    Q, R, D, k = q.shape[0], refs.shape[0], args.dim, args.k
    cases = {"f32_knn": lambda: ops.f32_knn(q, refs, k, exclude_self=excl),
             "torch fp64": lambda: torch_whole(q, refs, k, excl)}
    ours, theirs = cases["f32_knn"](), cases["torch fp64"]()              # the warm-up is the comparison
    same_idx = float((ours[1] == theirs[1]).double().mean())
    rel = float(((ours[0] - theirs[0]).abs() / theirs[0].abs().clamp_min(1e-300)).max())
    del ours, theirs
    ms, peak = {c: [] for c in cases}, {c: 0 for c in cases}
    for _ in range(args.repeats):
        for c, fn in cases.items():
            t, m = measure(fn)
            ms[c].append(t)
            peak[c] = max(peak[c], m)
    med = {c: statistics.median(v) for c, v in ms.items()}
    flop = executed_flop(Q, R, D, q is refs)
    rate = flop / (med["f32_knn"] * 1e-3) / 1e12
    print(json.dumps({
        "point": name, "Q": Q, "R": R, "D": D, "k": k, "repeats": args.repeats, "splits": ops.f32_knn_splits(Q, R),
        "f32_knn_ms": round(med["f32_knn"], 2), "f32_knn_ms_all": [round(v, 2) for v in ms["f32_knn"]],
        "torch_fp64_ms": round(med["torch fp64"], 2), "torch_fp64_ms_all": [round(v, 2) for v in ms["torch fp64"]],
        "torch_over_ours": round(med["torch fp64"] / med["f32_knn"], 3),
        "f32_knn_peak_extra_mib": round(peak["f32_knn"] / 2 ** 20, 1), "torch_fp64_peak_extra_mib": round(peak["torch fp64"] / 2 ** 20, 1),
        "executed_tflop": round(flop / 1e12, 3), "nominal_tflop": round(2.0 * Q * R * D / 1e12, 3),
        "f32_knn_tflops_executed": round(rate, 2), "bare_mfma_tflops": bare,
        "share_of_bare_mfma": None if not bare else round(rate / bare, 3),
        "equal_idx_share": same_idx, "max_rel_dist_diff": rel}), flush=True)
