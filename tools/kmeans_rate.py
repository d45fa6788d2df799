"""Rate of the k-means update (ops.f32_cluster_sums, csrc/kmeans.hip) and of one whole Lloyd step against the same
quantities written with torch in fp64 on the same device:
python tools/kmeans_rate.py [--repeats 5] [--inner 10] [--n 50000] [--dims 256 2048] [--ks 10 100 1000]

Every point is n rows of D floats in K clusters, once with balanced clusters and once with one cluster holding half the
rows (the rest spread evenly), the labels in scrambled order.  Timed forms, the median over `repeats` windows of `inner`
calls each (device events; one warm-up call of every form first, the forms alternating):

  sums          ops.f32_cluster_sums(x, labels, K, d2): the inverted index (torch sort + bincount) and the two kernels
  kernels       the two kernels alone on a prebuilt index
  torch sums    torch.zeros(K, D, fp64).index_add_(0, labels, x.double())
  lloyd         cluster.lloyd_step(x, centroids)
  torch lloyd   norms + x.double() @ c.double().T + argmin + index_add_ + the division

and for each the peak device memory above what the inputs hold.  The rate is n * D * 4 bytes (the set read once) over the
time.  The torch sums are compared with ours before anything is timed (atomics: equal to rounding, not to the bit).
Prints one JSON line per point, then the skewed / balanced time ratios.  The first line names the chunk length of the
library that runs (ops.cluster_block()): EDM_LIB_PATH=<a library built with -DEDM_CLUSTER_BLOCK=B -DCLUSTER_ROWS=U> gives
the figures of another chunk length or of other rows in flight, the chunk tables following the library."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinyedm_amd import _lib, cluster, ops  # noqa: E402
from tinyedm_amd.ops import _p, _stream  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--repeats", type=int, default=5)
p.add_argument("--inner", type=int, default=10)
p.add_argument("--n", type=int, default=50000)
p.add_argument("--dims", type=int, nargs="+", default=[256, 2048])
p.add_argument("--ks", type=int, nargs="+", default=[10, 100, 1000])
args = p.parse_args()
if not torch.cuda.is_available():
    sys.exit("kmeans_rate: needs a GPU (a CPU run measures nothing)")
dev = torch.device("cuda:0")


def make_labels(n, K, skewed, g):
    if skewed:
        half = n // 2
        rest = torch.arange(n - half) % max(K - 1, 1) + (1 if K > 1 else 0)
        labels = torch.cat([torch.zeros(half, dtype=torch.int64), rest])
    else:
        labels = torch.arange(n) % K
    return labels[torch.randperm(n, generator=g)].to(dev)


def kernels_only(x, index, d2, K):
    members, starts, first, chunk_cluster = index
    n, D = x.shape
    chunks = chunk_cluster.shape[0]
    partial = torch.empty(chunks, D, dtype=torch.float64, device=dev)
    partial_d2 = torch.empty(chunks, dtype=torch.float64, device=dev)
    sums = torch.empty(K, D, dtype=torch.float64, device=dev)
    d2sums = torch.empty(K, dtype=torch.float64, device=dev)
    _lib.call("edm_f32_cluster_sums_partial", _p(x), _p(members), _p(starts), _p(first), _p(chunk_cluster), _p(d2), n, D, K,
              chunks, _p(partial), _p(partial_d2), _stream())
    _lib.call("edm_f32_cluster_sums_finish", _p(partial), _p(partial_d2), _p(first), D, K, _p(sums), _p(d2sums), _stream())
    return sums, d2sums


def torch_sums(x, labels, K):
    return torch.zeros(K, x.shape[1], dtype=torch.float64, device=dev).index_add_(0, labels, x.double())


def torch_lloyd(x, c):
    x64, c64 = x.double(), c.double()
    d = (x64 * x64).sum(1, keepdim=True) + (c64 * c64).sum(1)[None, :] - 2.0 * (x64 @ c64.T)
    d2, labels = d.clamp_(min=0.0).min(dim=1)
    K = c.shape[0]
    sums = torch.zeros(K, x.shape[1], dtype=torch.float64, device=dev).index_add_(0, labels, x64)
    counts = torch.bincount(labels, minlength=K)
    inertia = torch.zeros(K, dtype=torch.float64, device=dev).index_add_(0, labels, d2)
    return labels, d2, (sums / counts.clamp(min=1).unsqueeze(1)).float(), counts, inertia


def measure(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.inner):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return a.elapsed_time(b) / args.inner, peak


print(json.dumps({"device": torch.cuda.get_device_name(0), "n": args.n, "cluster_block": ops.cluster_block(),
                  "repeats": args.repeats, "inner": args.inner}), flush=True)
g = torch.Generator().manual_seed(args.n)
ratios = {}
for D in args.dims:
    x = torch.randn(args.n, D, generator=g).to(dev)
    for K in args.ks:
        for skewed in (False, True):
            labels = make_labels(args.n, K, skewed, g)
            d2 = torch.rand(args.n, generator=g, dtype=torch.float64).to(dev)
            centroids = x[torch.randperm(args.n, generator=g)[:K].to(dev)].contiguous()
            index = ops._cluster_index(labels, K, torch.bincount(labels, minlength=K).cpu().numpy())
            cases = {"sums": lambda: ops.f32_cluster_sums(x, labels, K, d2),
                     "kernels": lambda: kernels_only(x, index, d2, K),
                     "torch_sums": lambda: torch_sums(x, labels, K),
                     "lloyd": lambda: cluster.lloyd_step(x, centroids),
                     "torch_lloyd": lambda: torch_lloyd(x, centroids)}
            ours, theirs = cases["sums"]()[0], cases["torch_sums"]()       # the warm-up is the comparison
            rel = float((ours - theirs).abs().max() / theirs.abs().max())
            assert torch.equal(cases["kernels"]()[0], ours)
            same_labels = float((cases["lloyd"]()[0] == cases["torch_lloyd"]()[0]).double().mean())
            del ours, theirs
            ms, peak = {c: [] for c in cases}, {c: 0 for c in cases}
            for _ in range(args.repeats):
                for c, fn in cases.items():
                    t, m = measure(fn)
                    ms[c].append(t)
                    peak[c] = max(peak[c], m)
            med = {c: statistics.median(v) for c, v in ms.items()}
            nbytes = 4.0 * args.n * D
            row = {"D": D, "K": K, "skewed": skewed, "chunks": int(index[3].shape[0]), "max_rel_diff_vs_torch": rel,
                   "equal_label_share": same_labels}
            for c in cases:
                row[c + "_ms"] = round(med[c], 4)
                row[c + "_ms_all"] = [round(v, 4) for v in ms[c]]
                row[c + "_peak_extra_mib"] = round(peak[c] / 2 ** 20, 1)
            for c in ("sums", "kernels", "torch_sums"):
                row[c + "_tb_per_s"] = round(nbytes / (med[c] * 1e-3) / 1e12, 3)
            row["torch_sums_over_sums"] = round(med["torch_sums"] / med["sums"], 3)
            row["torch_lloyd_over_lloyd"] = round(med["torch_lloyd"] / med["lloyd"], 3)
            ratios.setdefault((D, K), {})[skewed] = (med["kernels"], med["sums"])
            print(json.dumps(row), flush=True)
print(json.dumps({"skewed_over_balanced": [
    {"D": D, "K": K, "kernels": round(r[True][0] / r[False][0], 3), "sums": round(r[True][1] / r[False][1], 3)}
    for (D, K), r in ratios.items()]}), flush=True)
