"""Exact uint8 nearest neighbours (csrc/neighbors.hip, ops.u8_knn) against what a user can do without it on the same device
in the same process: chunked fp32 torch.matmul on the shifted values + torch.topk, distance blocks under 1 GB.
    python tools/microbench_knn.py [--sizes 10000x50000 50000x50000] [--D 3072] [--k 5] [--out knn.json]
Both are warmed up, then timed in alternating rounds in one process: a round is a batch of calls between two device events,
sized from the warm-up to last about --window seconds, first u8_knn, then the baseline.  Prints, per size: both times per
call (median and min over the rounds), the achieved int8 TOP/s of the whole u8_knn call (norms + search + merge + the int64
conversion; 2 Q R D operations) and that whole-call rate's share of the i8 MFMA peak (2 x the 2.5 PF dense bf16 peak; not a
kernel's share: that needs a kernel trace), and how many of the baseline's top-1 answers differ from the exact ones."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinyedm_amd import ops  # noqa: E402

dev = "cuda"
I8_PEAK = 5.0e15            # dense int8 MFMA operations / s: twice the bf16 rate per clock
BLOCK_BYTES = 1 << 30


def batch(fn, n):
    """seconds per call of n back-to-back calls between two device events"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    return out, s.elapsed_time(e) * 1e-3 / n


def alternate(fns, rounds, window):
    """[(last result, median s, min s, calls per round)] of each fn, timed in alternating rounds after a warm-up"""
    calls = []
    for fn in fns:
        batch(fn, 1)
        calls.append(max(1, math.ceil(window / batch(fn, 2)[1])))
    times, outs = [[] for _ in fns], [None] * len(fns)
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            outs[i], t = batch(fn, calls[i])
            times[i].append(t)
    return [(outs[i], statistics.median(times[i]), min(times[i]), calls[i]) for i in range(len(fns))]


def baseline(q, r, k):
    """fp32 on the shifted values: |q|^2 + |r|^2 - 2 q.r, one block of queries at a time"""
    rf = r.view(r.shape[0], -1).float() - 128.0
    rn = (rf * rf).sum(1)
    rows = max(1, min(q.shape[0], (BLOCK_BYTES - 1) // (4 * r.shape[0])))
    dist, idx = [], []
    for a in range(0, q.shape[0], rows):
        qf = q[a:a + rows].view(-1, rf.shape[1]).float() - 128.0
        d = (qf * qf).sum(1)[:, None] + rn[None, :] - 2.0 * torch.matmul(qf, rf.t())
        v, i = torch.topk(d, k, dim=1, largest=False)
        dist.append(v)
        idx.append(i)
    return torch.cat(dist), torch.cat(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["10000x50000", "50000x50000"])
    ap.add_argument("--D", type=int, default=3072)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed batch")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    g = torch.Generator(device=dev).manual_seed(0)
    results = []
    for size in args.sizes:
        Q, R = (int(v) for v in size.split("x"))
        r = torch.randint(0, 256, (R, args.D), dtype=torch.uint8, device=dev, generator=g)
        q = torch.randint(0, 256, (Q, args.D), dtype=torch.uint8, device=dev, generator=g)
        ((d, i), t_med, t_min, t_n), ((bd, bi), b_med, b_min, b_n) = alternate(
            [lambda: ops.u8_knn(q, r, args.k), lambda: baseline(q, r, args.k)], args.rounds, args.window)
        work = 2.0 * Q * R * args.D
        res = {"Q": Q, "R": R, "D": args.D, "k": args.k, "splits": ops.u8_knn_splits(Q, R),
               "knn_s_median": t_med, "knn_s_min": t_min, "baseline_s_median": b_med, "baseline_s_min": b_min,
               "rounds": args.rounds, "knn_calls_per_round": t_n, "baseline_calls_per_round": b_n,
               "int8_tops": work / t_med / 1e12, "share_of_i8_peak": work / t_med / I8_PEAK,
               "speedup": b_med / t_med, "baseline_top1_wrong": int((bi[:, 0] != i[:, 0]).sum()),
               "baseline_topk_wrong_rows": int((bi != i).any(1).sum()), "device": torch.cuda.get_device_name(0)}
        results.append(res)
        print(f"{Q} x {R} x {args.D}, k={args.k}, splits={res['splits']}: u8_knn {t_med * 1e3:.2f} ms (min {t_min * 1e3:.2f})  "
              f"{res['int8_tops']:.1f} int8 TOP/s = {100 * res['share_of_i8_peak']:.1f} % of the i8 MFMA peak   "
              f"fp32 matmul + topk {b_med * 1e3:.2f} ms (min {b_min * 1e3:.2f})  -> {res['speedup']:.2f}x   "
              f"baseline top-1 differs from exact in {res['baseline_top1_wrong']} of {Q} rows", flush=True)
        del r, q, d, i, bd, bi
        torch.cuda.empty_cache()
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
