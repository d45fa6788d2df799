"""The gathers of the resident image loaders against each other (csrc/data.hip) at the CIFAR-10 batch: u8_gather_normalize,
u8_gather_augment_normalize (exact ops) and u8_gather_augment_warp_normalize (exact + continuous ops: 2x up, warp, 2x down).
    python tools/microbench_augment.py [--B 128] [--shape 3x32x32] [--p 0.12 1.0] [--step-ms 12.4] [--out augment.json]
All are warmed up, then timed in alternating rounds in one process: a round is a batch of back-to-back calls between two
device events, sized from the warm-up to last about --window seconds.  Prints, per probability p: microseconds per call
(median and min over the rounds) and the warp gather's share of a training step of --step-ms milliseconds (the aim: under 1 %
of the 12.4 ms step of BENCH_r06.json).  p = 1 warps every sample: the kernel's worst case; 0.12 is cifar10_augment_warp.yaml's."""
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


def batch(fn, n):
    """seconds per call of n back-to-back calls between two device events"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3 / n


def alternate(fns, rounds, window):
    """[(median s, min s, calls per round)] of each fn, timed in alternating rounds after a warm-up"""
    calls = []
    for fn in fns:
        batch(fn, 3)
        calls.append(max(1, math.ceil(window / batch(fn, 20))))
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            times[i].append(batch(fn, calls[i]))
    return [(statistics.median(t), min(t), calls[i]) for i, t in enumerate(times)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--shape", type=str, default="3x32x32")
    ap.add_argument("--N", type=int, default=50000, help="images in the resident set")
    ap.add_argument("--p", type=float, nargs="+", default=[0.12, 1.0])
    ap.add_argument("--step-ms", type=float, default=12.4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.05, help="seconds of back-to-back calls per timed batch")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    C, H, W = (int(v) for v in args.shape.split("x"))
    g = torch.Generator(device=dev).manual_seed(0)
    data = torch.randint(0, 256, (args.N, C, H, W), dtype=torch.uint8, device=dev, generator=g)
    index = torch.randint(0, args.N, (args.B,), device=dev, generator=g)
    sq = ops.AUGMENT_OPS if H == W else ops.AUGMENT_OPS[:3]
    results = []
    for p in args.p:
        fns = [lambda: ops.u8_gather_normalize(data, index, flip=True, seed=1, epoch=2),
               lambda: ops.u8_gather_augment_normalize(data, index, flip=True, seed=1, epoch=2, p=p, ops=sq),
               lambda: ops.u8_gather_augment_warp_normalize(data, index, flip=True, seed=1, epoch=2, p=p, ops=sq)]
        (g_med, g_min, _), (a_med, a_min, _), (w_med, w_min, w_n) = alternate(fns, args.rounds, args.window)
        _, aug = fns[2]()
        warped = int(aug[:, 6:].any(dim=1).sum())
        res = {"B": args.B, "shape": [C, H, W], "p": p, "warped_samples": warped, "gather_us_median": g_med * 1e6,
               "gather_us_min": g_min * 1e6, "augment_us_median": a_med * 1e6, "augment_us_min": a_min * 1e6,
               "warp_us_median": w_med * 1e6, "warp_us_min": w_min * 1e6, "warp_calls_per_round": w_n, "rounds": args.rounds,
               "step_ms": args.step_ms, "warp_share_of_step": w_med / (args.step_ms * 1e-3),
               "device": torch.cuda.get_device_name(0)}
        results.append(res)
        print(f"B={args.B} {C}x{H}x{W} p={p} ({warped} samples warped): gather {g_med * 1e6:.1f} us (min {g_min * 1e6:.1f})  "
              f"exact ops {a_med * 1e6:.1f} us (min {a_min * 1e6:.1f})  exact + continuous {w_med * 1e6:.1f} us "
              f"(min {w_min * 1e6:.1f}) = {100 * res['warp_share_of_step']:.2f} % of a {args.step_ms} ms step", flush=True)
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
