"""Ball membership counts (csrc/neighbors.hip k_u8_ball_count, ops.u8_ball_count) against the top-1 search of the same build
on the same arrays (ops.u8_knn(k=1): the same distance tile with the top-k epilogue) and against what a user can do without
either: chunked fp32 torch.matmul on the shifted values, a compare with the radii and a sum, distance blocks under 1 GB.
    python tools/prdc_rate.py [--sizes 10000x50000 50000x50000] [--D 3072] [--out prdc_rate.json]
Protocol of tools/microbench_knn.py: all three are warmed up, then timed in alternating rounds in one process; a round is a
batch of calls between two device events, sized from the warm-up to last about --window seconds.  Data: random uint8; the
radius of a reference is the exact distance of a randomly chosen query to it, so about half of all pairs are inside and
every reference has a query exactly on its sphere.  Prints, per size: the three times per call (median and min over the
rounds; whole calls: norms + kernel + the sum / merge), ball count over top-1, and how many of the fp32 counts differ from the
exact ones."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from microbench_knn import BLOCK_BYTES, alternate  # noqa: E402
from tinyedm_amd import ops  # noqa: E402

dev = "cuda"
MARGIN = 1.03       # ball count no slower than top-1 within 3 %: ten times microbench_knn's run-to-run spread of 0.3 %


def exact_radii(q, r, g):
    """int64 [R]: d2 of a randomly chosen query to each reference, in integers, a block of references at a time"""
    pick = torch.randint(0, q.shape[0], (r.shape[0],), device=dev, generator=g)
    out = torch.empty(r.shape[0], dtype=torch.int64, device=dev)
    for a in range(0, r.shape[0], 4096):
        d = q[pick[a:a + 4096]].to(torch.int32) - r[a:a + 4096].to(torch.int32)
        out[a:a + 4096] = (d * d).sum(1, dtype=torch.int64)
    return out


def baseline(q, r, radii):
    """fp32 on the shifted values: |q|^2 + |r|^2 - 2 q.r <= radius, one block of queries at a time"""
    rf = r.view(r.shape[0], -1).float() - 128.0
    rn = (rf * rf).sum(1)
    rad = radii.float()
    rows = max(1, min(q.shape[0], (BLOCK_BYTES - 1) // (4 * r.shape[0])))
    out = []
    for a in range(0, q.shape[0], rows):
        qf = q[a:a + rows].view(-1, rf.shape[1]).float() - 128.0
        d = (qf * qf).sum(1)[:, None] + rn[None, :] - 2.0 * torch.matmul(qf, rf.t())
        out.append((d <= rad[None, :]).sum(1))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["10000x50000", "50000x50000"])
    ap.add_argument("--D", type=int, default=3072)
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
        radii = exact_radii(q, r, g)
        (c, c_med, c_min, c_n), (_, t_med, t_min, t_n), (b, b_med, b_min, b_n) = alternate(
            [lambda: ops.u8_ball_count(q, r, radii), lambda: ops.u8_knn(q, r, 1), lambda: baseline(q, r, radii)],
            args.rounds, args.window)
        res = {"Q": Q, "R": R, "D": args.D, "splits": ops.u8_knn_splits(Q, R),
               "ball_count_s_median": c_med, "ball_count_s_min": c_min, "knn1_s_median": t_med, "knn1_s_min": t_min,
               "baseline_s_median": b_med, "baseline_s_min": b_min, "rounds": args.rounds,
               "calls_per_round": [c_n, t_n, b_n], "int8_tops": 2.0 * Q * R * args.D / c_med / 1e12,
               "ball_count_over_knn1": c_med / t_med, "within_margin": bool(c_med <= MARGIN * t_med),
               "speedup_over_baseline": b_med / c_med, "baseline_counts_wrong": int((b != c).sum()),
               "mean_count": float(c.double().mean()), "device": torch.cuda.get_device_name(0)}
        results.append(res)
        print(f"{Q} x {R} x {args.D}, splits={res['splits']}: u8_ball_count {c_med * 1e3:.2f} ms (min {c_min * 1e3:.2f})  "
              f"{res['int8_tops']:.1f} int8 TOP/s   u8_knn(k=1) {t_med * 1e3:.2f} ms (min {t_min * 1e3:.2f})  -> ball count / "
              f"top-1 = {res['ball_count_over_knn1']:.3f} ({'within' if res['within_margin'] else 'OUTSIDE'} the 3 % margin)   "
              f"fp32 matmul + compare + sum {b_med * 1e3:.2f} ms (min {b_min * 1e3:.2f})  -> {res['speedup_over_baseline']:.2f}x   "
              f"fp32 counts differ from exact in {res['baseline_counts_wrong']} of {Q} rows (mean count {res['mean_count']:.0f})",
              flush=True)
        del r, q, radii, c, b
        torch.cuda.empty_cache()
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
