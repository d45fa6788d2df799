"""conv_in's input gradient (ops.conv_in_dgrad, csrc/conv_in_dgrad.hip) against the HBM time of its one large operand.

The kernel reads gy (bf16 NHWC [B, H, W, C0]) once and writes an image-sized fp32 tensor: its floor is the read of gy at the
HBM peak.  The timed loop walks a ring of gy buffers larger than the last-level cache, so every launch reads from HBM.

    python tools/microbench_convin_dgrad.py [--batch 64 512] [--size 32] [--c0 128] [--cimg 3] [--iters 200]

Prints one JSON line per batch: the time per launch (device events around the loop), the HBM time of gy at the peak, and
their ratio.  At batch 64 the kernel is about as short as the host takes to enqueue it, so that figure is an upper bound of
the kernel time; the larger batch is the one to read the streaming rate from."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinyedm_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s (MI355X data sheet)
RING_BYTES = 768 << 20      # beyond the 256 MiB last-level cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--c0", type=int, default=128)
    ap.add_argument("--cimg", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("microbench_convin_dgrad: needs a GPU")
    for B in a.batch:
        bench(a, B)


def bench(a, B):
    dev = "cuda"
    H, C0, Cimg = a.size, a.c0, a.cimg
    gy_bytes = B * H * H * C0 * 2
    ring = max(2, RING_BYTES // gy_bytes)
    gys = [torch.randn(B, H, H, C0, device=dev).to(torch.bfloat16) for _ in range(ring)]
    pack = torch.zeros(C0, ops.conv_in_dgrad_pack_cols(Cimg), device=dev)
    pack[:, :9 * Cimg] = torch.randn(C0, 9 * Cimg, device=dev).to(torch.bfloat16).float() / 8
    gD = torch.randn(B, Cimg, H, H, device=dev)
    sigma = torch.rand(B, device=dev) + 0.1
    out = {}
    for name, gd in (("with_gD", gD), ("without_gD", None)):
        for k in range(min(ring, 8)):
            ops.conv_in_dgrad(gys[k], pack, gd, sigma, 0.5)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for k in range(a.iters):
            ops.conv_in_dgrad(gys[k % ring], pack, gd, sigma, 0.5)
        e.record()
        torch.cuda.synchronize()
        out[name] = s.elapsed_time(e) / a.iters * 1e3
    hbm_us = gy_bytes / HBM_PEAK * 1e6
    print(json.dumps({"shape": [B, H, H, C0], "cimg": Cimg, "gy_bytes": gy_bytes, "ring_buffers": ring,
                      "us_with_gD": round(out["with_gD"], 2), "us_without_gD": round(out["without_gD"], 2),
                      "hbm_us_of_gy_at_8TBs": round(hbm_us, 2), "ratio_to_hbm_time": round(out["with_gD"] / hbm_us, 2),
                      "fma_per_launch": B * H * H * C0 * 9 * Cimg}))


if __name__ == "__main__":
    main()
