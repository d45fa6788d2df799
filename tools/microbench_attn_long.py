"""Time the tiled-softmax attention kernels (csrc/attention_long.hip) on maps above 256 tokens, and at N = 256 next to the
kernels of attention.hip: python tools/microbench_attn_long.py
TF/s from the FLOP counts ops._prof is given: 4 B N^2 C forward, 14 B N^2 C backward."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinyedm_amd import ops  # noqa: E402


def _time(fn, window_ms=300.0, repeats=3):
    """median and spread (us per call) of `repeats` timed windows of about window_ms each, after a warm-up"""
    fn()
    torch.cuda.synchronize()

    def window(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    iters = max(5, int(window_ms * 1e3 / window(5)))
    t = sorted(window(iters) for _ in range(repeats))
    return t[len(t) // 2], t[0], t[-1]


def run(B, H, W, C, heads, short=False):
    qkv = torch.randn(B, H, W, 3 * C, device="cuda").to(torch.bfloat16)
    gy = torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
    N = H * W
    y, stat = ops.attention_long_fwd(qkv, heads)
    kinds = [("long", lambda: ops.attention_long_fwd(qkv, heads), lambda: ops.attention_long_bwd(qkv, y, gy, stat, heads))]
    if short:
        kinds.append(("short", lambda: ops.attention_fwd(qkv, heads), lambda: ops.attention_bwd(qkv, y, gy, heads)))
    for kind, fwd, bwd in kinds:
        (tf, f0, f1), (tb, b0, b1) = _time(fwd), _time(bwd)
        print(f"B={B} {H}x{W} C={C} heads={heads} {kind:5s}: fwd {tf:8.1f} us [{f0:.1f}..{f1:.1f}] "
              f"({4.0 * B * N * N * C / tf / 1e6:6.1f} TF/s)  bwd {tb:8.1f} us [{b0:.1f}..{b1:.1f}] "
              f"({14.0 * B * N * N * C / tb / 1e6:6.1f} TF/s)", flush=True)


if __name__ == "__main__":
    run(128, 32, 32, 256, 4)
    run(16, 64, 64, 192, 1)
    run(128, 16, 16, 256, 4, short=True)
