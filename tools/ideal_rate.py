"""Rate of the ideal denoiser (ops.ideal_denoise, csrc/ideal.hip) against the same mathematics written with torch on the
same device -- fp32 matmul for the logits in the expansion |x|^2 - 2 x.y + |y|^2, softmax, fp32 matmul for the output:
python tools/ideal_rate.py [repeats] [ref_chunk]

Two points: Q = 512 queries against R = 50 000 uint8 references of K = 3072 elements (a CIFAR-10 training set), and
Q = 64 against R = 10 000.  The torch form is handed the normalised fp32 copy of the set (R * K * 4 bytes, built outside
the timed window) and its row norms; the library reads the uint8 rows.  The two are compared on one-hot-free inputs
before they are timed.  Each case is warmed up, then timed with device events over `repeats` runs, the cases alternating;
the median and the min..max spread are printed, and the achieved rate of the two products, 4 Q R K flop per call."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinyedm_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
ref_chunk = int(sys.argv[2]) if len(sys.argv) > 2 else None
K = 3072


def timed(cases, reps, warm=2):
    """name -> list of ms, the cases alternating within each repeat"""
    for fn in cases.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def torch_form(x, sigma, y, yy):
    """D* with torch: fp32 matmul, softmax, matmul"""
    x2 = x.view(x.shape[0], -1)
    inv = 1.0 / (2.0 * sigma * sigma)
    logits = (2.0 * (x2 @ y.t()) - yy[None, :] - (x2 * x2).sum(1, keepdim=True)) * inv[:, None]
    return (torch.softmax(logits, dim=1) @ y).view_as(x)


for Q, R in ((512, 50000), (64, 10000)):
    g = torch.Generator().manual_seed(Q + R)
    # clustered references (32 base images + a perturbation of +-24 grey levels) so that the softmax is not one-hot
    base = torch.randint(40, 216, (32, K), generator=g)
    refs = (base[torch.randint(0, 32, (R,), generator=g)] + torch.randint(-24, 25, (R, K), generator=g)).clamp_(0, 255)
    refs = refs.to(torch.uint8).to(dev).view(R, 3, 32, 32)
    y = (refs.view(R, K).float() / 255.0 - 0.5) / 0.5
    yy = (y * y).sum(1)
    sigma = torch.full((Q,), 4.0, device=dev)
    x = (y[torch.randint(0, R, (Q,), generator=g).to(dev)] + 4.0 * torch.randn(Q, K, generator=g).to(dev)).view(Q, 3, 32, 32)
    x = x.contiguous()
    norms = ops.u8_norms(refs)
    ours = ops.ideal_denoise(x, sigma, refs, norms, ref_chunk=ref_chunk)
    theirs = torch_form(x, sigma, y, yy)
    ops.check_health(dev, "ideal_rate")
    print(f"Q={Q} R={R} K={K}: max |ours - torch| {float((ours[0] - theirs).abs().max()):.3e}, mean effective count "
          f"{float(ours[2].exp().mean()):.1f}", flush=True)
    ms = timed({"ideal_denoise": lambda: ops.ideal_denoise(x, sigma, refs, norms, ref_chunk=ref_chunk),
                "torch fp32": lambda: torch_form(x, sigma, y, yy)}, reps)
    flop = 4.0 * Q * R * K
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"Q={Q} R={R} K={K} {k}: median {med[k]:.3f} ms over {reps} runs (min {min(v):.3f}, max {max(v):.3f}), "
              f"{flop / med[k] * 1e-9:.1f} TF/s of the two products", flush=True)
    print(f"Q={Q} R={R} K={K}: torch fp32 : ideal_denoise = {med['torch fp32'] / med['ideal_denoise']:.2f}", flush=True)
    del refs, y, yy, x, ours, theirs
    torch.cuda.empty_cache()
