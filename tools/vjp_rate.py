"""What a vector-Jacobian product of the denoiser costs: tinyedm.input_vjp (eval-mode bf16 forward + dgrad-only backward)
against one bf16 forward under torch.no_grad() and against a full training forward + backward at the same batch.

    python tools/vjp_rate.py [--config cifar10] [--batch 64] [--size 32] [--iters 20]

Prints one JSON line with the three times (ms, device synchronised) and the entry-point launches of each."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinyedm_amd as T  # noqa: E402
from tinyedm_amd import _lib, networks  # noqa: E402
from tinyedm_amd.config import compose, instantiate  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    calls0, t0 = _lib.N_CALLS, time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, (_lib.N_CALLS - calls0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cifar10")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vjp_rate: needs a GPU")
    cfg = compose(a.config, os.path.join(ROOT, "experiments", "conf"))
    networks.manual_seed(cfg.seed)
    torch.manual_seed(cfg.seed)
    model = instantiate(cfg.model).to("cuda")
    with torch.no_grad():
        model.denoiser.gain_out.fill_(0.7)          # (a fresh network has gain_out = 0: J would be c_skip I)
    opt = T.FusedAdam(list(model.parameters()), lr=1e-4)
    opt.zero_grad()
    C = model.denoiser.in_channels
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.batch, C, a.size, a.size, generator=g).cuda()
    sigma = (torch.randn(a.batch, generator=g) * 1.2 - 1.2).exp().cuda()
    labels = torch.randint(0, model.num_classes, (a.batch,), generator=g).cuda() if model.conditional else None
    cot = torch.randn(a.batch, C, a.size, a.size, generator=g).cuda()

    model.eval()

    def forward():
        with torch.no_grad():
            model(x, sigma, labels)

    def vjp():
        T.input_vjp(model, x, sigma, labels, cot)
    fwd_ms, fwd_calls = timed(forward, a.iters)
    vjp_ms, vjp_calls = timed(vjp, a.iters)

    model.train()

    def train():
        opt.zero_grad()
        model(x, sigma, labels).backward(cot)
    train_ms, train_calls = timed(train, a.iters)
    model.eval()
    print(json.dumps({"config": a.config, "batch": a.batch, "size": a.size, "forward_bf16_ms": round(fwd_ms, 3),
                      "input_vjp_ms": round(vjp_ms, 3), "train_fwd_bwd_ms": round(train_ms, 3),
                      "vjp_over_forward": round(vjp_ms / fwd_ms, 2), "vjp_over_train_fwd_bwd": round(vjp_ms / train_ms, 2),
                      "launches": {"forward": fwd_calls, "input_vjp": vjp_calls, "train_fwd_bwd": train_calls}}))


if __name__ == "__main__":
    main()
