"""How far an N-step solve is from the ODE's own solution, for a real network:
python tools/truncation_error.py [--ckpt_path CKPT [--load_ema] | --config_name cifar10] [--batch 16]
                                 [--network_dtype f32x3] [--ref_rtol 1e-5] [--rtols 1e-2,1e-3,1e-4] [--steps 8,12,18,32,64]

The reference is the adaptive solve (tinyedm.AdaptiveSolver) of the same net from the same x0 at the tight tolerance
--ref_rtol (atol = rtol / 10 throughout).  Printed: the RMS distance to it (over all elements, and the worst image) of
Heun and DPM-Solver++(2M / 3M) at each N with their network evaluations, then the adaptive solver's own rows
(rtol -> evaluations, iterations, share of rejected steps, distance).  A config name samples a random-init net (seeded by
the config); labels, for a conditional net, are drawn from --seed.  GPU only; reads nothing outside the tree."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinyedm  # noqa: E402
from tinyedm_amd import networks  # noqa: E402
from tinyedm_amd.config import compose, instantiate  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--ckpt_path", default=None)
    ap.add_argument("--load_ema", action="store_true")
    ap.add_argument("--config_name", default="cifar10")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--image_size", type=int, default=32)
    ap.add_argument("--network_dtype", choices=["bf16", "f32", "f32x3"], default="f32x3")
    ap.add_argument("--ref_rtol", type=float, default=1e-5)
    ap.add_argument("--rtols", default="1e-2,1e-3,1e-4")
    ap.add_argument("--steps", default="8,12,18,32,64")
    ap.add_argument("--max_iterations", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    if args.ckpt_path is not None:
        model = tinyedm.EDM.load_from_checkpoint(args.ckpt_path, load_ema=args.load_ema)
        what = f"{args.ckpt_path}{' (EMA)' if args.load_ema else ''}"
    else:
        cfg = compose(args.config_name, os.path.join(ROOT, "experiments", "conf"))
        networks.manual_seed(cfg.seed)
        torch.manual_seed(cfg.seed)
        model = instantiate(cfg.model)
        what = f"random-init {args.config_name}"
    model = model.to(dev).eval()
    model.denoiser.set_eval_dtype(args.network_dtype)
    g = torch.Generator().manual_seed(args.seed)
    B, C = args.batch, int(model.denoiser.in_channels)
    x0 = torch.randn(B, C, args.image_size, args.image_size, generator=g).to(dev)
    labels = torch.randint(0, model.num_classes, (B,), generator=g).to(dev) if model.conditional else None

    def adaptive(rtol):
        sol = tinyedm.AdaptiveSolver(rtol=rtol, atol=rtol / 10, max_iterations=args.max_iterations)
        t0 = time.perf_counter()
        out = sol.solve(model, x0, labels).double()
        torch.cuda.synchronize()
        return out, sol.last_stats, time.perf_counter() - t0

    def distance(out):
        d = (out.double() - ref).reshape(B, -1)
        return float((d * d).mean().sqrt()), float((d * d).mean(dim=1).sqrt().max())
    ref, st, dt = adaptive(args.ref_rtol)
    steps = int((st.accepted + st.rejected).sum())
    print(f"{what}, {args.network_dtype}, B={B}, seed {args.seed}; rms of the reference images {float(ref.pow(2).mean().sqrt()):.4f}")
    print(f"reference: adaptive rtol {args.ref_rtol:g}: {st.evaluations} evaluations, {st.iterations} iterations, accepted "
          f"{int(st.accepted.min())}..{int(st.accepted.max())} per image, rejected {int(st.rejected.sum())} of {steps} steps "
          f"({int(st.rejected.sum()) / steps:.1%}), {dt:.1f} s")
    print("| solver | N | evaluations | rms distance | worst image |")
    print("|---|---|---|---|---|")
    for name, make in (("Heun", lambda N: tinyedm.DeterministicSolver(num_steps=N)),
                       ("DPM-Solver++(2M)", lambda N: tinyedm.MultistepSolver(num_steps=N, order=2)),
                       ("DPM-Solver++(3M)", lambda N: tinyedm.MultistepSolver(num_steps=N, order=3))):
        for N in (int(v) for v in args.steps.split(",")):
            sol = make(N)
            a, w = distance(sol.solve(model, x0, labels))
            print(f"| {name} | {N} | {len(sol.guided_evaluations())} | {a:.3g} | {w:.3g} |", flush=True)
    print("| adaptive rtol | evaluations | iterations | rejected steps | rms distance | worst image |")
    print("|---|---|---|---|---|---|")
    for rtol in (float(v) for v in args.rtols.split(",")):
        out, st, dt = adaptive(rtol)
        a, w = distance(out)
        steps = int((st.accepted + st.rejected).sum())
        print(f"| {rtol:g} | {st.evaluations} | {st.iterations} | {int(st.rejected.sum()) / steps:.1%} | {a:.3g} | {w:.3g} |",
              flush=True)


if __name__ == "__main__":
    main()
