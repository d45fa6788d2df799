"""What an optimised sampling schedule buys for a real network, and what the pair-cost kernel costs:
python tools/schedule_gain.py [--ckpt_path CKPT [--load_ema] | --config_name cifar10] [--steps 8,10,22] [--grid 64]
                              [--warmup 64] [--batch 16] [--order 2] [--network_dtype f32x3] [--ref_rtol 1e-5] [--no_rate]

Gain: the schedules are optimised (tinyedm.schedule.optimize_schedule) on --warmup samples drawn from --warmup_seed; on
--batch OTHER x0, drawn from --seed, the RMS distance to the adaptive solve of the same net at the tight tolerance
--ref_rtol (atol = rtol / 10) is printed for Heun and DPM-Solver++(2M), each on the N-step Karras table and on the
optimised table, with the summed step costs of both tables where the grid holds the Karras one.  A sum of local errors is
not the global error: the optimised row can be the worse one, which is why the Karras row is always printed next to it.
A config name samples a random-init net (seeded by the config): plumbing, not a quality claim.

Rate: ops.pair_step_errors against the same quantity from a torch fp64 loop over the nodes (per node i one broadcast
over all j > i: [G - i, B, K] fp64 temporaries) on the same device, at G = 64, B = 64, K = 3072, order 2: the time of a
call (device events, warmed up, the two alternating, median of --repeats) and the peak memory each allocates beyond its
operands and its result.  The two results are compared first.  GPU only; reads nothing outside the tree."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tinyedm  # noqa: E402
from tinyedm_amd import networks, ops  # noqa: E402
from tinyedm_amd.config import compose, instantiate  # noqa: E402
from tinyedm_amd.schedule import optimize_schedule  # noqa: E402


def torch_pair_step_errors(X, S, tau, order):
    """ops.pair_step_errors by its definition in torch fp64, one broadcast per start node"""
    G, B = S.shape[0], S.shape[1]
    X, S = X.reshape(G + 1, B, -1), S.reshape(G, B, -1)
    d2 = torch.zeros((B, G, G + 1), dtype=torch.float64, device=X.device)
    for i in range(G):
        h = (tau[i + 1:] - tau[i])[:, None, None]                                  # [G - i, 1, 1]
        xi, si = X[i].double()[None], S[i].double()[None]
        e = xi + h * si - X[i + 1:].double()                                       # the Euler jump to every j > i
        if order == 2 and i + 1 < G:                                               # the trapezoid for the targets j < G
            e[:-1] = xi + (h[:-1] / 2) * (si + S[i + 1:].double()) - X[i + 1:G].double()
        d2[:, i, i + 1:] = (e * e).sum(dim=2).t()
    return d2


def rate(repeats, G=64, B=64, K=3072, order=2):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    tau = tinyedm.DeterministicSolver(num_steps=G).t_steps.double().to(dev)
    X = (torch.randn(G + 1, B, K, generator=g) * (tau.cpu() ** 2 + 0.25).sqrt().float()[:, None, None]).to(dev)
    S = torch.randn(G, B, K, generator=g).to(dev)
    cases = {"ops.pair_step_errors": lambda: ops.pair_step_errors(X, S, tau, order),
             "torch fp64 loop over the nodes": lambda: torch_pair_step_errors(X, S, tau, order)}
    a, b = (fn() for fn in cases.values())
    up = torch.triu(torch.ones(G, G + 1, dtype=torch.bool, device=dev), 1)
    print(f"pair costs at G = {G}, B = {B}, K = {K}, order {order}: largest relative difference of the two results "
          f"{float(((a - b).abs() / b.abs().clamp_min(1e-300))[:, up].max()):.3g}")
    del a, b
    ms, mem = {k: [] for k in cases}, {}
    for k, fn in cases.items():             # (also the warm-up)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        mem[k] = torch.cuda.max_memory_allocated() - base - out.numel() * out.element_size()
        del out
    for _ in range(repeats):
        for k, fn in cases.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            ms[k].append(s.elapsed_time(e))
    for k in cases:
        print(f"  {k}: median {statistics.median(ms[k]):.3f} ms over {repeats} calls (min {min(ms[k]):.3f}, max "
              f"{max(ms[k]):.3f}), peak extra memory {mem[k] / 2 ** 20:.1f} MiB")
    med = [statistics.median(v) for v in ms.values()]
    print(f"  the kernel takes {med[0] / med[1]:.3g} of the torch loop's time" + (" (it is SLOWER)" if med[0] > med[1] else ""))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--ckpt_path", default=None)
    ap.add_argument("--load_ema", action="store_true")
    ap.add_argument("--config_name", default="cifar10")
    ap.add_argument("--steps", default="8,10,22")
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--warmup_batch", type=int, default=32)
    ap.add_argument("--warmup_seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--order", type=int, choices=[1, 2], default=2)
    ap.add_argument("--image_size", type=int, default=32)
    ap.add_argument("--network_dtype", choices=["bf16", "f32", "f32x3"], default="f32x3")
    ap.add_argument("--ref_rtol", type=float, default=1e-5)
    ap.add_argument("--max_iterations", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no_rate", action="store_true")
    ap.add_argument("--no_gain", action="store_true")
    args = ap.parse_args(argv)
    if args.seed == args.warmup_seed:
        ap.error("--seed and --warmup_seed must differ: the schedule is judged on x0 it was not optimised on")
    dev = torch.device("cuda:0")
    if not args.no_gain:
        if args.ckpt_path is not None:
            model = tinyedm.EDM.load_from_checkpoint(args.ckpt_path, load_ema=args.load_ema)
            what = f"{args.ckpt_path}{' (EMA)' if args.load_ema else ''}"
        else:
            cfg = compose(args.config_name, os.path.join(ROOT, "experiments", "conf"))
            networks.manual_seed(cfg.seed)
            torch.manual_seed(cfg.seed)
            model = instantiate(cfg.model)
            what = f"random-init {args.config_name} (plumbing: not a quality claim)"
        model = model.to(dev).eval()
        model.denoiser.set_eval_dtype(args.network_dtype)
        steps = [int(v) for v in args.steps.split(",")]
        B, C = args.batch, int(model.denoiser.in_channels)
        shape = (C, args.image_size, args.image_size)
        found = optimize_schedule(model, steps, shape=shape, grid=args.grid, warmup=args.warmup, batch_size=args.warmup_batch,
                                  order=args.order, seed=args.warmup_seed,
                                  num_classes=model.num_classes if model.conditional else None, device=dev)
        g = torch.Generator().manual_seed(args.seed)
        x0 = torch.randn(B, *shape, generator=g).to(dev)
        labels = torch.randint(0, model.num_classes, (B,), generator=g).to(dev) if model.conditional else None
        ref = tinyedm.AdaptiveSolver(rtol=args.ref_rtol, atol=args.ref_rtol / 10,
                                     max_iterations=args.max_iterations).solve(model, x0, labels).double()

        def distance(sol):
            d = sol.solve(model, x0, labels).double() - ref
            return float((d * d).mean().sqrt())
        print(f"{what}, {args.network_dtype}; grid {args.grid}, order {args.order}, warm-up {args.warmup} samples of seed "
              f"{args.warmup_seed}; judged on {B} x0 of seed {args.seed} against the adaptive solve at rtol {args.ref_rtol:g} "
              f"(rms of its images {float(ref.pow(2).mean().sqrt()):.4f})")
        print("| N | table | summed step cost | Heun rms distance | DPM-Solver++(2M) rms distance |")
        print("|---|---|---|---|---|")
        for s in found:
            N = s.num_steps
            karras = "n/a" if s.karras_cost is None else f"{s.karras_cost:.4g}"
            for name, cost, kw in (("Karras", karras, dict(num_steps=N)), ("optimised", f"{s.cost:.4g}", dict(sigmas=s.sigmas))):
                print(f"| {N} | {name} | {cost} | {distance(tinyedm.DeterministicSolver(**kw)):.4g} | "
                      f"{distance(tinyedm.MultistepSolver(order=2, **kw)):.4g} |", flush=True)
            print(f"|  | nodes {s.indices} | | | |")
    if not args.no_rate:
        rate(args.repeats)


if __name__ == "__main__":
    main()
