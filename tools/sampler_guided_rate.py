"""hipGraph-replayed 32-step guided Heun solve rate of the CIFAR-10 net, guided by a second random-init CIFAR-10 net of
the same config:  python tools/sampler_guided_rate.py [B] [bf16|f32|f32x3] [reps] [cfg]

Three cases: unguided (63 network evaluations); guided on all 63 evaluations (126); guided on the interval
(0.28, 5.42] only (20 of the 63 evaluations guided: 83).

With `cfg` as the fourth argument, the class-conditional CIFAR-10 net (cifar10_cond) instead, guided on all evaluations
twice: by its own label-free evaluation (guide="unconditional", no second network) and by a separate random-init net of
the same config; each with the peak device memory of its capture and replays (the self-guided case runs first, before
the second network exists)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import tinyedm  # noqa: E402
from tinyedm.config import instantiate  # noqa: E402

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
dt_name = sys.argv[2] if len(sys.argv) > 2 else "f32x3"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
cfg_mode = len(sys.argv) > 4 and sys.argv[4] == "cfg"
model, cfg = bench.build_model(dev, conditional=cfg_mode)
model.eval()
model.denoiser.set_eval_dtype(dt_name)
x0 = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(7)).to(dev)
labels = torch.randint(0, 10, (B,), generator=torch.Generator().manual_seed(8)).to(dev) if cfg_mode else None


def separate_guide():
    tinyedm.manual_seed(cfg.seed + 1)
    torch.manual_seed(cfg.seed + 1)
    guide = instantiate(cfg.model).to(dev).eval()
    guide.denoiser.set_eval_dtype(dt_name)
    return guide


if cfg_mode:
    cases = (("cond, self-guided (guide='unconditional')", lambda: {"guide": "unconditional", "guidance": 2.0}),
             ("cond, separate guide net", lambda: {"guide": separate_guide(), "guidance": 2.0}))
else:
    guide = separate_guide()
    cases = (("unguided", lambda: {}), ("guided, all", lambda: {"guide": guide, "guidance": 2.0}),
             ("guided, (0.28, 5.42]", lambda: {"guide": guide, "guidance": 2.0, "guidance_interval": (0.28, 5.42)}))
base = None
for name, kw in cases:
    solver = tinyedm.DeterministicSolver(num_steps=32, **kw())
    nfe = 63 + sum(solver.guided_evaluations())
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    out = solver.solve(model, x0, labels, graph=True)          # capture + warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = solver.solve(model, x0, labels, graph=True)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    peak = torch.cuda.max_memory_allocated(dev) / 2 ** 20
    base = base or dt
    print(f"{dt_name} B={B} {name}: {nfe} evaluations, {dt * 1e3:.1f} ms per solve, {B / dt:.1f} img/s, "
          f"{dt / base:.3f}x first case, peak {peak:.0f} MiB, |x|={float(out.norm()):.4f}", flush=True)
    del solver, out
