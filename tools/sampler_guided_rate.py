"""hipGraph-replayed 32-step guided Heun solve rate of the CIFAR-10 net, guided by a second random-init CIFAR-10 net of
the same config:  python tools/sampler_guided_rate.py [B] [bf16|f32|f32x3] [reps]

Three cases: unguided (63 network evaluations); guided on all 63 evaluations (126); guided on the interval
(0.28, 5.42] only (20 of the 63 evaluations guided: 83)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import tinyedm  # noqa: E402
from tinyedm.config import instantiate  # noqa: E402

dev = torch.device("cuda:0")
model, cfg = bench.build_model(dev)
model.eval()
tinyedm.manual_seed(cfg.seed + 1)
torch.manual_seed(cfg.seed + 1)
guide = instantiate(cfg.model).to(dev).eval()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
dt_name = sys.argv[2] if len(sys.argv) > 2 else "f32x3"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
model.denoiser.set_eval_dtype(dt_name)
guide.denoiser.set_eval_dtype(dt_name)
x0 = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(7)).to(dev)
base = None
for name, kw in (("unguided", {}), ("guided, all", {"guide": guide, "guidance": 2.0}),
                 ("guided, (0.28, 5.42]", {"guide": guide, "guidance": 2.0, "guidance_interval": (0.28, 5.42)})):
    solver = tinyedm.DeterministicSolver(num_steps=32, **kw)
    nfe = 63 + sum(solver.guided_evaluations())
    out = solver.solve(model, x0, None, graph=True)          # capture + warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = solver.solve(model, x0, None, graph=True)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    base = base or dt
    print(f"{dt_name} B={B} {name}: {nfe} evaluations, {dt * 1e3:.1f} ms per solve, {B / dt:.1f} img/s, "
          f"{dt / base:.3f}x unguided, |x|={float(out.norm()):.4f}", flush=True)
