"""hipGraph-replayed 32-step stochastic Heun solve rate of the CIFAR-10 net:
python tools/sampler_stochastic_rate.py [B] [bf16|f32|f32x3] [reps] [cases]

Three cases (comma-separated names for [cases], default all): det, the deterministic solve; all, churn on every step
(S_churn 40, no window: 32 k_heun_churn launches per solve); window, EDM's ImageNet setting (S_churn 40, S_min 0.05,
S_max 50, S_noise 1.003).  Every case evaluates the network 63 times per solve."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import tinyedm  # noqa: E402

CASES = {
    "det": {"S_churn": 0.0},
    "all": {"S_churn": 40.0},
    "window": {"S_churn": 40.0, "S_min": 0.05, "S_max": 50.0, "S_noise": 1.003},
}

dev = torch.device("cuda:0")
model, cfg = bench.build_model(dev)
model.eval()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
dt_name = sys.argv[2] if len(sys.argv) > 2 else "bf16"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
names = sys.argv[4].split(",") if len(sys.argv) > 4 else list(CASES)
model.denoiser.set_eval_dtype(dt_name)
x0 = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(7)).to(dev)
base = None
for name in names:
    solver = tinyedm.StochasticSolver(num_steps=32, seed=1, **CASES[name])
    churned = int((solver.churn_schedule().gamma > 0).sum())
    out = solver.solve(model, x0, None, graph=True)          # capture + warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = solver.solve(model, x0, None, graph=True)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    base = base if base is not None else (dt if name == "det" else None)
    ratio = f"{dt / base:.4f}x deterministic" if base else "(no deterministic case run)"
    print(f"{dt_name} B={B} {name}: {churned} churned steps, {dt * 1e3:.2f} ms per solve, {B / dt:.1f} img/s, {ratio}, "
          f"|x|={float(out.norm()):.4f}", flush=True)
