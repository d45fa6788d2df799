"""hipGraph-replayed solve rate of the CIFAR-10 net, Heun against DPM-Solver++ multistep:
python tools/sampler_multistep_rate.py [B] [bf16|f32|f32x3,...] [reps] [cases]

Three cases (comma-separated names for [cases], default all): heun32, the 32-step Heun solve (63 network
evaluations); 2m32, DPM-Solver++(2M) with 32 steps (32 evaluations, 32 k_dpm_multistep launches); 3m18, DPM-Solver++(3M)
with 18 steps (18 evaluations).  Several precisions may be given, comma-separated (default bf16,f32x3)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import tinyedm  # noqa: E402

CASES = {
    "heun32": lambda: tinyedm.DeterministicSolver(num_steps=32),
    "2m32": lambda: tinyedm.MultistepSolver(num_steps=32, order=2),
    "3m18": lambda: tinyedm.MultistepSolver(num_steps=18, order=3),
}

dev = torch.device("cuda:0")
model, cfg = bench.build_model(dev)
model.eval()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
dtypes = (sys.argv[2] if len(sys.argv) > 2 else "bf16,f32x3").split(",")
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
names = sys.argv[4].split(",") if len(sys.argv) > 4 else list(CASES)
x0 = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(7)).to(dev)
for dt_name in dtypes:
    model.denoiser.set_eval_dtype(dt_name)
    base = None
    for name in names:
        solver = CASES[name]()
        evals = len(solver.guided_evaluations())
        out = solver.solve(model, x0, None, graph=True)          # capture + warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = solver.solve(model, x0, None, graph=True)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        base = base if base is not None else (dt if name == "heun32" else None)
        ratio = f"{dt / base:.4f}x heun32" if base else "(no heun32 case run)"
        print(f"{dt_name} B={B} {name}: {evals} evaluations, {dt * 1e3:.2f} ms per solve, {dt / evals * 1e3:.3f} ms per "
              f"evaluation, {B / dt:.1f} img/s, {ratio}, |x|={float(out.norm()):.4f}", flush=True)
