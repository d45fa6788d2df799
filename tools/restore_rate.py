"""Cost of zero-shot restoration (solve(..., degradation=, measurement=)) against the plain solve on the CIFAR-10 net,
32 Heun steps: python tools/restore_rate.py [B] [repeats] [scale] [dtypes, comma separated] [modes, comma separated]

A restoring solve adds one fp32 pass over the state (ops.project_denoised) to each of the 63 network evaluations; from
the bytes moved the expectation is an overhead well under one per cent.  For every evaluation precision (bf16, f32x3)
and mode (eager, graph) the plain and the restoring solve are warmed up (and captured), then timed ALTERNATELY with
device events over `repeats` rounds, so that clock and thermal drift hit both alike; the median, the min..max spread
and the ratio of the medians are printed."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import tinyedm  # noqa: E402

dev = torch.device("cuda:0")
model, cfg = bench.build_model(dev)
model.eval()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
scale = int(sys.argv[3]) if len(sys.argv) > 3 else 4
dtypes = sys.argv[4].split(",") if len(sys.argv) > 4 else ["bf16", "f32x3"]
modes = sys.argv[5].split(",") if len(sys.argv) > 5 else ["eager", "graph"]
g = torch.Generator().manual_seed(7)
x0 = torch.randn(B, 3, 32, 32, generator=g).to(dev)
deg = tinyedm.LinearDegradation(scale)
y = deg.measure((0.5 * torch.randn(B, 3, 32, 32, generator=g)).to(dev))
solver = tinyedm.DeterministicSolver(num_steps=32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


for dt_name in dtypes:
    model.denoiser.set_eval_dtype(dt_name)
    for mode in modes:
        graph = mode == "graph"
        cases = {"plain": lambda: solver.solve(model, x0, None, graph),
                 "restore": lambda: solver.solve(model, x0, None, graph, degradation=deg, measurement=y)}
        for fn in cases.values():
            for _ in range(2):          # capture + warm-up
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in cases}
        for _ in range(reps):
            for name, fn in cases.items():
                t, out = timed(fn)
                ms[name].append(t)
        med = {name: statistics.median(v) for name, v in ms.items()}
        for name, v in ms.items():
            print(f"{dt_name} {mode} B={B} {name}: median {med[name]:.2f} ms per solve over {reps} solves (min "
                  f"{min(v):.2f}, max {max(v):.2f}), {B / med[name] * 1e3:.1f} img/s", flush=True)
        resid = float((deg.measure(out.float()) - y).abs().max())
        print(f"{dt_name} {mode} B={B} scale={scale}: restore : plain = {med['restore'] / med['plain']:.4f}, "
              f"max |A x - y| = {resid:.2e}", flush=True)
