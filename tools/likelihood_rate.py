"""Cost of DeterministicSolver.log_likelihood against invert on the CIFAR-10 net, 32 steps, hipGraph replays:
python tools/likelihood_rate.py [B] [f32x3|f32] [repeats] [num_probes]

Both run 62 network evaluations; log_likelihood evaluates (1 + 2 * num_probes) B rows per call where invert evaluates
B, so about 3x at one probe is the expectation from the batch arithmetic.  Each case is captured and warmed up, then
timed with device events over `repeats` replays; the median and the min..max spread are printed."""
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
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
dt_name = sys.argv[2] if len(sys.argv) > 2 else "f32x3"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
K = int(sys.argv[4]) if len(sys.argv) > 4 else 1
model.denoiser.set_eval_dtype(dt_name)
img = (0.5 * torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(7))).to(dev)
solver = tinyedm.DeterministicSolver(num_steps=32, seed=1)
cases = {"invert": lambda: solver.invert(model, img, None, graph=True),
         "log_likelihood": lambda: solver.log_likelihood(model, img, None, graph=True, num_probes=K)}
med = {}
for name, fn in cases.items():
    for _ in range(3):              # capture + warm-up
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    med[name] = statistics.median(ms)
    print(f"{dt_name} B={B} {name}: median {med[name]:.2f} ms per solve over {reps} replays (min {min(ms):.2f}, max "
          f"{max(ms):.2f}), {B / med[name] * 1e3:.1f} img/s, mean(out)={float(out.double().mean()):.6g}", flush=True)
print(f"{dt_name} B={B} num_probes={K}: log_likelihood : invert = {med['log_likelihood'] / med['invert']:.3f}", flush=True)
