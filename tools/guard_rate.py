"""Cost of the guarded optimizer step on the CIFAR-10 configuration (conf/cifar10.yaml, B=128, 35.6 M parameters), A/B in
one process with HIP events, warm-up first, medians over alternating rounds:
  1. the guard's three launches alone on the model's real gradient arena, next to k_adam_ema on the same arena (the guard
     reads one stream where the optimizer pass moves ten: target <= 0.2 x), and next to the guarded optimizer kernel;
  2. ms/step of the hipGraph-replayed step: unguarded with the fused weight-gradient finish (what an unguarded run
     takes), unguarded with EDM_FUSED_OPT=0 (whole-arena optimizer pass), and guarded (which implies the latter).
     guarded - unfused is the guard itself, guarded - fused the whole price of the feature.
python tools/guard_rate.py [steps_per_block] [rounds] [chunk ...]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import tinyedm  # noqa: E402
from tinyedm_amd import ops  # noqa: E402
from tinyedm_amd.ema import EMAOptimizer  # noqa: E402
from tinyedm_amd.graph import CapturedTrainStep  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
chunks = [int(c) for c in sys.argv[3:]] or [ops.GUARD_CHUNK]

dev = torch.device("cuda:0")
model, cfg = bench.build_model(dev)
model.train()
base = model.configure_optimizers()["optimizer"]
base.fuse_zero_grad = True
opt = EMAOptimizer(base, device=dev, gamma=tinyedm.sigma_rel_to_gamma(model.ema_length),
                   every_n_steps=model.every_n_steps)
opt.zero_grad()
g = torch.Generator().manual_seed(42)
batch = ((0.5 * torch.randn(128, 3, 32, 32, generator=g)).to(dev), torch.randint(0, 10, (128,), generator=g).to(dev))
n = base.arena.numel


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def report(name, t, extra=""):
    t = np.array(t)
    print(f"  {name:34s} median {np.median(t):8.4f} ms  (min {t.min():.4f}, max {t.max():.4f}){extra}", flush=True)
    return float(np.median(t))


# ---- 1. the kernels alone, on copies of the real arenas (lr = 0 keeps the state finite over thousands of launches)
theta, m, v, ema = (t.clone() for t in (base.arena.theta, base.m, base.v, opt.ema_arena))
grad = (1e-3 * torch.randn(n, generator=torch.Generator().manual_seed(1))).to(dev)
numels = [p.numel() for p in base.arena.params]
sumsq = torch.zeros(len(numels), dtype=torch.float64, device=dev)
rec = ops.guard_record(dev)
adam_args = (0.0, 0.9, 0.999, 1e-8, 10, 0.999, 1.0)
kernels = {"k_adam_ema": lambda: ops.adam_ema(theta, grad, m, v, ema, *adam_args),
           "k_adam_ema_guarded": lambda: ops.adam_ema_guarded(theta, grad, m, v, ema, rec, *adam_args)}
for c in chunks:
    tab = ops.grad_guard_table(base.arena.offsets, numels, n, dev, chunk=c)
    kernels[f"grad_guard (chunk {c}, {tab.chunks.shape[0]} chunks)"] = \
        lambda tab=tab: ops.grad_guard(grad, tab, sumsq, rec, max_norm=1.0, skip_nonfinite=True)
for fn in kernels.values():
    timed(fn, 20)
times = {k: [] for k in kernels}
for r in range(rounds):
    for k in (list(kernels) if r % 2 == 0 else list(kernels)[::-1]):
        times[k].append(timed(kernels[k], 50))
print(f"kernels alone, {n / 1e6:.1f} M parameters in {len(numels)} tensors, {rounds} rounds x 50 launches:")
med = {k: report(k, t) for k, t in times.items()}
for k, t in med.items():
    if k.startswith("grad_guard"):
        print(f"  {k}: {t / med['k_adam_ema']:.3f} x k_adam_ema (target <= 0.2), {4 * n / t / 1e6:.0f} GB/s of gradient read; "
              f"k_adam_ema moves {9 * 4 * n / med['k_adam_ema'] / 1e6:.0f} GB/s", flush=True)
print(f"  guarded / unguarded optimizer kernel: {med['k_adam_ema_guarded'] / med['k_adam_ema']:.3f}")
del theta, m, v, ema, grad


# ---- 2. the captured step in three forms (one optimizer: the forms differ in what step_dyn launches)
def make(fused, guard):
    os.environ["EDM_FUSED_OPT"] = "1" if fused else "0"
    base.set_guard(**(dict(max_norm=1.0, skip_nonfinite=True) if guard else {}))
    step = CapturedTrainStep(model, opt)
    for _ in range(CapturedTrainStep.WARMUP + 3):
        step(batch)
    assert step.last_path == ("fused" if fused and not guard else "unfused"), step.last_path
    return step


forms = {}
forms["unguarded, fused finish"] = (make(True, False), False)
forms["unguarded, EDM_FUSED_OPT=0"] = (make(False, False), False)
forms["guarded"] = (make(False, True), True)
torch.cuda.synchronize()


def run_form(name):
    step, guard = forms[name]
    base.set_guard(**(dict(max_norm=1.0, skip_nonfinite=True) if guard else {}))
    step(batch)                                  # (one untimed step after the switch)
    return timed(lambda: step(batch), steps)


times = {k: [] for k in forms}
for r in range(rounds):
    for k in (list(forms) if r % 2 == 0 else list(forms)[::-1]):
        times[k].append(run_form(k))
print(f"captured CIFAR-10 step, B=128, {rounds} rounds x {steps} steps per block:")
med = {k: report(k, t, f"  {128e3 / np.median(t):.0f} img/s") for k, t in times.items()}
fu, un, gd = med["unguarded, fused finish"], med["unguarded, EDM_FUSED_OPT=0"], med["guarded"]
print(f"  guarded - unfused = {1e3 * (gd - un):+.1f} us/step (the guard's own launches)")
print(f"  guarded - fused   = {1e3 * (gd - fu):+.1f} us/step ({100 * (gd / fu - 1):+.2f} %: the feature's full price)")
print(f"  guard record after the run: {base.guard_stats() if base.guard is not None else None}")
