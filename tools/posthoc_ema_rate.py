"""Cost of post-hoc EMA tracking: the hipGraph-replayed CIFAR-10 training step (conf/cifar10.yaml, B=128) with 0 and with
2 power-function profiles, blocks of the two alternating within one process, timed with HIP events; then the time of
one snapshot (device staging copy + pinned host copy + file write).
python tools/posthoc_ema_rate.py [steps_per_block] [rounds] [snapshot_dir]"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import tinyedm  # noqa: E402
from tinyedm_amd.ema import EMAOptimizer  # noqa: E402
from tinyedm_amd.graph import CapturedTrainStep  # noqa: E402
from tinyedm_amd.posthoc_ema import PostHocEMA  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 6
snap_dir = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="phema_rate_")

dev = torch.device("cuda:0")
model, cfg = bench.build_model(dev)
model.train()
base = model.configure_optimizers()["optimizer"]
base.fuse_zero_grad = True
opt = EMAOptimizer(base, device=dev, gamma=tinyedm.sigma_rel_to_gamma(model.ema_length),
                   every_n_steps=model.every_n_steps)
g = torch.Generator().manual_seed(42)
batch = ((0.5 * torch.randn(128, 3, 32, 32, generator=g)).to(dev), torch.randint(0, 10, (128,), generator=g).to(dev))

plain = CapturedTrainStep(model, opt)
for _ in range(CapturedTrainStep.WARMUP + 2):
    plain(batch)
cb = PostHocEMA(sigma_rels=(0.05, 0.10), snapshot_every_n_steps=10 ** 9, snapshot_dir=snap_dir)


class _T:
    optimizers = [opt]
    global_rank = 0
    global_step = 0


cb.on_fit_start(_T, model)           # attaches the profiles: `tracked` captures the edm_adam_ema_phema form
tracked = CapturedTrainStep(model, opt)
for _ in range(CapturedTrainStep.WARMUP + 2):
    tracked(batch)
torch.cuda.synchronize()
n = base.arena.numel


def block(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn(batch)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / steps


times = {"0": [], "2": []}
for r in range(rounds):
    for name, fn in (("0", plain), ("2", tracked)) if r % 2 == 0 else (("2", tracked), ("0", plain)):
        times[name].append(block(fn))
t0, t2 = np.array(times["0"]), np.array(times["2"])
ratio = t2 / t0
print(f"captured CIFAR-10 step, B=128, {n / 1e6:.1f} M params, {rounds} rounds x {steps} steps per block")
print(f"  0 profiles: {t0.mean():.3f} ms/step (min {t0.min():.3f}, max {t0.max():.3f})")
print(f"  2 profiles: {t2.mean():.3f} ms/step (min {t2.min():.3f}, max {t2.max():.3f})")
print(f"  ratio 2/0: mean {ratio.mean():.4f}, min {ratio.min():.4f}, max {ratio.max():.4f}; "
      f"added {1e3 * (t2.mean() - t0.mean()):.1f} us/step (profile traffic {2 * 8 * n / 1e6:.0f} MB/step)")

# one snapshot: staging copy + async host copy (on the step stream's timeline), then the file write at the next hook
torch.cuda.synchronize()
h0 = time.perf_counter()
cb._start(base.phema.count, base.phema.count)
h1 = time.perf_counter()
cb.flush()
h2 = time.perf_counter()
size = sum(os.path.getsize(os.path.join(snap_dir, f)) for f in os.listdir(snap_dir))
print(f"  snapshot: start {1e3 * (h1 - h0):.1f} ms host, copy wait + write {1e3 * (h2 - h1):.1f} ms, "
      f"{size / 1e6:.0f} MB on disk for 2 profiles")
