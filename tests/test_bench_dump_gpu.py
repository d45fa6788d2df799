"""bench.py --dump-outputs: what the timed paths computed lands in DIR/<name>.npy (float32, at most 64 MB), and two runs
with the same arguments -- same seeded inputs -- write the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"train_loss", "train_weights", "train_ema_weights", "train_adam_m", "train_adam_v", "sampler_bf16_images",
         "sampler_f32_images", "sampler_f32x3_images"}


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--batch", "16", "--step-launch", "graph", "--sampler-batch", "8", "--sampler-f32-batch", "8",
                        "--sampler-iters", "1", "--no-cpu-baseline", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}
    return line, arrays


def rel(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def test_dump_outputs_are_the_timed_results_and_repeat(tmp_path):
    line, a = _bench(tmp_path / "a")
    assert line["steps"] == 3 and line["config"]["step_launch"] == "hipGraph replay"
    assert set(a) == NAMES
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["train_loss"].shape == (1,) and float(a["train_loss"][0]) == pytest.approx(line["config"]["final_loss"], rel=1e-6)
    assert a["train_weights"].shape == a["train_adam_v"].shape == (1 << 21,)          # seeded sample of the 35.6 M arena
    assert a["sampler_bf16_images"].shape == a["sampler_f32_images"].shape == (8, 3, 32, 32)
    _, b = _bench(tmp_path / "b")
    assert set(b) == NAMES
    for k in sorted(NAMES):
        # the Adam moments carry the order of the atomically accumulated weight gradients (as in test_graph_gpu.py)
        assert rel(b[k], a[k]) <= (2e-2 if k.startswith("train_adam") else 1e-5), k
