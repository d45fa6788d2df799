"""bench.py: a plain run prints the headline line only; --full adds the roofline, the sampler legs and the CPU baseline."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config"}


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--batch", "16", *extra], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def test_plain_run_is_the_headline_line():
    line, err = _bench()
    assert set(line) == HEADLINE, sorted(line)
    assert line["steps"] == 3 and line["warmup"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["config"]["per_gpu_batch"] == 16 and line["config"]["step_launch"] in ("hipGraph replay", "eager")
    assert "sampler (" not in err and "cpu baseline" not in err


def test_full_run_adds_roofline_sampler_and_cpu_baseline():
    line, _ = _bench("--full", "--sampler-batch", "8", "--sampler-f32-batch", "8", "--sampler-iters", "1",
                     "--cpu-batch", "2", "--cpu-steps", "1")
    assert HEADLINE <= set(line)
    roof = line["roofline"]
    # (at batch 16 the dominant 32x32 kernel of batch 128 is not dispatched: the instrumented steps time the others)
    assert roof["bound"] == "mfma" and "library_gemm_tflops_same_shape" in roof and roof["per_kernel"]
    assert all(k["launches"] > 0 and k["ms"] > 0 for k in roof["per_kernel"].values()), roof["per_kernel"]
    for leg, dtype in (("sampler", "bf16"), ("sampler_fp32", "f32"), ("sampler_fp32_split", "f32x3")):
        assert line[leg]["network_dtype"] == dtype and line[leg]["batch"] == 8 and line[leg]["img_per_s"] > 0, leg
    assert line["cpu_baseline"]["value"] > 0
