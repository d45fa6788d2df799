"""Cost of DiffusionClassifier.classify against NoiseLevelEvaluator.evaluate on the class-conditional CIFAR-10 net, and of
the two class-sweep kernels against the replicated form they replace:
python tools/classify_rate.py [num_images] [bf16|f32x3|f32] [repeats] [num_levels]

Both evaluators run network calls of 512 rows (batch_size = 512; C = 10, so a classifier call holds 51 pairs = 510
rows), and network rows/s is the comparable figure: the classifier spends C rows on an (image, level) pair where the
evaluator spends one.  Kernels: P = 51 pairs x C = 10 at 3x32x32, ops.eval_diffuse_classes + ops.eval_sqerr_classes
against index_select + repeat_interleave + ops.eval_diffuse + ops.eval_sqerr on the P * C replicated rows.  The two
forms are checked to give the same bits before they are timed.  Each case is warmed up, then timed with device events
over `repeats` runs, the cases alternating; the median and the min..max spread are printed."""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tinyedm_amd import ops  # noqa: E402
from tinyedm_amd.classify import DiffusionClassifier  # noqa: E402
from tinyedm_amd.evaluate import NoiseLevelEvaluator  # noqa: E402

dev = torch.device("cuda:0")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
dt_name = sys.argv[2] if len(sys.argv) > 2 else "bf16"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
L = int(sys.argv[4]) if len(sys.argv) > 4 else 8
C, BATCH = 10, 512
model, cfg = bench.build_model(dev, conditional=True)
model.eval()
g = torch.Generator().manual_seed(7)
img = (0.5 * torch.randn(N, 3, 32, 32, generator=g)).to(dev)
lab = torch.randint(0, C, (N,), generator=g).to(dev)


def timed(cases, reps, warm=2):
    """name -> list of ms, the cases alternating within each repeat"""
    for fn in cases.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, fn in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


# ---------------------------------------------------------------- the evaluators
clf = DiffusionClassifier(num_levels=L, batch_size=BATCH, network_dtype=dt_name, seed=1)
ev = NoiseLevelEvaluator(num_levels=L, batch_size=BATCH, network_dtype=dt_name, seed=1)
# the evaluator gets C times the images, so both evaluate about N * L * C network rows per run
img_ev, lab_ev = img.repeat(C, 1, 1, 1), lab.repeat(C)
res = {}
ms = timed({"classify": lambda: res.__setitem__("c", clf.classify(model, img, lab)),
            "evaluate": lambda: res.__setitem__("e", ev.evaluate(model, img_ev, lab_ev))}, reps, warm=1)
rows = {"classify": N * L * C, "evaluate": N * C * L}
rate = {}
for k, v in ms.items():
    med = statistics.median(v)
    rate[k] = rows[k] / med * 1e3
    extra = f", {N / med * 1e3:.1f} images/s" if k == "classify" else ""
    print(f"{dt_name} {k}: median {med:.1f} ms over {reps} runs (min {min(v):.1f}, max {max(v):.1f}), "
          f"{rows[k]} network rows, {rate[k]:.0f} rows/s{extra}", flush=True)
print(f"{dt_name} N={N} L={L} C={C}: classify rows/s : evaluate rows/s = {rate['classify'] / rate['evaluate']:.3f}; "
      f"accuracy {res['c']['accuracy']:.4f} (random weights), expected_loss {res['e']['expected_loss']:.6g}", flush=True)

# ---------------------------------------------------------------- the kernels against the replicated form
P = BATCH // C
src = img[:P].contiguous() if N >= P else img.repeat((P + N - 1) // N, 1, 1, 1)[:P].contiguous()
idx = torch.arange(P, device=dev)
ids = torch.from_numpy(np.arange(P, dtype=np.uint32)).to(dev)
level = (torch.arange(P, dtype=torch.int32) % L).to(dev)
ids_rep = torch.from_numpy(np.repeat(np.arange(P, dtype=np.uint32), C)).to(dev)      # (a work list is built once)
level_rep = level.repeat_interleave(C)
sig = torch.tensor(clf.levels.levels_for(model), dtype=torch.float32, device=dev)
rec = ops.churn_record(1, 0, dev)
D = torch.randn(P * C, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(dev)
out = torch.empty(P * C, dtype=torch.float64, device=dev)
REPEAT = 500         # launches per timed window: one launch is tens of microseconds, a window tens of milliseconds


def sweep():
    for _ in range(REPEAT):
        clean = src.index_select(0, idx)
        noisy, s = ops.eval_diffuse_classes(clean, ids, level, sig, rec, C, check_levels=False)
        ops.eval_sqerr_classes(D, clean, C, out=out)
    return noisy, s, out


def replicated():
    for _ in range(REPEAT):
        clean = src.index_select(0, idx).repeat_interleave(C, 0)
        noisy, s = ops.eval_diffuse(clean, ids_rep, level_rep, sig, rec, check_levels=False)
        ops.eval_sqerr(D, clean, out=out)
    return noisy, s, out


a = [t.clone() for t in sweep()]
b = [t.clone() for t in replicated()]
assert all(torch.equal(x, y) for x, y in zip(a, b)), "the class-sweep kernels and the replicated form differ"
ms = timed({"class sweep": sweep, "replicated": replicated}, max(reps, 7))
med = {k: statistics.median(v) / REPEAT * 1e3 for k, v in ms.items()}
for k, v in ms.items():
    print(f"kernels P={P} C={C} 3x32x32, {k}: median {med[k]:.1f} us per (gather, diffuse, sqerr) over {len(v)} windows of "
          f"{REPEAT} (min {min(v) / REPEAT * 1e3:.1f}, max {max(v) / REPEAT * 1e3:.1f})", flush=True)
print(f"kernels: replicated : class sweep = {med['replicated'] / med['class sweep']:.2f}", flush=True)
ops.check_health(dev, "classify_rate")
