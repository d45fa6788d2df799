"""Cost of FeatureExtractor.extract against one full evaluation of the same batch, and of the pool kernel against torch's mean:
python tools/feature_rate.py [f32x3|f32] [repeats] [batch]

Extraction: the random-init CIFAR-10 net, `batch` (512) uint8 images, taps "mid" (the last encoder block), the first 8x8
encoder block and the last decoder block, each against `model(noisy, sigma)` on the same noised batch in the same dtype.
extract() also normalises, noises and pools; the full evaluation is the network alone, so the ratio is an upper bound on
the network's share.  Pool kernel: ops.f32_pool_features against x.mean((1, 2)) on 512x32x32x256 (512 MiB: beyond the
256 MiB last-level cache, an HBM rate), 512x8x8x256 (32 MiB: cache-resident when replayed, not an HBM rate) and
1x32x32x192 (one map: launch-bound).  GB/s counts the bytes the algorithm needs, 4 (B HW C + B C).  Each case is warmed up,
then timed with device events over `repeats` windows, the cases alternating; the median and the min..max spread are printed.
Nothing is asserted."""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tinyedm_amd import ops  # noqa: E402
from tinyedm_amd.callbacks import _eval_dtype  # noqa: E402
from tinyedm_amd.features import FeatureExtractor  # noqa: E402
from tinyedm_amd.networks import DownSample  # noqa: E402

dev = torch.device("cuda:0")
dt_name = sys.argv[1] if len(sys.argv) > 1 else "f32x3"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
B = int(sys.argv[3]) if len(sys.argv) > 3 else 512
model, cfg = bench.build_model(dev)
model.eval()


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


# ---------------------------------------------------------------- extraction against a full evaluation
enc = list(model.denoiser.encoder_blocks)
downs, first8 = 0, len(enc) - 1
for i, blk in enumerate(enc):
    downs += isinstance(blk.resample, DownSample)
    if downs == 2:
        first8 = i
        break
taps = {"mid": "mid", "first 8x8": f"enc{first8}", "last decoder": f"dec{len(model.denoiser.decoder_blocks) - 1}"}
images = torch.from_numpy(np.random.default_rng(7).integers(0, 256, size=(B, 32, 32, 3), dtype=np.uint8)).to(dev)
clean = ops.u8_gather_normalize(images.permute(0, 3, 1, 2).contiguous(), torch.arange(B, device=dev), 0.5, 0.5)
sigma = torch.full((B,), 0.1, device=dev)
noisy = clean + 0.1 * torch.randn(clean.shape, device=dev, generator=torch.Generator(dev).manual_seed(1))


def full():
    with torch.no_grad(), _eval_dtype(model, dt_name):
        return model(noisy, sigma)


cases = {"full evaluation": full}
for label, tap in taps.items():
    ex = FeatureExtractor(model, sigma=0.1, taps=(tap,), batch_size=B, network_dtype=dt_name)
    cases[f"extract {tap} ({label})"] = lambda ex=ex: ex.extract(images)
ms = timed(cases, reps, warm=2)
base = statistics.median(ms["full evaluation"])
for k, v in ms.items():
    med = statistics.median(v)
    print(f"{dt_name} B={B} {k}: median {med:.1f} ms over {reps} runs (min {min(v):.1f}, max {max(v):.1f}), "
          f"{B / med * 1e3:.0f} images/s, {med / base:.3f} of a full evaluation", flush=True)

# ---------------------------------------------------------------- the pool kernel against torch's mean
for shape, repeat in (((512, 32, 32, 256), 10), ((512, 8, 8, 256), 200), ((1, 32, 32, 192), 500)):
    x = torch.randn(shape, device=dev, generator=torch.Generator(dev).manual_seed(2))
    out = torch.empty(shape[0], shape[3], device=dev)
    nbytes = 4.0 * (x.numel() + out.numel())

    def pool(x=x, out=out, repeat=repeat):
        for _ in range(repeat):
            ops.f32_pool_features(x, out)

    def mean(x=x, out=out, repeat=repeat):
        for _ in range(repeat):
            torch.mean(x, dim=(1, 2), out=out)

    diff = (ops.f32_pool_features(x).double() - x.double().mean((1, 2))).abs().max().item()
    ms = timed({"f32_pool_features": pool, "torch mean": mean}, max(reps, 7))
    med = {k: statistics.median(v) / repeat for k, v in ms.items()}
    for k, v in ms.items():
        print(f"pool {'x'.join(map(str, shape))} {k}: median {med[k] * 1e3:.1f} us per launch over {len(v)} windows of {repeat} "
              f"(min {min(v) / repeat * 1e3:.1f}, max {max(v) / repeat * 1e3:.1f}), {nbytes / med[k] / 1e6:.0f} GB/s",
              flush=True)
    print(f"pool {'x'.join(map(str, shape))}: torch mean : f32_pool_features = {med['torch mean'] / med['f32_pool_features']:.2f}"
          f" (max |difference from the fp64 mean| {diff:.2e})", flush=True)
ops.check_health(dev, "feature_rate")
