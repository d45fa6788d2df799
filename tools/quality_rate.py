"""Rate of the paired image quality kernels (csrc/quality.hip) against the same quantities written with torch in fp64 on the
same device:
python tools/quality_rate.py [--repeats 5] [--inner 3] [--scale 1.0]

  pair_ssim            ops.pair_ssim on 50 000 x 32 x 32 x 3 and 10 000 x 64 x 64 x 3 uint8 (Gaussian 11 / 1.5)
  torch_ssim           the same quantity: the five moments by F.conv2d with the grouped separable Gaussian on .double()
                       inputs (valid region), the map, its mean, and the squared error
  feature_distance     ops.f32_pair_feature_distance on 512 x 32 x 32 x 256 and 512 x 8 x 8 x 256
  torch_distance       F.normalize(x.double(), dim=-1, eps=1e-10) of both, subtract, square, mean.  F.normalize divides by
                       max(|x|, eps), the kernel by |x| + eps: at the norms of this data (about 16) the two quantities
                       differ by 1e-11 relative, which is what max_abs_diff_vs_torch shows for these rows; nothing
                       asserts on it (the tests compare with the exact form, tests/quality_ref.py)

Timed as the median over `repeats` windows of `inner` calls each (device events; one warm-up call of every form first,
which is also the comparison of the two results; the forms alternating), with the peak device memory above what the
inputs hold and the rate of the input bytes read once.  --scale shrinks the image counts (a quick look).  Prints one JSON
line per point; cells where the kernel is not faster read so in `torch_over_ours` < 1."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tinyedm_amd import compare, ops  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--repeats", type=int, default=5)
p.add_argument("--inner", type=int, default=3)
p.add_argument("--scale", type=float, default=1.0)
args = p.parse_args()
if not torch.cuda.is_available():
    sys.exit("quality_rate: needs a GPU (a CPU run measures nothing)")
dev = torch.device("cuda:0")
WINDOW = compare.gaussian_window(11, 1.5)


def torch_ssim(a, b, chunk=5000):
    """uint8 [n, H, W, C] -> (ssim fp64 [n, C], sse fp64 [n, C]); in chunks of images: five fp64 maps of the whole set do
    not fit beside it"""
    w = torch.from_numpy(WINDOW).to(dev)
    C = a.shape[3]
    wr, wc = w.view(1, 1, 1, -1).repeat(C, 1, 1, 1), w.view(1, 1, -1, 1).repeat(C, 1, 1, 1)
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    filt = lambda x: F.conv2d(F.conv2d(x, wr, groups=C), wc, groups=C)      # noqa: E731
    ssim, sse = [], []
    for i in range(0, a.shape[0], chunk):
        x, y = (t[i:i + chunk].permute(0, 3, 1, 2).double() for t in (a, b))
        mx, my = filt(x), filt(y)
        vx, vy, cov = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
        s = ((2 * mx * my + c1) * (2 * cov + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
        ssim.append(s.mean(dim=(2, 3)))
        sse.append(((x - y) ** 2).sum(dim=(2, 3)))
    return torch.cat(ssim), torch.cat(sse)


def torch_distance(a, b):
    x, y = F.normalize(a.double(), dim=-1, eps=1e-10), F.normalize(b.double(), dim=-1, eps=1e-10)
    return ((x - y) ** 2).sum(dim=-1).mean(dim=(1, 2))


def measure(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.inner):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return s.elapsed_time(e) / args.inner, peak


def point(name, cases, nbytes, diff):
    ms, peak = {c: [] for c in cases}, {c: 0 for c in cases}
    for _ in range(args.repeats):
        for c, fn in cases.items():
            t, m = measure(fn)
            ms[c].append(t)
            peak[c] = max(peak[c], m)
    med = {c: statistics.median(v) for c, v in ms.items()}
    row = {"point": name, "input_mib": round(nbytes / 2 ** 20, 1), "max_abs_diff_vs_torch": diff}
    for c in cases:
        row[c + "_ms"] = round(med[c], 4)
        row[c + "_ms_all"] = [round(v, 4) for v in ms[c]]
        row[c + "_peak_extra_mib"] = round(peak[c] / 2 ** 20, 1)
        row[c + "_gb_per_s"] = round(nbytes / (med[c] * 1e-3) / 1e9, 1)
    ours, theirs = list(cases)
    row["torch_over_ours"] = round(med[theirs] / med[ours], 3)
    print(json.dumps(row), flush=True)


print(json.dumps({"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "inner": args.inner, "scale": args.scale}),
      flush=True)
g = torch.Generator().manual_seed(0)
for n, size in ((50000, 32), (10000, 64)):
    n = max(1, int(n * args.scale))
    a = torch.randint(0, 256, (n, size, size, 3), generator=g, dtype=torch.uint8).to(dev)
    b = (a.int() + torch.randint(-20, 21, a.shape, generator=g).to(dev)).clamp(0, 255).to(torch.uint8)
    cases = {"pair_ssim": lambda: ops.pair_ssim(a, b, WINDOW, 255.0), "torch_ssim": lambda: torch_ssim(a, b)}
    ours, theirs = cases["pair_ssim"](), cases["torch_ssim"]()          # the warm-up is the comparison
    assert torch.equal(ours[1], theirs[1]), "the squared error of uint8 images is exact in both"
    diff = float((ours[0] - theirs[0]).abs().max())
    del ours, theirs
    point(f"ssim {n}x{size}x{size}x3 u8", cases, 2.0 * a.numel(), diff)
    del a, b
for B, size, C in ((512, 32, 256), (512, 8, 256)):
    B = max(1, int(B * args.scale))
    a = torch.randn(B, size, size, C, generator=g).to(dev)
    b = a + 0.3 * torch.randn(B, size, size, C, generator=g).to(dev)
    cases = {"feature_distance": lambda: ops.f32_pair_feature_distance(a, b), "torch_distance": lambda: torch_distance(a, b)}
    diff = float((cases["feature_distance"]() - cases["torch_distance"]()).abs().max())
    point(f"distance {B}x{size}x{size}x{C} f32", cases, 8.0 * a.numel(), diff)
    del a, b
