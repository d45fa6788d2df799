"""Paired image quality: image i against reference i.

Inpainting, SDEdit, zero-shot restoration (DDNM) and posterior sampling (DPS) all produce an image that is meant to be
compared with a known original.  This module scores such pairs, one number per image:

    mse, psnr    the squared error, summed on the GPU with SSIM in one pass (uint8: an exact integer)
    ssim         the structural similarity index of Wang, Bovik, Sheikh, Simoncelli 2004: Gaussian 11 / 1.5 window (or a
                 uniform one), fp64 throughout, the mean over the VALID region (no padding), biased variances -- the
                 quantity the original implementation and scikit-image's structural_similarity(gaussian_weights=True,
                 use_sample_covariance=False) average, per channel and then over the channels
    perceptual   with a checkpoint: the LPIPS FORM of a distance (Zhang et al. 2018) on the project's own denoiser
                 activations -- every pixel's channel vector scaled to unit length, subtracted, squared, averaged over
                 space, averaged over the taps

    python -m tinyedm.generate --ckpt_path last.ckpt --load_ema --init_dir photos --restore_scale 4 --output_dir restored ...
    python -m tinyedm.compare --image_dir restored --ref_image_dir photos --ckpt_path last.ckpt --load_ema --report quality.json

The perceptual number is the project's own distance, NOT LPIPS: the extractor is this project's denoiser, not VGG or
AlexNet, and the learned linear layers of LPIPS are absent.  The numbers are comparable between image sets scored with the
SAME extractor checkpoint, sigma, taps and seed, not with published LPIPS tables.  Both images of a pair are noised with
the same stream (seed, id), so identical images are at distance exactly 0.  The defaults (sigma 0.1, "mid") are the
feature extractor's: a starting point that has not been measured on this project's checkpoints, and no claim is made
about how well the distance tracks human judgement.
"""
from __future__ import annotations

import argparse
import json
import math
import os

import numpy as np
import torch

from .features import NETWORK_DTYPES, check_sigma

MAX_WIN = 15                    # ops.SSIM_MAX_WIN, repeated here so that the argument check needs no GPU library
WINDOWS = ("gaussian", "uniform")
PSNR_FLOOR = 1e-12              # on the MSE in [0, 1] pixel units: identical images read 120 dB, not infinity
METRICS = ("mse", "psnr", "ssim", "perceptual")
WORST_IS_HIGH = {"mse": True, "psnr": False, "ssim": False, "perceptual": True}


# ---------------------------------------------------------------------------------------------------- windows
def _check_win(win_size, who):
    if isinstance(win_size, bool) or not isinstance(win_size, int) or win_size % 2 == 0 or not 3 <= win_size <= MAX_WIN:
        raise ValueError(f"{who}: win_size must be an odd integer in [3, {MAX_WIN}], got {win_size!r}")


def gaussian_window(win_size: int = 11, sigma: float = 1.5) -> np.ndarray:
    """the fp64 taps exp(-(k - c)^2 / (2 sigma^2)), k = 0 .. win_size - 1, c = (win_size - 1) / 2, divided by their sum
    (Wang et al. 2004: 11 taps, sigma 1.5).  Built on the host, so the kernel and a reference use the same bits."""
    _check_win(win_size, "gaussian_window")
    try:
        s = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"gaussian_window: sigma must be a number, got {sigma!r}") from None
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"gaussian_window: sigma must be finite and > 0, got {sigma}")
    k = np.arange(win_size, dtype=np.float64) - (win_size - 1) / 2.0
    w = np.exp(-(k * k) / (2.0 * s * s))
    w = w / w.sum()
    return 0.5 * (w + w[::-1])        # (exactly symmetric)


def uniform_window(win_size: int = 7) -> np.ndarray:
    """win_size equal fp64 taps of 1 / win_size"""
    _check_win(win_size, "uniform_window")
    return np.full(win_size, 1.0 / win_size, dtype=np.float64)


def make_window(window: str, win_size: int, win_sigma: float) -> np.ndarray:
    if window not in WINDOWS:
        raise ValueError(f"compare: window must be one of {WINDOWS}, got {window!r}")
    return gaussian_window(win_size, win_sigma) if window == "gaussian" else uniform_window(win_size)


def default_win_size(image_size: int) -> int:
    """11 taps (Wang et al. 2004) where the image holds them, else the largest odd window that fits"""
    fit = image_size if image_size % 2 else image_size - 1
    return max(3, min(11, fit))


def psnr_from_sse(sse, count, data_range):
    """PSNR in dB from a sum of squared errors over `count` values of range `data_range`: -10 log10 of the MSE in [0, 1]
    pixel units, floored at 1e-12 as generate's restore report does (identical images: 120 dB).  Tensors or numbers;
    fp64."""
    sse = torch.as_tensor(sse, dtype=torch.float64)
    count = torch.as_tensor(count, dtype=torch.float64).to(sse.device)
    mse01 = sse / (count * float(data_range) ** 2)
    return -10.0 * torch.log10(mse01.clamp_min(PSNR_FLOOR))


def region_from_box(box, H: int, W: int, win_size: int) -> np.ndarray:
    """uint8 [1, H, W], 1 inside X0 <= x < X1, Y0 <= y < Y1.  Refused when the box is not inside the image or holds no
    valid window centre (a centre is at least (win_size - 1) / 2 from every edge): its SSIM would be NaN."""
    try:
        x0, y0, x1, y1 = (int(v) for v in box)
        ok = len(box) == 4 and all(int(v) == v for v in box)
    except (TypeError, ValueError):
        ok = False
    if not ok or not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
        raise ValueError(f"compare: a box X0 Y0 X1 Y1 needs integers with 0 <= X0 < X1 <= {W} and 0 <= Y0 < Y1 <= {H}, "
                         f"got {list(box) if hasattr(box, '__iter__') else box}")
    half = (win_size - 1) // 2
    if max(x0, half) >= min(x1, W - half) or max(y0, half) >= min(y1, H - half):
        raise ValueError(f"compare: the box {[x0, y0, x1, y1]} holds no valid centre of a {win_size}-tap window in a "
                         f"{H} x {W} image (centres lie in [{half}, {W - half}) x [{half}, {H - half}))")
    r = np.zeros((1, H, W), dtype=np.uint8)
    r[0, y0:y1, x0:x1] = 1
    return r


def summarize(values) -> dict:
    """mean, std (population), median, min, max of a 1-d fp64 tensor"""
    v = torch.as_tensor(values, dtype=torch.float64).flatten().cpu()
    return {"mean": float(v.mean()), "std": float(v.std(unbiased=False)), "median": float(v.median()),
            "min": float(v.min()), "max": float(v.max())}


def worst_indices(values, metric: str, k: int) -> list:
    """the positions of the k worst images of a metric, the worst first, ties to the lower position"""
    v = torch.as_tensor(values, dtype=torch.float64).flatten().cpu().numpy()
    order = np.argsort(-v if WORST_IS_HIGH[metric] else v, kind="stable")
    return [int(i) for i in order[:k]]


# ---------------------------------------------------------------------------------------------------- the scorer
class PairedQuality:
    """score(images, references, region=None, labels=None, ids=None) -> per-image mse, psnr, ssim (and, with a model,
    the perceptual distance) of image i against reference i.

    model: an EDM (the extractor of the perceptual distance) or None (pixel metrics only).  win_size, win_sigma, window:
    the SSIM window ("gaussian" or "uniform").  sigma, taps, seed, batch_size, network_dtype, conditional: the
    FeatureExtractor's, whose defaults (0.1, "mid") nobody has measured on this project's checkpoints; batch_size changes no
    bit of a result.  mean, std: how float32 images in network range map to pixels, pixel = x * std * 2 + mean clamped to
    [0, 1] as the image writer does (default 0.5 and 0.25: x / 2 + 1 / 2, the inverse of the uint8 normalisation)."""

    def __init__(self, model=None, win_size: int = 11, win_sigma: float = 1.5, window: str = "gaussian", sigma: float = 0.1,
                 taps=("mid",), seed: int = 0, batch_size: int = 512, network_dtype: str = "f32x3",
                 conditional: bool = False, mean=None, std=None):
        self.window_name, self.win_size, self.win_sigma = window, win_size, float(win_sigma)
        self.window = make_window(window, win_size, win_sigma)
        self.extractor = None
        if model is not None:
            from .features import FeatureExtractor
            self.extractor = FeatureExtractor(model, sigma=sigma, taps=taps, seed=seed, batch_size=batch_size,
                                              network_dtype=network_dtype, conditional=conditional)
        else:
            check_sigma(sigma, "compare")
            if network_dtype not in NETWORK_DTYPES:
                raise ValueError(f"compare: network_dtype must be one of {NETWORK_DTYPES}, got {network_dtype!r}")
            if conditional:
                raise ValueError("compare: conditional=True needs a model")
        for name, v in (("mean", mean), ("std", std)):
            if v is not None and not all(math.isfinite(float(x)) for x in v):
                raise ValueError(f"compare: {name} must hold finite numbers, got {v}")
        if std is not None and not all(float(x) > 0.0 for x in std):
            raise ValueError(f"compare: std must be > 0, got {std}")
        self.mean, self.std = mean, std
        self.model = model

    # -- operands
    def _device(self):
        if self.model is not None:
            return next(self.model.parameters()).device
        return torch.device("cuda", torch.cuda.current_device())

    def _pair(self, images, references):
        """-> (a, b, is_u8): both uint8 [n, H, W, C] or both float32 [n, C, H, W], on the device"""
        sets = []
        for name, x in (("images", images), ("references", references)):
            if isinstance(x, np.ndarray):
                x = torch.from_numpy(np.ascontiguousarray(x))
            if not isinstance(x, torch.Tensor) or x.dtype not in (torch.uint8, torch.float32) or x.dim() != 4 or x.numel() == 0:
                what = f"{x.dtype} {tuple(x.shape)}" if isinstance(x, torch.Tensor) else type(x).__name__
                raise ValueError(f"compare: {name} must be non-empty uint8 [n, H, W, C] or float32 [n, C, H, W], got {what}")
            sets.append(x)
        a, b = sets
        if a.dtype != b.dtype:
            raise ValueError(f"compare: images are {a.dtype} and references {b.dtype}: mixed dtypes are refused (score both "
                             "as uint8 PNG levels or both as float32 in network range)")
        if a.shape != b.shape:
            raise ValueError(f"compare: images {tuple(a.shape)} and references {tuple(b.shape)} differ in shape")
        is_u8 = a.dtype == torch.uint8
        if is_u8:
            dev = self._device()
            a, b = a.to(dev), b.to(dev)
        else:
            if not (a.is_cuda and b.is_cuda and a.device == b.device):
                raise ValueError("compare: float32 images must be on one GPU")
            if not (bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())):
                raise ValueError("compare: non-finite images")
        H, W = (a.shape[1], a.shape[2]) if is_u8 else (a.shape[2], a.shape[3])
        if self.win_size > min(H, W):
            raise ValueError(f"compare: a window of {self.win_size} taps does not fit {H} x {W} images")
        return a.contiguous(), b.contiguous(), is_u8, H, W

    def _pixels(self, x):
        """float32 network range -> [0, 1] pixels, as the writer maps them"""
        C = x.shape[1]
        mean = (0.5,) * C if self.mean is None else tuple(float(v) for v in self.mean)
        std = (0.25,) * C if self.std is None else tuple(float(v) for v in self.std)
        if len(mean) != C or len(std) != C:
            raise ValueError(f"compare: mean / std must hold {C} values")
        m = torch.tensor(mean, dtype=torch.float32, device=x.device).view(1, -1, 1, 1)
        sd = torch.tensor(std, dtype=torch.float32, device=x.device).view(1, -1, 1, 1)
        return (x * sd * 2.0 + m).clamp(0.0, 1.0).contiguous()

    def _region(self, region, n, H, W, dev):
        if region is None:
            return None
        r = torch.from_numpy(np.ascontiguousarray(region)) if isinstance(region, np.ndarray) else region
        if not isinstance(r, torch.Tensor) or r.dtype not in (torch.uint8, torch.bool) or r.dim() != 3 or \
                r.shape[0] not in (1, n) or tuple(r.shape[1:]) != (H, W):
            what = f"{r.dtype} {tuple(r.shape)}" if isinstance(r, torch.Tensor) else type(r).__name__
            raise ValueError(f"compare: region must be uint8 or bool [{n} or 1, {H}, {W}], got {what}")
        r = r.to(dev).to(torch.uint8).contiguous()
        half = (self.win_size - 1) // 2
        seen = (r[:, half:H - half, half:W - half] != 0).flatten(1).any(dim=1)
        if not bool(seen.all()):
            raise ValueError(f"compare: region row {int(torch.nonzero(~seen)[0])} counts no valid window centre (centres lie "
                             f"at least {half} from every edge): its SSIM would be NaN")
        return r

    @torch.no_grad()
    def score(self, images, references, region=None, labels=None, ids=None) -> dict:
        """images, references: both uint8 [n, H, W, C] (numpy or torch; scored on the integers, L = 255) or both float32
        [n, C, H, W] in network range on the GPU (mapped to [0, 1] pixels and clamped, L = 1).  region: uint8 / bool
        [n or 1, H, W], non-zero = counted (ops.pair_ssim).  labels, ids: the FeatureExtractor's; image i and reference i
        are noised with the same stream (seed, ids[i]).  Returns fp64 tensors on the device: mse [n] (in the units of the
        scored pixels: levels^2 for uint8), psnr [n], ssim [n] (the mean over channels), ssim_channels [n, C], counts int32
        [n, 2], with a model perceptual [n] (the mean over taps) and perceptual_taps [n, T]; and "summary": per metric
        mean, std, median, min, max and "worst", the position of the worst image."""
        from . import ops
        a, b, is_u8, H, W = self._pair(images, references)
        n = a.shape[0]
        region = self._region(region, n, H, W, a.device)
        if is_u8:
            pa, pb, L, C = a, b, 255.0, a.shape[3]
        else:
            pa, pb, L, C = self._pixels(a), self._pixels(b), 1.0, a.shape[1]
        ssim_c, sse, counts = ops.pair_ssim(pa, pb, self.window, L, region)
        npix = counts[:, 0].double() * C
        total = sse.sum(dim=1)
        out = {"mse": total / npix, "psnr": psnr_from_sse(total, npix, L), "ssim": ssim_c.mean(dim=1),
               "ssim_channels": ssim_c, "counts": counts}
        if self.extractor is not None:
            ex = self.extractor
            dist = torch.empty(n, len(ex.taps), dtype=torch.float64, device=a.device)
            for lo, hi, (ma, mb) in ex.tapped_maps(a, b, labels=labels, ids=ids):
                for col, t in enumerate(ex.taps):
                    ops.f32_pair_feature_distance(ma[t], mb[t], dist[lo:hi], col)
            ops.check_health(a.device, "PairedQuality.score")
            out["perceptual_taps"] = dist
            out["perceptual"] = dist.mean(dim=1)
        out["summary"] = {m: {**summarize(out[m]), "worst": worst_indices(out[m], m, 1)[0]} for m in METRICS if m in out}
        return out


def report_rows(scores, indices) -> list:
    """the per-image rows of a report: one dict per image, in order"""
    cols = {m: scores[m].cpu().tolist() for m in METRICS if m in scores}
    ch = scores["ssim_channels"].cpu().tolist()
    taps = scores["perceptual_taps"].cpu().tolist() if "perceptual_taps" in scores else None
    rows = []
    for i, idx in enumerate(indices):
        row = {"index": int(idx), **{m: v[i] for m, v in cols.items()}, "ssim_channels": ch[i]}
        if taps is not None:
            row["perceptual_taps"] = taps[i]
        rows.append(row)
    return rows


def worst_table(scores, indices, k: int) -> dict:
    """per metric the `index` of the k worst images, the worst first"""
    return {m: [int(indices[i]) for i in worst_indices(scores[m], m, k)] for m in METRICS if m in scores}


# ---------------------------------------------------------------------------------------------------- command line
def png_indices(image_dir, where) -> list:
    """the indices of the <index>.png files of a directory, ascending"""
    names = [f for f in os.listdir(image_dir) if f.lower().endswith(".png")]
    bad = [f for f in names if not os.path.splitext(f)[0].isdigit()]
    if bad:
        raise ValueError(f"compare: {where} holds PNGs that are not named <index>.png: {sorted(bad)[:3]}")
    if not names:
        raise ValueError(f"compare: no PNG in {image_dir}")
    idx = sorted(int(os.path.splitext(f)[0]) for f in names)
    if len(set(idx)) != len(idx):
        raise ValueError(f"compare: {where} names an index twice (as in 7.png and 07.png)")
    return idx


def read_pairs(image_dir, ref_image_dir):
    """the two directories paired by their <index>.png names -> (indices, images uint8 [n, H, W, C], references the
    same).  Index sets that differ are refused, the first missing index named."""
    from .neighbors import read_png_dir
    ia, ib = png_indices(image_dir, "--image_dir"), png_indices(ref_image_dir, "--ref_image_dir")
    if ia != ib:
        only_a, only_b = sorted(set(ia) - set(ib)), sorted(set(ib) - set(ia))
        if only_a:
            raise ValueError(f"compare: {only_a[0]}.png is in --image_dir but missing from --ref_image_dir "
                             f"({len(only_a)} such, {len(only_b)} the other way)")
        raise ValueError(f"compare: {only_b[0]}.png is in --ref_image_dir but missing from --image_dir ({len(only_b)} such)")
    a = np.stack(read_png_dir(image_dir, "compare", "--image_dir"))
    b = np.stack(read_png_dir(ref_image_dir, "compare", "--ref_image_dir", a.shape[1:3], a.shape[3]))
    return ia, a, b


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Paired image quality: MSE, PSNR, SSIM and (with a checkpoint) a denoiser-"
                                            "feature distance of <index>.png against <index>.png")
    p.add_argument("--image_dir", type=str, required=True, help="directory of <index>.png images (as generate writes them)")
    p.add_argument("--ref_image_dir", type=str, required=True, help="the originals, paired by index")
    p.add_argument("--ckpt_path", type=str, default=None, help="the extractor of the perceptual distance (none: pixel metrics)")
    p.add_argument("--load_ema", action="store_true", help="use the EMA weights of the checkpoint")
    p.add_argument("--sigma", type=float, default=None, help="the noise level the activations are taken at (default 0.1)")
    p.add_argument("--taps", type=str, nargs="+", default=None, help='block outputs: "enc<i>", "dec<i>" or "mid" (default mid)')
    p.add_argument("--seed", type=int, default=None, help="the noise seed (default 0)")
    p.add_argument("--network_dtype", type=str, default=None, help="f32x3 (default) or f32")
    p.add_argument("--batch_size", type=int, default=512)
    p.add_argument("--region_box", type=int, nargs=4, metavar=("X0", "Y0", "X1", "Y1"), default=None,
                   help="score only X0 <= x < X1, Y0 <= y < Y1 (an inpainted box)")
    p.add_argument("--win_size", type=int, default=11, help=f"SSIM window taps, odd, 3 .. {MAX_WIN} (default 11)")
    p.add_argument("--win_sigma", type=float, default=1.5, help="standard deviation of the Gaussian window (default 1.5)")
    p.add_argument("--window", type=str, default="gaussian", help="gaussian (default) or uniform")
    p.add_argument("--worst", type=int, default=10, metavar="K", help="list the K worst images per metric (default 10)")
    p.add_argument("--report", type=str, required=True, metavar="QUALITY.json")
    return p


def check_args(args) -> None:
    """every choice that needs nothing loaded, checked before a file, a checkpoint or the GPU is touched"""
    make_window(args.window, args.win_size, args.win_sigma)
    if args.ckpt_path is None:
        for flag in ("sigma", "taps", "seed", "network_dtype"):
            if getattr(args, flag) is not None:
                raise ValueError(f"compare: --{flag} belongs to the perceptual distance, which needs --ckpt_path")
        if args.load_ema:
            raise ValueError("compare: --load_ema needs --ckpt_path")
    else:
        if args.network_dtype is not None and args.network_dtype not in NETWORK_DTYPES:
            raise ValueError(f"compare: --network_dtype must be one of {NETWORK_DTYPES}, got {args.network_dtype!r}")
        if args.sigma is not None:
            check_sigma(args.sigma, "compare: --sigma")
        if args.seed is not None and (isinstance(args.seed, bool) or not isinstance(args.seed, int)
                                      or not 0 <= args.seed < 1 << 64):
            raise ValueError(f"compare: --seed must be in [0, 2**64), got {args.seed!r}")
        if args.taps is not None and len(set(args.taps)) != len(args.taps):
            raise ValueError(f"compare: --taps names a tap twice: {args.taps}")
    for flag in ("batch_size", "worst"):
        v = getattr(args, flag)
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"compare: --{flag} must be an integer >= 1, got {v!r}")
    if args.region_box is not None:
        x0, y0, x1, y1 = args.region_box
        if not (0 <= x0 < x1 and 0 <= y0 < y1):
            raise ValueError(f"compare: --region_box X0 Y0 X1 Y1 needs 0 <= X0 < X1 and 0 <= Y0 < Y1, got {args.region_box}")
    if os.path.abspath(args.image_dir) == os.path.abspath(args.ref_image_dir):
        raise ValueError("compare: --image_dir and --ref_image_dir are the same directory")


def run(args) -> dict:
    """read the pairs, score them, write --report; returns the report"""
    indices, images, refs = read_pairs(args.image_dir, args.ref_image_dir)
    H, W = images.shape[1:3]
    if args.win_size > min(H, W):
        raise ValueError(f"compare: --win_size {args.win_size} does not fit {H} x {W} images")
    region = None if args.region_box is None else region_from_box(args.region_box, H, W, args.win_size)
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dev = torch.device("cuda", torch.cuda.current_device())
    model = None
    perceptual = {}
    if args.ckpt_path is not None:
        from .features import _load_model
        model = _load_model(args.ckpt_path, args.load_ema, dev)
        perceptual = {"sigma": 0.1 if args.sigma is None else args.sigma, "taps": tuple(args.taps or ("mid",)),
                      "seed": args.seed or 0, "network_dtype": args.network_dtype or "f32x3"}
    pq = PairedQuality(model, win_size=args.win_size, win_sigma=args.win_sigma, window=args.window,
                       batch_size=args.batch_size, **perceptual)
    scores = pq.score(images, refs, region=region, ids=np.asarray(indices, dtype=np.int64))
    report = {"settings": {"image_dir": args.image_dir, "ref_image_dir": args.ref_image_dir, "num_images": len(indices),
                           "image_shape": [int(H), int(W), int(images.shape[3])], "data_range": 255,
                           "window": args.window, "win_size": args.win_size, "win_sigma": args.win_sigma,
                           "region_box": args.region_box, "ckpt_path": args.ckpt_path, "load_ema": bool(args.load_ema),
                           **{k: (list(v) if isinstance(v, tuple) else v) for k, v in perceptual.items()}},
              "summary": scores["summary"], "images": report_rows(scores, indices),
              "worst": worst_table(scores, indices, args.worst)}
    with open(args.report, "w") as f:
        json.dump(report, f, indent=1)
    for m, s in scores["summary"].items():
        print(f"{m:>10s}: mean {s['mean']:.6g}  median {s['median']:.6g}  min {s['min']:.6g}  max {s['max']:.6g}  "
              f"worst {indices[s['worst']]}.png")
    print(f"wrote {args.report}", flush=True)
    return report


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        check_args(args)
    except ValueError as e:
        parser.error(str(e))
    return run(args)


if __name__ == "__main__":
    main()
