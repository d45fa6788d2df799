"""Loss by noise level: the denoising error of held-out images at a fixed set of noise levels with fixed noise (Karras et
al. 2022, Sec. 5 / Fig. 5a; Karras et al. 2024, Sec. 2 and 3).  A deterministic number that tells two checkpoints apart:

    python -m tinyedm.evaluate --ckpt_path ema_0.05.ckpt ema_0.10.ckpt ema_0.15.ckpt --dataset cifar10 \\
        --data_dir datasets/cifar --report loss.json

`val_loss` draws a fresh sigma and fresh noise for every batch; here every image meets every level, and the noise of an
(image, level, draw) is a function of the seed alone (ops.eval_diffuse: the Philox counter holds the image's id, not its
row in a batch), so the same checkpoint gives the same bits whatever the batch size, the order or the number of ranks.
The squared errors are summed in fp64 in a fixed order on the device (ops.eval_sqerr) into one [draws, levels, images]
matrix, copied to the host once, and reduced there in id order.

Levels.  Without `--sigmas` the L levels are the quantile midpoints of the training distribution ln sigma ~ N(P_mean,
P_std): sigma_l = exp(P_mean + P_std * Phi^-1((l + 1/2) / L)).  Each level then stands for an equal share of the
training draws, and the plain mean over the levels of lambda(sigma_l) * mse_l is a stratified estimate of the expected
training loss E_sigma[lambda(sigma) * mse(sigma)], reported as `expected_loss`.  Explicit levels have no such reading:
`expected_loss` is None and checkpoints are ranked by the mean of `loss` over the levels given.

Under torch.distributed each rank evaluates the images with id = rank (mod world) and the per-level (count, sum, sum of
squares) are merged with one fp64 all-reduce (`merge_level_sums` is the same merge on the host)."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics

import numpy as np
import torch

NETWORK_DTYPES = ("bf16", "f32x3", "f32")
MAX_LEVELS = 65535              # ops.EVAL_MAX_LEVELS: a level is the low half of the Philox tag


# ---------------------------------------------------------------------------------------------------- host arithmetic
def level_sigmas(P_mean: float, P_std: float, num_levels: int) -> list:
    """the quantile midpoints of ln sigma ~ N(P_mean, P_std): sigma_l = exp(P_mean + P_std * Phi^-1((l + 1/2) / L))"""
    if isinstance(num_levels, bool) or not isinstance(num_levels, int) or not 1 <= num_levels <= MAX_LEVELS:
        raise ValueError(f"evaluate: num_levels must be an integer in [1, {MAX_LEVELS}], got {num_levels!r}")
    P_mean, P_std = float(P_mean), float(P_std)
    if not (math.isfinite(P_mean) and math.isfinite(P_std) and P_std > 0.0):
        raise ValueError(f"evaluate: P_mean must be finite and P_std finite and > 0, got {P_mean}, {P_std}")
    inv = statistics.NormalDist().inv_cdf
    return [math.exp(P_mean + P_std * inv((l + 0.5) / num_levels)) for l in range(num_levels)]


def check_sigmas(sigmas) -> list:
    """explicit levels as a list of floats: 1 to 65 535 of them, positive, finite, strictly increasing (also once rounded
    to the fp32 the kernels read)"""
    if isinstance(sigmas, torch.Tensor):
        sigmas = sigmas.detach().cpu().flatten().tolist()
    try:
        out = [float(s) for s in sigmas]
    except (TypeError, ValueError):
        raise ValueError(f"evaluate: sigmas must be a sequence of numbers, got {sigmas!r}") from None
    if not 1 <= len(out) <= MAX_LEVELS:
        raise ValueError(f"evaluate: between 1 and {MAX_LEVELS} sigmas are needed, got {len(out)}")
    if not all(math.isfinite(s) and s > 0.0 for s in out):
        raise ValueError(f"evaluate: sigmas must be finite and > 0, got {out}")
    f32 = [float(np.float32(s)) for s in out]
    if not all(0.0 < a < b and math.isfinite(b) for a, b in zip(f32, f32[1:])) or not 0.0 < f32[0] < math.inf:
        raise ValueError(f"evaluate: sigmas must be strictly increasing (as fp32), got {out}")
    return out


def edm_weight(sigma: float, sigma_data: float) -> float:
    """lambda(sigma) = (sigma^2 + sigma_data^2) / (sigma * sigma_data)^2, the weighting of the training loss"""
    return (sigma * sigma + sigma_data * sigma_data) / (sigma * sigma_data) ** 2


def level_sums(se, chw: int) -> np.ndarray:
    """se: fp64 [draws, L, n] summed squared errors, the images in id order -> fp64 [3, L]: (count, sum, sum of squares)
    over the images of v_i = mean over the draws of se_i / chw, each sum taken sequentially in id order"""
    se = np.asarray(se, dtype=np.float64)
    if se.ndim != 3 or se.shape[0] < 1 or int(chw) < 1:
        raise ValueError(f"level_sums: expected a [draws, L, n] matrix and chw >= 1, got {se.shape}, {chw}")
    v = se.mean(axis=0) / float(chw)                       # [L, n]
    out = np.zeros((3, se.shape[1]), dtype=np.float64)
    out[0] = float(se.shape[2])
    if se.shape[2]:
        out[1] = np.cumsum(v, axis=1)[:, -1]
        out[2] = np.cumsum(v * v, axis=1)[:, -1]
    return out


def merge_level_sums(parts) -> np.ndarray:
    """the (count, sum, sum of squares) of several shards of the images -> those of their union: fp64 [3, L]"""
    parts = [np.asarray(p, dtype=np.float64) for p in parts]
    if not parts or any(p.ndim != 2 or p.shape != parts[0].shape or p.shape[0] != 3 for p in parts):
        raise ValueError("merge_level_sums: expected one or more [3, L] arrays of one shape")
    out = np.zeros_like(parts[0])
    for p in parts:
        out = out + p
    return out


def level_stats(sums, sigmas, sigma_data: float) -> dict:
    """(count, sum, sum of squares) [3, L] -> the per-level report: sigma, count, mse, mse_stderr (the standard error of
    the mean over the images; None below two images) and loss = lambda(sigma) * mse"""
    sums = np.asarray(sums, dtype=np.float64)
    sigmas = [float(s) for s in sigmas]
    if sums.shape != (3, len(sigmas)):
        raise ValueError(f"level_stats: expected sums of shape {(3, len(sigmas))}, got {sums.shape}")
    out = {"sigma": sigmas, "count": [], "mse": [], "mse_stderr": [], "loss": []}
    for l, s in enumerate(sigmas):
        n, s1, s2 = float(sums[0, l]), float(sums[1, l]), float(sums[2, l])
        if n < 1:
            raise ValueError("level_stats: no image was evaluated")
        mse = s1 / n
        out["count"].append(int(n))
        out["mse"].append(mse)
        out["mse_stderr"].append(math.sqrt(max(s2 - s1 * s1 / n, 0.0) / (n - 1.0) / n) if n >= 2 else None)
        out["loss"].append(edm_weight(s, float(sigma_data)) * mse)
    return out


def check_images(images, labels, ids, who: str = "evaluate"):
    """the operands of an evaluation -> (contiguous fp32 NCHW images on the GPU, labels [N] on their device or None,
    ids as int64 [N] on the host: given, or 0 .. N - 1)"""
    if not isinstance(images, torch.Tensor) or not images.is_cuda or images.dtype != torch.float32 or images.dim() != 4:
        raise ValueError(f"{who}: images must be an fp32 NCHW tensor on the GPU")
    N, dev = images.shape[0], images.device
    if N == 0 or images[0].numel() == 0:
        raise ValueError(f"{who}: no images")
    images = images.contiguous()
    ids_h = np.arange(N, dtype=np.int64) if ids is None else np.asarray(
        ids.detach().cpu() if isinstance(ids, torch.Tensor) else ids).astype(np.int64).reshape(-1)
    if ids_h.shape[0] != N or ids_h.min() < 0 or ids_h.max() >= 1 << 32 or np.unique(ids_h).shape[0] != N:
        raise ValueError(f"{who}: ids must be {N} distinct integers in [0, 2**32)")
    if labels is not None:
        if not isinstance(labels, torch.Tensor) or labels.numel() != N:
            raise ValueError(f"{who}: labels must be a tensor of {N} class indices")
        labels = labels.to(dev).reshape(N)
    return images, labels, ids_h


# ---------------------------------------------------------------------------------------------------- the evaluator
class NoiseLevelEvaluator:
    """evaluate(model, images, labels=None, ids=None) -> the per-level denoising error of `images` (see the module text).

    sigmas: explicit levels (list or tensor), or None for `num_levels` quantile midpoints of N(P_mean, P_std), with
    P_mean / P_std defaulting to the model's diffuser.  seed and num_draws select the noise: draw d of image id at level l
    is the stream (seed, d, id, l).  batch_size is the number of (image, level) pairs per network call; it changes no
    bit of the result.  network_dtype is the evaluation precision of an EDM's denoiser ("bf16", "f32x3" or "f32").
    sigma_data is used for lambda(sigma) when the model has no `sigma_data` attribute (a plain callable)."""

    def __init__(self, sigmas=None, num_levels: int = 16, P_mean=None, P_std=None, seed: int = 0, num_draws: int = 1,
                 batch_size: int = 512, network_dtype: str = "bf16", sigma_data: float = 0.5):
        self.sigmas = None if sigmas is None else check_sigmas(sigmas)
        if self.sigmas is None:
            level_sigmas(0.0, 1.0, num_levels)                      # (validates num_levels)
            for name, v in (("P_mean", P_mean), ("P_std", P_std)):
                if v is not None and not math.isfinite(float(v)):
                    raise ValueError(f"evaluate: {name} must be finite, got {v}")
            if P_std is not None and float(P_std) <= 0.0:
                raise ValueError(f"evaluate: P_std must be > 0, got {P_std}")
        self.num_levels = num_levels if self.sigmas is None else len(self.sigmas)
        self.P_mean, self.P_std = P_mean, P_std
        for name, v, lo, hi in (("seed", seed, 0, 1 << 64), ("num_draws", num_draws, 1, 1 << 16),
                                ("batch_size", batch_size, 1, 65536)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v < hi:
                raise ValueError(f"evaluate: {name} must be an integer in [{lo}, {hi}), got {v!r}")
        self.seed, self.num_draws, self.batch_size = seed, num_draws, batch_size
        if network_dtype not in NETWORK_DTYPES:
            raise ValueError(f"evaluate: network_dtype must be one of {NETWORK_DTYPES}, got {network_dtype!r}")
        self.network_dtype = network_dtype
        if not (math.isfinite(float(sigma_data)) and float(sigma_data) > 0.0):
            raise ValueError(f"evaluate: sigma_data must be finite and > 0, got {sigma_data}")
        self.sigma_data = float(sigma_data)

    def levels_for(self, model) -> list:
        """the levels this evaluator uses on `model` (fp64; the kernels read them rounded to fp32)"""
        if self.sigmas is not None:
            return list(self.sigmas)
        d = getattr(model, "diffuser", None)
        P_mean = self.P_mean if self.P_mean is not None else getattr(d, "P_mean", None)
        P_std = self.P_std if self.P_std is not None else getattr(d, "P_std", None)
        if P_mean is None or P_std is None:
            raise ValueError("evaluate: the training-distribution levels need P_mean and P_std (the model has no diffuser)")
        return check_sigmas(level_sigmas(P_mean, P_std, self.num_levels))

    @torch.no_grad()
    def evaluate(self, model, images, labels=None, ids=None) -> dict:
        from . import ops
        from .callbacks import _eval_dtype
        images, labels, ids_h = check_images(images, labels, ids)
        N, dev = images.shape[0], images.device
        sigmas = [float(np.float32(s)) for s in self.levels_for(model)]     # what the kernel and the network see
        L, R, chw = len(sigmas), self.num_draws, images[0].numel()
        sigma_data = float(getattr(model, "sigma_data", self.sigma_data))

        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank() if world > 1 else 0
        order = np.argsort(ids_h, kind="stable")                  # id order
        if world > 1:
            order = order[ids_h[order] % world == rank]
        n = int(order.shape[0])
        sums = np.zeros((3, L), dtype=np.float64)
        se_h = torch.zeros(R, L, 0, dtype=torch.float64)
        if n:
            # the work list, level-major, built and checked on the host, uploaded once: item t = (level t // n, image t % n)
            total = L * n
            item_img = torch.from_numpy(np.tile(order, L)).to(dev)
            item_ids = torch.from_numpy(np.tile(ids_h[order].astype(np.uint32), L)).to(dev)
            item_level = torch.from_numpy(np.repeat(np.arange(L, dtype=np.int32), n)).to(dev)
            sig_dev = torch.tensor(sigmas, dtype=torch.float32, device=dev)
            se = torch.empty(R, L, n, dtype=torch.float64, device=dev)
            is_module = isinstance(model, torch.nn.Module)
            was_training = is_module and model.training
            if is_module:
                model.eval()
            try:
                with _eval_dtype(model, self.network_dtype):
                    for d in range(R):
                        rec = ops.churn_record(self.seed, d, dev)
                        flat = se[d].view(-1)
                        for t0 in range(0, total, self.batch_size):
                            t1 = min(total, t0 + self.batch_size)
                            idx = item_img[t0:t1]
                            clean = images.index_select(0, idx)
                            noisy, sigma = ops.eval_diffuse(clean, item_ids[t0:t1], item_level[t0:t1], sig_dev, rec,
                                                            check_levels=False)     # (levels built above: 0 .. L - 1)
                            D = model(noisy, sigma, None if labels is None else labels.index_select(0, idx))
                            if tuple(D.shape) != tuple(clean.shape):
                                raise ValueError(f"evaluate: the model returned {tuple(D.shape)} for {tuple(clean.shape)}")
                            ops.eval_sqerr(D.float().contiguous(), clean, out=flat[t0:t1])
            finally:
                if was_training:
                    model.train()
            se_h = se.cpu()                                         # the one device -> host copy
            ops.check_health(dev, "NoiseLevelEvaluator.evaluate")
            sums = level_sums(se_h.numpy(), chw)
        if world > 1:
            t = torch.from_numpy(sums).to(dev)
            dist.all_reduce(t)
            sums = t.cpu().numpy()
        out = level_stats(sums, sigmas, sigma_data)
        out["sums"] = sums.tolist()
        out["expected_loss"] = None if self.sigmas is not None else math.fsum(out["loss"]) / L
        out["mean_loss"] = math.fsum(out["loss"]) / L
        out.update(num_draws=R, seed=self.seed, network_dtype=self.network_dtype, sigma_data=sigma_data,
                   ids=ids_h[order].tolist(), se=se_h)
        u = getattr(model, "u", None)
        if u is not None:
            four, _ = model.embedding(torch.tensor(sigmas, dtype=torch.float32, device=dev), None)
            out["uncertainty"] = u(four).flatten().double().cpu().tolist()
        return out


def report_entry(result: dict) -> dict:
    """the JSON-serialisable part of an evaluate() result (without the se matrix and the id list)"""
    return {k: v for k, v in result.items() if k not in ("se", "ids")}


def best_checkpoint(entries: dict):
    """(name, criterion) of the entry with the lowest expected_loss, or, with explicit levels, the lowest mean loss"""
    if not entries:
        raise ValueError("best_checkpoint: no entries")
    key = "expected_loss" if all(e.get("expected_loss") is not None for e in entries.values()) else "mean_loss"
    return min(entries, key=lambda k: entries[k][key]), key


# ---------------------------------------------------------------------------------------------------- command line
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Denoising loss by noise level of one or more checkpoints on held-out images")
    p.add_argument("--ckpt_path", type=str, nargs="+", required=True, help="one or more checkpoints to compare")
    p.add_argument("--load_ema", action="store_true", help="evaluate the EMA weights of the checkpoints")
    p.add_argument("--dataset", choices=["cifar10", "mnist"], default=None, help="built-in test split (with --data_dir)")
    p.add_argument("--data_dir", type=str, default=None)
    p.add_argument("--image_dir", type=str, default=None, help="directory of <index>.png images (as generate writes them)")
    p.add_argument("--labels_json", type=str, default=None,
                   help="--image_dir with a conditional model: a JSON list of class indices, one per image in index order")
    p.add_argument("--mean", type=float, nargs="+", default=None)
    p.add_argument("--std", type=float, nargs="+", default=None)
    p.add_argument("--image_size", type=int, default=None)
    p.add_argument("--in_channels", type=int, default=None)
    p.add_argument("--num_levels", type=int, default=16, help="levels at the quantile midpoints of the training distribution")
    p.add_argument("--sigmas", type=float, nargs="+", default=None, help="explicit levels, strictly increasing")
    p.add_argument("--num_images", type=int, default=1024)
    p.add_argument("--num_draws", type=int, default=1)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--batch_size", type=int, default=512)
    p.add_argument("--network_dtype", choices=list(NETWORK_DTYPES), default="bf16")
    p.add_argument("--report", type=str, required=True, metavar="OUT.json")
    return p


def check_data_args(args, who: str = "evaluate") -> None:
    """the data, label and checkpoint flags, which need nothing loaded"""
    if (args.dataset is None) == (args.image_dir is None):
        raise ValueError(f"{who}: give exactly one data source: --dataset cifar10|mnist --data_dir DIR, or --image_dir DIR")
    if args.dataset is not None:
        if args.data_dir is None:
            raise ValueError(f"{who}: --dataset needs --data_dir")
        for flag in ("labels_json", "mean", "std", "image_size", "in_channels"):
            if getattr(args, flag) is not None:
                raise ValueError(f"{who}: --{flag} goes with --image_dir (the built-in datasets carry their own)")
    else:
        if args.data_dir is not None:
            raise ValueError(f"{who}: --data_dir goes with --dataset")
        if args.image_size is None or args.image_size < 1:
            raise ValueError(f"{who}: --image_dir needs --image_size")
        if (args.mean is None) != (args.std is None):
            raise ValueError(f"{who}: --mean and --std go together")
        if args.in_channels is not None and args.in_channels < 1:
            raise ValueError(f"{who}: --in_channels must be >= 1, got {args.in_channels}")
        if args.mean is not None and args.in_channels is not None and not (
                len(args.mean) == len(args.std) == args.in_channels):
            raise ValueError(f"{who}: --mean and --std need one value per channel")
    if isinstance(args.num_images, bool) or not isinstance(args.num_images, int) or args.num_images < 1:
        raise ValueError(f"{who}: --num_images must be an integer >= 1, got {args.num_images!r}")
    if len(set(args.ckpt_path)) != len(args.ckpt_path):
        raise ValueError(f"{who}: --ckpt_path names a checkpoint twice")


def check_args(args) -> NoiseLevelEvaluator:
    """every choice that needs nothing loaded, checked before a checkpoint or the GPU is touched; returns the evaluator"""
    check_data_args(args)
    return NoiseLevelEvaluator(sigmas=args.sigmas, num_levels=args.num_levels, seed=args.seed, num_draws=args.num_draws,
                               batch_size=args.batch_size, network_dtype=args.network_dtype)


def _load_data(args, model, dev, who: str = "evaluate"):
    """(images fp32 NCHW on dev, labels or None): the first --num_images of the source"""
    from . import ops
    if args.dataset is not None:
        from .datamodules import read_cifar10, read_mnist
        x, y = (read_cifar10 if args.dataset == "cifar10" else read_mnist)(args.data_dir, False)
        n = min(args.num_images, x.shape[0])
        data = torch.from_numpy(np.ascontiguousarray(x[:n])).to(dev)
        images = ops.u8_gather_normalize(data, torch.arange(n, device=dev), 0.5, 0.5)    # as the datamodules deliver it
        return images, torch.from_numpy(np.asarray(y[:n], dtype=np.int64)).to(dev)
    from .generate import CIFAR_MEAN, CIFAR_STD, load_images
    C = int(args.in_channels) if args.in_channels is not None else int(model.denoiser.in_channels)
    mean, std = (args.mean, args.std) if args.mean is not None else (
        (CIFAR_MEAN, CIFAR_STD) if C == 3 else ((0.5,) * C, (0.25,) * C))
    images = load_images(args.image_dir, mean, std, args.image_size, C)[:args.num_images]
    labels = None
    if args.labels_json is not None:
        with open(args.labels_json) as f:
            labels = json.load(f)
        if not isinstance(labels, list) or len(labels) < images.shape[0] or not all(
                isinstance(v, int) and not isinstance(v, bool) and v >= 0 for v in labels):
            raise ValueError(f"{who}: --labels_json must hold a list of at least {images.shape[0]} class indices")
        labels = torch.tensor(labels[:images.shape[0]], dtype=torch.int64, device=dev)
    return images.to(dev), labels


def format_table(entries: dict) -> str:
    names = list(entries)
    first = entries[names[0]]
    lines = ["level      sigma  " + "  ".join(f"{'loss[' + str(i) + ']':>12s} {'mse[' + str(i) + ']':>12s}"
                                            for i in range(len(names)))]
    for l, s in enumerate(first["sigma"]):
        lines.append(f"{l:5d} {s:10.4g}  " + "  ".join(f"{entries[k]['loss'][l]:12.6g} {entries[k]['mse'][l]:12.6g}"
                                                       for k in names))
    for i, k in enumerate(names):
        e = entries[k]
        tail = f"expected_loss {e['expected_loss']:.6g}" if e["expected_loss"] is not None else f"mean loss {e['mean_loss']:.6g}"
        lines.append(f"[{i}] {k}: {tail}")
    return "\n".join(lines)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        evaluator = check_args(args)
    except ValueError as e:
        parser.error(str(e))
    from .edm import EDM
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dev = torch.device("cuda", torch.cuda.current_device())
    entries, levels, data = {}, None, None
    for path in args.ckpt_path:
        model = EDM.load_from_checkpoint(path, load_ema=args.load_ema).to(dev).eval()
        if data is None:
            data = _load_data(args, model, dev)
        images, labels = data
        if model.conditional and labels is None:
            print(f"evaluate: {path} is class-conditional and no labels were given: evaluated label-free", flush=True)
        res = evaluator.evaluate(model, images, labels if model.conditional else None)
        if levels is not None and res["sigma"] != levels:
            raise ValueError(f"evaluate: {path} has another training distribution (P_mean / P_std) than the first "
                             "checkpoint; compare them at explicit --sigmas")
        levels = res["sigma"]
        entries[path] = report_entry(res)
        del model
    best, key = best_checkpoint(entries)
    report = {"sigmas": levels, "num_images": int(data[0].shape[0]), "num_draws": args.num_draws, "seed": args.seed,
              "network_dtype": args.network_dtype, "load_ema": bool(args.load_ema), "checkpoints": entries,
              "best": best, "criterion": key}
    if int(os.environ.get("RANK", "0")) == 0:
        with open(args.report, "w") as f:
            json.dump(report, f, indent=1)
        print(format_table(entries))
        if len(entries) > 1:
            how = "expected_loss" if key == "expected_loss" else "mean loss over the explicit levels (no expected_loss)"
            print(f"lowest {how}: {best} ({entries[best][key]:.6g})")
        print(f"wrote {args.report}", flush=True)
    return report


if __name__ == "__main__":
    main()
