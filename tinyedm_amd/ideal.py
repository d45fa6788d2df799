"""The ideal denoiser of a training set, and how far a network is from it.

The minimiser of the EDM training loss on a finite training set is known in closed form (Karras et al. 2022, App. B.3,
eq. 57): D*(x; sigma) = sum_i w_i y_i with w = softmax_i(-|x - y_i|^2 / (2 sigma^2)) over the training images y_i.
`IdealDenoiser` evaluates it on the GPU (csrc/ideal.hip: both products on the fp32 matrix pipe against the resident uint8
set) as a plain callable `ideal(x, sigma, class_labels)`, which every solver here and `NoiseLevelEvaluator` accept in place
of a network.  From it come the exact floor of the training loss at each noise level, the distance of a network's output
to the memorising optimum, the effective number of training images that explain a noisy input (exp of the entropy of w)
and the exact log density of the noised empirical distribution.

    python -m tinyedm.ideal --dataset cifar10 --data_dir datasets/cifar --ckpt_path last.ckpt --load_ema \\
        --num_images 1024 --report gap.json

reports, per noise level of `tinyedm.evaluate` and with its fixed noise, `ideal_train_mse` (the floor), `ideal_test_mse`,
the mean effective count on both sets and, per checkpoint, `train_mse`, `test_mse`, `excess_train = train_mse -
ideal_train_mse` and `to_ideal_train` / `to_ideal_test` = mean |D_net - D*|^2 / K at the same noisy inputs, each also
weighted by lambda(sigma).  Without `--ckpt_path` the report holds the ideal columns only.

    python -m tinyedm.ideal --dataset cifar10 --data_dir datasets/cifar --samples 64 --output_dir ideal_samples

samples from D* with the solvers (`--solver heun|dpmpp`, `--S_churn`, `--num_steps`, `--seed`), writes `<index>.png` as
generate does and `top_index.json`, the training image each sample ended on: with a sound solver the PNGs are training images.
"""
from __future__ import annotations

import argparse
import json
import math
import os

import numpy as np

MAX_K = 32768               # ops.IDEAL_MAX_K, repeated here so that the host checks need no GPU library
MAX_R = 2 ** 31 - 128       # ops.IDEAL_MAX_R
SOLVERS = ("heun", "dpmpp")


# ---------------------------------------------------------------------------------------------------- host arithmetic
def check_sigma(sigma) -> float:
    """a noise level given as a Python number: finite and > 0"""
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)):
        raise ValueError(f"ideal: sigma must be a number or a tensor, got {sigma!r}")
    s = float(sigma)
    with np.errstate(over="ignore"):
        f = float(np.float32(s))            # what the kernel reads
    if not (math.isfinite(s) and s > 0.0 and math.isfinite(f) and f > 0.0):
        raise ValueError(f"ideal: sigma must be finite and > 0 (also as fp32), got {sigma!r}")
    return s


def check_set(shape, dtype_is_u8: bool, labels, mean, std, sigma_data, num_classes, ref_chunk):
    """everything about a training set that needs no device: the shape and dtype of the images, the labels, the
    normalisation and the chunk length -> (labels as int32 [R] or None, num_classes or None, images per class or None)"""
    if not dtype_is_u8:
        raise ValueError("IdealDenoiser: data_u8 must be uint8 (the bytes the datamodules hold)")
    shape = tuple(int(v) for v in shape)
    if len(shape) != 4:
        raise ValueError(f"IdealDenoiser: data_u8 must be [R, C, H, W], got {shape}")
    R, K = shape[0], int(np.prod(shape[1:]))
    if R < 1 or K < 1:
        raise ValueError(f"IdealDenoiser: the training set is empty: {shape}")
    if K > MAX_K or R > MAX_R:
        raise ValueError(f"IdealDenoiser: at most {MAX_K} elements per image and 2^31 - 128 images, got {shape}")
    for name, v in (("mean", mean), ("std", std), ("sigma_data", sigma_data)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)):
            raise ValueError(f"IdealDenoiser: {name} must be a finite number (one value for all channels), got {v!r}")
    if float(std) <= 0.0 or float(sigma_data) <= 0.0:
        raise ValueError(f"IdealDenoiser: std and sigma_data must be > 0, got {std}, {sigma_data}")
    if ref_chunk is not None and (isinstance(ref_chunk, bool) or not isinstance(ref_chunk, int) or ref_chunk < 1):
        raise ValueError(f"IdealDenoiser: ref_chunk must be None or an integer >= 1, got {ref_chunk!r}")
    if labels is None:
        if num_classes is not None:
            raise ValueError("IdealDenoiser: num_classes goes with labels")
        return None, None, None
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.shape[0] != R or lab.dtype.kind not in "iu":
        raise ValueError(f"IdealDenoiser: labels must be {R} integer class indices, got {lab.dtype} {lab.shape}")
    lab = lab.astype(np.int64)
    if num_classes is None:
        num_classes = int(lab.max()) + 1
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes < 2 ** 31:
        raise ValueError(f"IdealDenoiser: num_classes must be an integer in [1, 2^31), got {num_classes!r}")
    if lab.min() < 0 or lab.max() >= num_classes:
        raise ValueError(f"IdealDenoiser: labels must lie in [0, {num_classes}), got [{lab.min()}, {lab.max()}]")
    counts = np.bincount(lab, minlength=num_classes)
    if (counts == 0).any():
        raise ValueError(f"IdealDenoiser: class {int(np.argmin(counts != 0))} owns no image: its softmax would be empty")
    return lab.astype(np.int32), num_classes, counts


def log_density(lse, n_refs, K: int, sigma):
    """lse - log R' - (K / 2) log(2 pi sigma^2) in fp64: the exact log density (nats) of the noised empirical
    distribution (the mixture of R' Gaussians N(y_i, sigma^2 I)) at the query"""
    sigma = np.asarray(sigma, dtype=np.float64)
    return (np.asarray(lse, dtype=np.float64) - np.log(np.asarray(n_refs, dtype=np.float64))
            - 0.5 * float(K) * np.log(2.0 * math.pi * sigma * sigma))


# ---------------------------------------------------------------------------------------------------- the denoiser
class IdealDenoiser:
    """D*(x; sigma) of a uint8 training set as a plain callable (deliberately not an nn.Module: it has no parameters, no
    modes and no state a checkpoint could hold).  data_u8: uint8 [R, C, H, W], numpy or torch, moved to `device` once
    and kept as uint8; y = (u / 255 - mean) / std with one mean and std for all channels.  labels: one class index per
    image; every class in range(num_classes) must own an image.  The set stays in the caller's order (the class
    restriction is a label compare in the kernel), so `top_index` is an index into data_u8 and a label-free call on a
    labelled set is the unlabelled computation bit for bit.  The references are walked ref_chunk rows at a time (None:
    ops.IDEAL_REF_CHUNK); with ref_chunk fixed the bits of an output row depend on (x, sigma, class) of that row alone."""

    def __init__(self, data_u8, labels=None, *, mean=0.5, std=0.5, sigma_data=0.5, num_classes=None, ref_chunk=None,
                 device=None):
        import torch
        is_np = isinstance(data_u8, np.ndarray)
        if not is_np and not isinstance(data_u8, torch.Tensor):
            raise ValueError(f"IdealDenoiser: data_u8 must be a numpy array or a tensor, got {type(data_u8).__name__}")
        if isinstance(labels, torch.Tensor):
            labels = labels.detach().cpu().numpy()
        elif labels is not None:
            labels = np.asarray(labels)
        lab, self.num_classes, self.class_counts = check_set(
            data_u8.shape, data_u8.dtype == (np.uint8 if is_np else torch.uint8), labels, mean, std, sigma_data,
            num_classes, ref_chunk)
        self.mean, self.std, self.sigma_data, self.ref_chunk = float(mean), float(std), float(sigma_data), ref_chunk
        from . import ops
        data = torch.from_numpy(np.ascontiguousarray(data_u8)) if is_np else data_u8
        if device is None:
            device = data.device if data.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.data = data.to(device).contiguous()
        self.device = self.data.device
        self.ref_labels = None if lab is None else torch.from_numpy(lab).to(self.device)
        self.norms = ops.u8_norms(self.data)
        self.image_shape = tuple(self.data.shape[1:])
        self.num_refs, self.K = int(self.data.shape[0]), int(np.prod(self.image_shape))

    # ------------------------------------------------------------------ operands
    def _operands(self, x, sigma, class_labels):
        import torch
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("IdealDenoiser: x must be a CUDA/HIP tensor -- tinyedm_amd has no CPU path")
        if x.dim() != 4 or tuple(x.shape[1:]) != self.image_shape or x.shape[0] < 1 or not x.is_floating_point():
            raise ValueError(f"IdealDenoiser: x must be a floating-point [B, {', '.join(map(str, self.image_shape))}] tensor, "
                             f"got {x.dtype} {tuple(x.shape)}")
        if x.device != self.device:
            raise ValueError(f"IdealDenoiser: x is on {x.device}, the training set on {self.device}")
        B = x.shape[0]
        if isinstance(sigma, torch.Tensor):
            if not sigma.is_cuda:
                raise RuntimeError("IdealDenoiser: a sigma tensor must be a CUDA/HIP tensor -- tinyedm_amd has no CPU path")
            if sigma.numel() not in (1, B):
                raise ValueError(f"IdealDenoiser: sigma must hold 1 or {B} values, got {tuple(sigma.shape)}")
            sig = sigma.detach().to(device=self.device, dtype=torch.float32).reshape(-1).expand(B).contiguous()
        else:
            sig = torch.full((B,), check_sigma(sigma), dtype=torch.float32, device=self.device)
        lab = None
        # (a set without labels is an unconditional model: as the guide of a conditional solve it is handed the labels)
        if class_labels is not None and self.ref_labels is not None:
            if not isinstance(class_labels, torch.Tensor) or not class_labels.is_cuda:
                raise RuntimeError("IdealDenoiser: class_labels must be a CUDA/HIP tensor")
            if class_labels.numel() != B or class_labels.is_floating_point():
                raise ValueError(f"IdealDenoiser: class_labels must be {B} class indices, got {class_labels.dtype} "
                                 f"{tuple(class_labels.shape)}")
            lab = class_labels.detach().to(device=self.device, dtype=torch.int64).reshape(B).contiguous()
        return x.detach().float().contiguous(), sig, lab

    def _run(self, x, sigma, class_labels):
        from . import ops
        xf, sig, lab = self._operands(x, sigma, class_labels)
        out = ops.ideal_denoise(xf, sig, self.data, self.norms, self.mean, self.std, ref_labels=self.ref_labels, labels=lab,
                                num_classes=self.num_classes, ref_chunk=self.ref_chunk)
        return out, sig, lab

    def __call__(self, x, sigma, class_labels=None):
        """D*(x; sigma) as fp32 NCHW in the shape of x.  sigma: a Python number, a 0-d tensor or a [B] tensor.
        class_labels=None uses every training image, also on a labelled set; a set without labels ignores them."""
        return self._run(x, sigma, class_labels)[0][0]

    def stats_device(self, x, sigma, class_labels=None) -> tuple:
        """(D, lse, entropy, top_weight, top_index int32) on the device: stats() without its host read"""
        return self._run(x, sigma, class_labels)[0]

    def stats(self, x, sigma, class_labels=None) -> dict:
        """D and the per-query statistics of the softmax: lse = log sum_i exp(l_i), entropy = -sum w log w,
        effective_count = exp(entropy), top_weight and top_index (the largest weight and its training image, ties to the
        lower index) as device tensors, and log_density, the exact log density of the noised empirical distribution in
        nats, as an fp64 host array (one host read)."""
        import torch
        (D, lse, ent, top_w, top_idx), sig, lab = self._run(x, sigma, class_labels)
        n_refs = np.full(D.shape[0], float(self.num_refs))
        if lab is not None:
            lab_h = lab.cpu().numpy()
            ok = (lab_h >= 0) & (lab_h < self.num_classes)
            n_refs = np.where(ok, self.class_counts[np.where(ok, lab_h, 0)], np.nan).astype(np.float64)
        logp = log_density(lse.double().cpu().numpy(), n_refs, self.K, sig.double().cpu().numpy())
        return {"D": D, "lse": lse, "entropy": ent, "effective_count": ent.exp(), "top_weight": top_w,
                "top_index": top_idx.to(torch.int64), "log_density": logp}


# ---------------------------------------------------------------------------------------------------- the gap report
def reduce_gap(se: dict, eff: dict, chw: int, sigmas, sigma_data: float) -> dict:
    """The host reduction of the report.  se: name -> fp64 [draws, L, n] summed squared errors, images in id order, under
    the names ideal_train, ideal_test and, with a network, train, test, to_ideal_train, to_ideal_test; eff: "train" /
    "test" -> [draws, L, n] effective counts.  Every mean is evaluate.level_sums' sequential sum in id order.  Returns the
    per-level lists {sigma, weight, <name>_mse or to_ideal_*, excess_train, effective_count_*} and, under "weighted", the
    same error columns times lambda(sigma)."""
    from .evaluate import edm_weight, level_sums
    sigmas = [float(s) for s in sigmas]
    L = len(sigmas)
    lam = [edm_weight(s, float(sigma_data)) for s in sigmas]
    out = {"sigma": sigmas, "weight": lam}

    def mean(m):
        s = level_sums(m, chw)
        if s.shape[1] != L:
            raise ValueError(f"reduce_gap: expected {L} levels, got {s.shape[1]}")
        return [float(s[1, l] / s[0, l]) for l in range(L)]

    for name, m in se.items():
        out[name if name.startswith("to_ideal") else name + "_mse"] = mean(m)
    if "train" in se:
        out["excess_train"] = [a - b for a, b in zip(out["train_mse"], out["ideal_train_mse"])]
    for name, m in eff.items():
        out["effective_count_" + name] = mean(np.asarray(m, dtype=np.float64) * float(chw))    # (level_sums divides by chw)
    cols = [k for k in out if k.endswith("_mse") or k.startswith("to_ideal") or k == "excess_train"]
    out["weighted"] = {k: [w * v for w, v in zip(lam, out[k])] for k in cols}
    return out


def gap_sums(evaluator, ideal: IdealDenoiser, images, labels=None, model=None, ids=None) -> tuple:
    """One pass over `images` at the evaluator's levels with its fixed noise (ops.eval_diffuse: the same (id, level, draw)
    meets the same bits as in evaluate) -> (se, eff, sigmas): se["ideal"] = |D* - clean|^2 and, with a model, se["net"] =
    |D_net - clean|^2 and se["to_ideal"] = |D_net - D*|^2, each fp64 [draws, L, n] by ops.eval_sqerr with the images in
    id order; eff: the effective counts, same shape.  labels are given to both the network and D*."""
    import torch
    from . import ops
    from .callbacks import _eval_dtype
    from .evaluate import check_images
    images, labels, ids_h = check_images(images, labels, ids, "ideal")
    n, dev = images.shape[0], images.device
    sigmas = [float(np.float32(s)) for s in evaluator.levels_for(model if model is not None else ideal)]
    L, R = len(sigmas), evaluator.num_draws
    order = np.argsort(ids_h, kind="stable")
    total = L * n
    item_img = torch.from_numpy(np.tile(order, L)).to(dev)
    item_ids = torch.from_numpy(np.tile(ids_h[order].astype(np.uint32), L)).to(dev)
    item_level = torch.from_numpy(np.repeat(np.arange(L, dtype=np.int32), n)).to(dev)
    sig_dev = torch.tensor(sigmas, dtype=torch.float32, device=dev)
    names = ("ideal",) + (("net", "to_ideal") if model is not None else ())
    se = {k: torch.empty(R, L, n, dtype=torch.float64, device=dev) for k in names}
    eff = torch.empty(R, L, n, dtype=torch.float32, device=dev)
    is_module = isinstance(model, torch.nn.Module)
    was_training = is_module and model.training
    if is_module:
        model.eval()
    try:
        with torch.no_grad(), _eval_dtype(model, evaluator.network_dtype):
            for d in range(R):
                rec = ops.churn_record(evaluator.seed, d, dev)
                for t0 in range(0, total, evaluator.batch_size):
                    t1 = min(total, t0 + evaluator.batch_size)
                    idx = item_img[t0:t1]
                    clean = images.index_select(0, idx)
                    lab = None if labels is None else labels.index_select(0, idx)
                    noisy, sigma = ops.eval_diffuse(clean, item_ids[t0:t1], item_level[t0:t1], sig_dev, rec,
                                                    check_levels=False)
                    st = ideal.stats_device(noisy, sigma, lab)
                    ops.eval_sqerr(st[0], clean, out=se["ideal"][d].view(-1)[t0:t1])
                    eff[d].view(-1)[t0:t1] = st[2].exp()
                    if model is not None:
                        Dn = model(noisy, sigma, lab).float().contiguous()
                        if tuple(Dn.shape) != tuple(clean.shape):
                            raise ValueError(f"ideal: the model returned {tuple(Dn.shape)} for {tuple(clean.shape)}")
                        ops.eval_sqerr(Dn, clean, out=se["net"][d].view(-1)[t0:t1])
                        ops.eval_sqerr(Dn, st[0], out=se["to_ideal"][d].view(-1)[t0:t1])
    finally:
        if was_training:
            model.train()
    se_h = {k: v.cpu().numpy() for k, v in se.items()}
    eff_h = eff.double().cpu().numpy()
    ops.check_health(dev, "ideal.gap_sums")
    return se_h, eff_h, sigmas


def gap_report(evaluator, ideal: IdealDenoiser, train_images, test_images, train_labels=None, test_labels=None,
               model=None) -> dict:
    """The gap-to-ideal report of one model (None: the ideal columns only) on training and held-out images: reduce_gap of
    the two gap_sums passes.  `model` is any callable model(x, sigma, labels); the ideal denoiser itself gives
    to_ideal_train == 0 and excess_train == 0 exactly."""
    se, eff = {}, {}
    sigmas = None
    for split, images, labels in (("train", train_images, train_labels), ("test", test_images, test_labels)):
        s, e, sigmas = gap_sums(evaluator, ideal, images, labels, model)
        se["ideal_" + split] = s["ideal"]
        if model is not None:
            se[split], se["to_ideal_" + split] = s["net"], s["to_ideal"]
        eff[split] = e
    chw = int(np.prod(ideal.image_shape))
    sigma_data = float(getattr(model, "sigma_data", ideal.sigma_data)) if model is not None else ideal.sigma_data
    out = reduce_gap(se, eff, chw, sigmas, sigma_data)
    out.update(num_train=int(train_images.shape[0]), num_test=int(test_images.shape[0]), num_draws=evaluator.num_draws,
               seed=evaluator.seed, sigma_data=sigma_data, num_references=ideal.num_refs)
    return out


# ---------------------------------------------------------------------------------------------------- command line
def build_parser() -> argparse.ArgumentParser:
    from .evaluate import NETWORK_DTYPES
    p = argparse.ArgumentParser(description="The ideal denoiser of a training set: gap-to-ideal report and sampling")
    p.add_argument("--dataset", choices=["cifar10", "mnist"], default=None, help="built-in: train split = the training "
                   "set, test split = the held-out images (with --data_dir)")
    p.add_argument("--data_dir", type=str, default=None)
    p.add_argument("--image_dir", type=str, default=None, help="held-out images as a directory of <index>.png")
    p.add_argument("--train_image_dir", type=str, default=None, help="with --image_dir: the training set, <index>.png")
    p.add_argument("--labels_json", type=str, default=None, help="--image_dir: a JSON list of class indices in index order")
    p.add_argument("--train_labels_json", type=str, default=None, help="--train_image_dir: the same for the training set")
    p.add_argument("--mean", type=float, nargs="+", default=None, help="one value for all channels (default 0.5)")
    p.add_argument("--std", type=float, nargs="+", default=None, help="one value for all channels (default 0.5)")
    p.add_argument("--image_size", type=int, default=None)
    p.add_argument("--in_channels", type=int, default=None)
    p.add_argument("--ckpt_path", type=str, nargs="*", default=[], help="checkpoints to compare with the ideal denoiser")
    p.add_argument("--load_ema", action="store_true")
    p.add_argument("--network_dtype", choices=list(NETWORK_DTYPES), default="bf16")
    p.add_argument("--conditional", action="store_true", help="use the labels for both the network and D*")
    p.add_argument("--num_levels", type=int, default=16)
    p.add_argument("--sigmas", type=float, nargs="+", default=None, help="explicit levels, strictly increasing")
    p.add_argument("--P_mean", type=float, default=None, help="ln sigma ~ N(P_mean, P_std) of --num_levels (default: the "
                   "checkpoint's; needed without a checkpoint and without --sigmas)")
    p.add_argument("--P_std", type=float, default=None)
    p.add_argument("--num_images", type=int, default=1024, help="training images and as many held-out images")
    p.add_argument("--num_draws", type=int, default=1)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--batch_size", type=int, default=512)
    p.add_argument("--ref_chunk", type=int, default=None)
    p.add_argument("--report", type=str, default=None, metavar="OUT.json", help="write the gap-to-ideal report")
    p.add_argument("--samples", type=int, default=None, metavar="N", help="sample N images from D* (with --output_dir)")
    p.add_argument("--output_dir", type=str, default=None)
    p.add_argument("--num_steps", type=int, default=18)
    p.add_argument("--solver", choices=list(SOLVERS), default="heun")
    p.add_argument("--solver_order", type=int, choices=[1, 2, 3], default=2)
    p.add_argument("--S_churn", type=float, default=0.0)
    return p


def _one_value(v, name):
    if v is None:
        return 0.5
    if len(set(v)) != 1:
        raise ValueError(f"ideal: --{name} must be one value for all channels (per-channel normalisation is not supported)")
    return float(v[0])


def check_args(args):
    """every choice that needs nothing loaded, checked before a file or the GPU is touched -> the evaluator of the report
    (None in sampling mode)"""
    from .evaluate import NoiseLevelEvaluator, check_data_args
    if (args.report is None) == (args.samples is None):
        raise ValueError("ideal: give exactly one task: --report OUT.json, or --samples N --output_dir DIR")
    check_data_args(args, "ideal")
    if args.dataset is None:
        if args.train_image_dir is None:
            raise ValueError("ideal: --image_dir (the held-out images) needs --train_image_dir (the training set)")
        if (args.labels_json is None) != (args.train_labels_json is None):
            raise ValueError("ideal: --labels_json and --train_labels_json go together")
        if args.conditional and args.labels_json is None:
            raise ValueError("ideal: --conditional with --image_dir needs --labels_json and --train_labels_json")
    elif args.train_image_dir is not None or args.train_labels_json is not None:
        raise ValueError("ideal: --train_image_dir and --train_labels_json go with --image_dir")
    mean, std = _one_value(args.mean, "mean"), _one_value(args.std, "std")
    if not (math.isfinite(mean) and math.isfinite(std) and std > 0.0):
        raise ValueError(f"ideal: --mean must be finite and --std finite and > 0, got {mean}, {std}")
    if args.ref_chunk is not None and args.ref_chunk < 1:
        raise ValueError(f"ideal: --ref_chunk must be >= 1, got {args.ref_chunk}")
    if args.samples is not None:
        if args.samples < 1:
            raise ValueError(f"ideal: --samples must be >= 1, got {args.samples}")
        if args.output_dir is None:
            raise ValueError("ideal: --samples needs --output_dir")
        if args.ckpt_path:
            raise ValueError("ideal: --samples draws from the ideal denoiser and takes no --ckpt_path")
        if args.num_steps < 2:
            raise ValueError(f"ideal: --num_steps must be >= 2, got {args.num_steps}")
        if not (math.isfinite(args.S_churn) and args.S_churn >= 0.0):
            raise ValueError(f"ideal: --S_churn must be finite and >= 0, got {args.S_churn}")
        if args.solver == "dpmpp" and args.S_churn != 0.0:
            raise ValueError("ideal: --S_churn goes with --solver heun")
        if not 0 <= args.seed < 1 << 64 or args.batch_size < 1:
            raise ValueError("ideal: --seed must be in [0, 2^64) and --batch_size >= 1")
        return None
    if args.output_dir is not None:
        raise ValueError("ideal: --output_dir goes with --samples")
    if not args.ckpt_path and args.sigmas is None and (args.P_mean is None or args.P_std is None):
        raise ValueError("ideal: without a checkpoint the levels need --sigmas, or --P_mean and --P_std")
    return NoiseLevelEvaluator(sigmas=args.sigmas, num_levels=args.num_levels, P_mean=args.P_mean, P_std=args.P_std,
                               seed=args.seed, num_draws=args.num_draws, batch_size=args.batch_size,
                               network_dtype=args.network_dtype)


def _read_labels(path, n, who):
    with open(path) as f:
        labels = json.load(f)
    if not isinstance(labels, list) or len(labels) < n or not all(
            isinstance(v, int) and not isinstance(v, bool) and v >= 0 for v in labels):
        raise ValueError(f"ideal: {who} must hold a list of at least {n} class indices")
    return np.asarray(labels[:n], dtype=np.int64)


def _load_sets(args):
    """(train uint8 [R, C, H, W], train labels or None, held-out uint8, held-out labels or None) on the host"""
    if args.dataset is not None:
        from .datamodules import read_cifar10, read_mnist
        read = read_cifar10 if args.dataset == "cifar10" else read_mnist
        (xtr, ytr), (xte, yte) = read(args.data_dir, True), read(args.data_dir, False)
        nchw = lambda x: np.ascontiguousarray(np.asarray(x)[:, None] if np.asarray(x).ndim == 3 else np.asarray(x))  # noqa: E731
        return nchw(xtr), np.asarray(ytr, dtype=np.int64), nchw(xte), np.asarray(yte, dtype=np.int64)
    from .neighbors import load_images_u8
    train = load_images_u8(args.train_image_dir, args.image_size, args.in_channels)
    test = load_images_u8(args.image_dir, args.image_size, train.shape[1])
    ltr = lte = None
    if args.labels_json is not None:
        ltr = _read_labels(args.train_labels_json, train.shape[0], "--train_labels_json")
        lte = _read_labels(args.labels_json, test.shape[0], "--labels_json")
    return train, ltr, test, lte


def _sample(args, ideal, dev) -> dict:
    import types
    import torch
    from .callbacks import PreditionWriter
    from .solvers import DeterministicSolver, MultistepSolver, StochasticSolver
    common = dict(num_steps=args.num_steps, seed=args.seed)
    if args.solver == "dpmpp":
        solver = MultistepSolver(order=args.solver_order, **common)
    elif args.S_churn != 0.0:
        solver = StochasticSolver(S_churn=args.S_churn, **common)
    else:
        solver = DeterministicSolver(**common)
    C = ideal.image_shape[0]
    writer = PreditionWriter(args.output_dir, "batch", mean=(ideal.mean,) * C, std=(ideal.std,) * C)
    gen = torch.Generator().manual_seed(args.seed)
    sigma_last = float(solver.t_steps[args.num_steps - 1])
    tops, labels_out = [], []
    for a in range(0, args.samples, args.batch_size):
        n = min(args.batch_size, args.samples - a)
        x0 = torch.randn((n,) + ideal.image_shape, generator=gen).to(dev)
        lab = None
        if args.conditional:
            lab = torch.randint(0, ideal.num_classes, (n,), generator=gen).to(dev)
            labels_out += lab.cpu().tolist()
        x = solver.solve(ideal, x0, lab)
        tops += ideal.stats(x, sigma_last, lab)["top_index"].cpu().tolist()
        writer.write_on_batch_end(None, types.SimpleNamespace(device=dev), x, None, None, 0, 0)
    out = {"num_samples": args.samples, "solver": args.solver, "num_steps": args.num_steps, "seed": args.seed,
           "S_churn": args.S_churn, "top_index": tops}
    if args.conditional:
        out["class_labels"] = labels_out
    with open(os.path.join(args.output_dir, "top_index.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote images 0..{args.samples - 1} and top_index.json to {args.output_dir}", flush=True)
    return out


def format_table(report: dict, names: list) -> str:
    first = report["ideal"] if not names else report["checkpoints"][names[0]]
    lines = [f"level      sigma  {'ideal_train':>12s} {'ideal_test':>12s} {'eff_train':>10s} {'eff_test':>10s}"
             + "".join(f"  {'train[' + str(i) + ']':>12s} {'test[' + str(i) + ']':>12s} {'to_ideal[' + str(i) + ']':>12s}"
                       for i in range(len(names)))]
    for l, s in enumerate(first["sigma"]):
        row = (f"{l:5d} {s:10.4g}  {first['ideal_train_mse'][l]:12.6g} {first['ideal_test_mse'][l]:12.6g} "
               f"{first['effective_count_train'][l]:10.4g} {first['effective_count_test'][l]:10.4g}")
        for k in names:
            e = report["checkpoints"][k]
            row += f"  {e['train_mse'][l]:12.6g} {e['test_mse'][l]:12.6g} {e['to_ideal_train'][l]:12.6g}"
        lines.append(row)
    return "\n".join(lines)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        evaluator = check_args(args)
    except ValueError as e:
        parser.error(str(e))
    import torch
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dev = torch.device("cuda", torch.cuda.current_device())
    train, ltr, test, lte = _load_sets(args)
    mean, std = _one_value(args.mean, "mean"), _one_value(args.std, "std")
    if not args.conditional:
        ltr = lte = None
    ideal = IdealDenoiser(train, ltr, mean=mean, std=std, ref_chunk=args.ref_chunk, device=dev)
    if evaluator is None:
        return _sample(args, ideal, dev)
    from . import ops
    from .edm import EDM
    n = min(args.num_images, train.shape[0], test.shape[0])
    tr = ops.u8_gather_normalize(ideal.data, torch.arange(n, device=dev), mean, std)
    te = ops.u8_gather_normalize(torch.from_numpy(np.ascontiguousarray(test[:n])).to(dev), torch.arange(n, device=dev),
                                 mean, std)
    ltr_d = None if ltr is None else torch.from_numpy(ltr[:n]).to(dev)
    lte_d = None if lte is None else torch.from_numpy(lte[:n]).to(dev)
    report = {"num_images": n, "num_references": ideal.num_refs, "conditional": bool(args.conditional),
              "num_draws": args.num_draws, "seed": args.seed, "network_dtype": args.network_dtype,
              "load_ema": bool(args.load_ema), "checkpoints": {}}
    if not args.ckpt_path:
        report["ideal"] = gap_report(evaluator, ideal, tr, te, ltr_d, lte_d, None)
    for path in args.ckpt_path:
        model = EDM.load_from_checkpoint(path, load_ema=args.load_ema).to(dev).eval()
        if args.conditional and not model.conditional:
            raise ValueError(f"ideal: --conditional but {path} is not class-conditional")
        report["checkpoints"][path] = gap_report(evaluator, ideal, tr, te, ltr_d, lte_d, model)
        del model
    with open(args.report, "w") as f:
        json.dump(report, f, indent=1)
    print(format_table(report, list(args.ckpt_path)))
    print(f"wrote {args.report}", flush=True)
    return report


if __name__ == "__main__":
    main()
