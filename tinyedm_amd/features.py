"""Denoiser activations as features, and two probes of them.

A trained EDM denoiser is a representation learner: the global-average-pooled activations of an intermediate block, taken
on a slightly noised image, linear-probe on par with dedicated self-supervised encoders (Xiang et al. 2023, "Denoising
Diffusion Autoencoders are Unified Self-supervised Learners").  Any checkpoint of this project is therefore a feature
extractor for the tools that take `--features` (tinyedm.frechet, tinyedm.prdc, tinyedm.neighbors):

    python -m tinyedm.features --ckpt_path ema.ckpt --load_ema --image_dir samples --out samples.npy
    python -m tinyedm.features --ckpt_path ema.ckpt --load_ema --dataset cifar10 --data_dir data --split train --out train.npy
    python -m tinyedm.frechet --features samples.npy --ref_features train.npy --report fd.json

These are the project's own features, not Inception features: the numbers are comparable between checkpoints and sample
sets scored with the SAME extractor checkpoint, not with published FID tables.

The features.  Image i is noised at one level sigma with noise that depends on (seed, ids[i]) alone (ops.eval_diffuse), the
denoiser runs at reference precision ("f32x3" or "f32") up to the deepest requested tap and no further
(Denoiser.forward_taps), and each tapped NHWC map is averaged over its pixels in fp64 in a fixed order
(ops.f32_pool_features) straight into the tap's columns of the result.  A row therefore has the same bits whatever batch it
travelled in.

The probes.  The linear-probe and k-NN accuracy of the features is a checkpoint metric in its own right (representation
quality), and the sweep over noise levels and taps is how sigma and the tap are chosen: the defaults (sigma 0.1, "mid")
are a starting point that has not been measured on this project's checkpoints.

    python -m tinyedm.features --probe --ckpt_path a.ckpt b.ckpt --dataset cifar10 --data_dir data \\
        --sweep_sigmas 0.05 0.1 0.2 0.4 --sweep_taps enc5 mid dec2 --report probe.json
"""
from __future__ import annotations

import argparse
import json
import math
import os

import numpy as np
import torch

NETWORK_DTYPES = ("f32x3", "f32")
KNN_MAX_K = 32          # ops.KNN_MAX_K, repeated here so that the argument check needs no GPU library


# ---------------------------------------------------------------------------------------------------- the extractor
def check_sigma(sigma, who: str = "features") -> float:
    try:
        s = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: sigma must be a number, got {sigma!r}") from None
    if not (math.isfinite(s) and s > 0.0 and math.isfinite(float(np.float32(s))) and float(np.float32(s)) > 0.0):
        raise ValueError(f"{who}: sigma must be finite and > 0 (c_noise = ln(sigma) / 4), got {sigma}")
    return s


class FeatureExtractor:
    """extract(images, labels=None, ids=None) -> float32 [n, dim] on the device: the pooled activations of `taps` of
    `model` (an EDM) on the images noised at `sigma`, the taps side by side in the order given.

    sigma and taps: the defaults (0.1, "mid" = the last encoder block) are a starting point nobody has measured on this
    project's checkpoints; `python -m tinyedm.features --probe --sweep_sigmas ... --sweep_taps ...` is how to pick them.
    seed selects the noise: image id draws the stream (seed, id).  batch_size is the number of images per network call; it
    changes no bit of the result.  network_dtype: "f32x3" or "f32" (features are taken at reference precision).
    conditional=True passes the labels to the network, so the features are conditioned on the true class (for generated
    samples: the labels `generate --labels_to` recorded); the default passes none."""

    def __init__(self, model, sigma: float = 0.1, taps=("mid",), seed: int = 0, batch_size: int = 512,
                 network_dtype: str = "f32x3", conditional: bool = False):
        from .networks import tap_positions
        den = getattr(model, "denoiser", None)
        if den is None or not hasattr(den, "forward_taps") or not hasattr(model, "forward_taps"):
            raise ValueError("features: the model must be an EDM with a tinyedm_amd Denoiser")
        if network_dtype not in NETWORK_DTYPES:
            raise ValueError(f"features: network_dtype must be one of {NETWORK_DTYPES} (features are taken at reference "
                             f"precision; the bf16 forward has no taps), got {network_dtype!r}")
        self.sigma = check_sigma(sigma)
        pos = tap_positions(taps, len(den.encoder_blocks), len(den.decoder_blocks))
        self.taps = tuple(pos)
        for name, v, lo, hi in (("seed", seed, 0, 1 << 64), ("batch_size", batch_size, 1, 65536)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v < hi:
                raise ValueError(f"features: {name} must be an integer in [{lo}, {hi}), got {v!r}")
        if conditional and not getattr(model, "conditional", False):
            raise ValueError("features: conditional=True needs a class-conditional model")
        self.model, self.seed, self.batch_size = model, seed, batch_size
        self.network_dtype, self.conditional = network_dtype, bool(conditional)
        blocks = list(den.encoder_blocks) + list(den.decoder_blocks)
        self.widths = tuple(int(blocks[pos[t]].conv_3x3_2.weight.shape[0]) for t in self.taps)

    @property
    def dim(self) -> int:
        return sum(self.widths)

    def _images(self, images, labels, ids):
        """-> (uint8 NCHW on the device or None, fp32 NCHW on the device or None, labels or None, ids uint32 on the device)"""
        from .evaluate import check_images
        u8 = f32 = None
        if isinstance(images, np.ndarray):
            images = torch.from_numpy(np.ascontiguousarray(images))
        if isinstance(images, torch.Tensor) and images.dtype == torch.uint8:
            if images.dim() != 4 or images.numel() == 0:
                raise ValueError(f"features: uint8 images must be a non-empty [n, H, W, C] tensor, got {tuple(images.shape)}")
            dev = next(self.model.parameters()).device
            u8 = images.to(dev).permute(0, 3, 1, 2).contiguous()
        else:
            f32, _, _ = check_images(images, None, None, "features")
            dev = f32.device
        n = (u8 if f32 is None else f32).shape[0]
        ids_h = np.arange(n, dtype=np.int64) if ids is None else np.asarray(
            ids.detach().cpu() if isinstance(ids, torch.Tensor) else ids).astype(np.int64).reshape(-1)
        if ids_h.shape[0] != n or ids_h.min() < 0 or ids_h.max() >= 1 << 32 or np.unique(ids_h).shape[0] != n:
            raise ValueError(f"features: ids must be {n} distinct integers in [0, 2**32)")
        if labels is not None:
            labels = torch.as_tensor(labels)
            if labels.numel() != n:
                raise ValueError(f"features: labels must be a tensor of {n} class indices")
            labels = labels.to(dev).reshape(n)
        if self.conditional:
            if labels is None:
                raise ValueError("features: conditional=True needs the labels of the images")
            labels = labels.to(torch.int64)
            if int(labels.min()) < 0 or int(labels.max()) >= int(self.model.num_classes):
                raise ValueError(f"features: labels must lie in [0, {self.model.num_classes})")
        return u8, f32, (labels if self.conditional else None), torch.from_numpy(ids_h.astype(np.uint32)).to(dev)

    @torch.no_grad()
    def extract(self, images, labels=None, ids=None) -> torch.Tensor:
        """images: uint8 [n, H, W, C] (normalised as the datamodules do, mean 0.5 and std 0.5) or float32 [n, C, H, W]
        already in network range, on the GPU (uint8 images are moved there).  ids: n distinct integers in [0, 2**32)
        that name the images' noise streams (default 0 .. n - 1)."""
        from . import ops
        out = dev = None
        for a, b, (maps,), n in self._tapped(images, labels=labels, ids=ids):
            if out is None:
                dev = maps[self.taps[0]].device
                out = torch.empty(n, self.dim, dtype=torch.float32, device=dev)
            col = 0
            for t, width in zip(self.taps, self.widths):
                ops.f32_pool_features(maps[t], out[a:b], col)
                col += width
        if out is None:
            raise ValueError("features: no images")
        ops.check_health(dev, "FeatureExtractor.extract")
        return out

    def tapped_maps(self, *image_sets, labels=None, ids=None):
        """The tapped activations batch by batch: yields (a, b, maps), maps a tuple with one dict {tap: fp32 NHWC map of
        the images a .. b - 1} per image set, in the order given.  Every set is an `images` of extract() with the same
        count and shape; image i of every set is noised with the SAME stream (seed, ids[i]) and shares labels[i], so
        sets that are to be compared image by image (compare.PairedQuality) meet the same noise.  The maps of a batch are
        the caller's.  Eval mode, network_dtype and no_grad are set for the work of one batch and put back before it is
        yielded: between batches, and if the generator is abandoned, the model and the grad mode are as the caller
        left them."""
        for a, b, maps, _ in self._tapped(*image_sets, labels=labels, ids=ids):
            yield a, b, maps

    def _tapped(self, *image_sets, labels=None, ids=None):
        """tapped_maps with the image count as a fourth item"""
        from . import ops
        if not image_sets:
            raise ValueError("features: no images")
        sets = []
        for images in image_sets:
            u8, f32, lab, ids_dev = self._images(images, labels, ids)
            sets.append((u8, f32))
            src = u8 if u8 is not None else f32
            first = sets[0][0] if sets[0][0] is not None else sets[0][1]
            if src.shape != first.shape or src.dtype != first.dtype or src.device != first.device:
                raise ValueError(f"features: the image sets differ: {src.dtype} {tuple(src.shape)} on {src.device} against "
                                 f"{first.dtype} {tuple(first.shape)} on {first.device}")
        labels = lab
        n, dev = first.shape[0], first.device
        level = torch.zeros(n, dtype=torch.int32, device=dev)
        sig_dev = torch.tensor([self.sigma], dtype=torch.float32, device=dev)
        rec = ops.churn_record(self.seed, 0, dev)
        for a in range(0, n, self.batch_size):
            b = min(n, a + self.batch_size)
            yield a, b, self._batch_maps(sets, a, b, labels, ids_dev, level, sig_dev, rec), n

    def _batch_maps(self, sets, a, b, labels, ids_dev, level, sig_dev, rec) -> tuple:
        """the maps of images a .. b - 1 of every set; the model's modes are changed here and put back here"""
        from . import ops
        from .callbacks import _eval_dtype
        model, dev = self.model, level.device
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad(), _eval_dtype(model, self.network_dtype):
                out = []
                for u8, f32 in sets:
                    clean = f32[a:b] if u8 is None else ops.u8_gather_normalize(u8, torch.arange(a, b, device=dev), 0.5, 0.5)
                    noisy, sigma = ops.eval_diffuse(clean, ids_dev[a:b], level[a:b], sig_dev, rec, check_levels=False)
                    maps = model.forward_taps(noisy, sigma, None if labels is None else labels[a:b], self.taps)
                    for t, width in zip(self.taps, self.widths):
                        if maps[t].shape[-1] != width:
                            raise ValueError(f"features: tap {t} gave {maps[t].shape[-1]} channels, expected {width}")
                    out.append(maps)
                return tuple(out)
        finally:
            if was_training:
                model.train()


# ---------------------------------------------------------------------------------------------------- the probes
def _probe_sets(train_x, train_y, num_classes, who):
    """the checks both probes share -> (train_x float32 [n, D] on the GPU, train_y int64 [n] on its device)"""
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 2:
        raise ValueError(f"{who}: num_classes must be an integer >= 2, got {num_classes!r}")
    x = _rows(train_x, "train_x", who)
    y = _labels(train_y, x.shape[0], num_classes, "train_y", who).to(x.device)
    if x.shape[0] < num_classes:
        raise ValueError(f"{who}: {x.shape[0]} training rows for {num_classes} classes: fewer rows than classes")
    counts = torch.bincount(y, minlength=num_classes)
    empty = torch.nonzero(counts == 0).flatten().tolist()
    if empty:
        raise ValueError(f"{who}: no training row of class {', '.join(str(c) for c in empty)}")
    return x, y, counts


def _rows(x, name, who):
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.numel() == 0:
        what = f"{x.dtype} {tuple(x.shape)}" if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"{who}: {name} must be a non-empty float32 [n, D] tensor, got {what}")
    if not x.is_cuda:
        raise ValueError(f"{who}: {name}: expected a CUDA/HIP tensor -- tinyedm_amd has no CPU path")
    if not bool(torch.isfinite(x).all()):
        raise ValueError(f"{who}: {name} holds non-finite features")
    return x.contiguous()


def _labels(y, n, num_classes, name, who):
    t = torch.as_tensor(np.asarray(y) if not isinstance(y, torch.Tensor) else y)
    if t.dtype.is_floating_point or t.dtype == torch.bool or t.numel() != n:
        raise ValueError(f"{who}: {name} must hold {n} integer class indices")
    t = t.reshape(n).to(torch.int64)
    if n and (int(t.min()) < 0 or int(t.max()) >= num_classes):
        raise ValueError(f"{who}: {name} must lie in [0, {num_classes}), got {int(t.min())} .. {int(t.max())}")
    return t


def _first_max(scores):
    """argmax over the last axis, ties to the lower index (stated, not left to the library)"""
    K = scores.shape[1]
    top = scores.max(dim=1, keepdim=True).values
    return torch.where(scores == top, torch.arange(K, device=scores.device), K).min(dim=1).values


class RidgeProbe:
    """predict(x) = argmax_c ((x - mean) . W + prior)_c in fp64 on the device, ties to the lower class"""

    def __init__(self, mean, W, prior, num_classes):
        self.mean, self.W, self.prior, self.num_classes = mean, W, prior, num_classes

    def predict(self, x) -> torch.Tensor:
        x = _rows(x, "x", "ridge_probe")
        if x.shape[1] != self.mean.shape[0] or x.device != self.W.device:
            raise ValueError(f"ridge_probe: expected [n, {self.mean.shape[0]}] features on {self.W.device}, got "
                             f"{tuple(x.shape)} on {x.device}")
        return _first_max((x.double() - self.mean) @ self.W + self.prior)

    def accuracy(self, x, y) -> float:
        pred = self.predict(x)
        y = _labels(y, pred.shape[0], self.num_classes, "y", "ridge_probe").to(pred.device)
        return float((pred == y).double().mean())


def ridge_solve(n, total, gram, class_sums, class_counts, l2):
    """The closed form on the host, numpy fp64: mean mu = total / n, covariance S = gram / n - mu mu^T, one-hot prior
    ybar_c = n_c / n; solves (S + l2 * (tr S / D) * I) W = class_sums^T / n - mu ybar^T -> (mu [D], W [D, K], ybar [K]).
    class_sums [K, D]: the sum of the rows of each class."""
    total, gram = np.asarray(total, dtype=np.float64), np.asarray(gram, dtype=np.float64)
    cs, cnt = np.asarray(class_sums, dtype=np.float64), np.asarray(class_counts, dtype=np.float64)
    D = total.shape[0]
    if not (math.isfinite(float(l2)) and float(l2) > 0.0):
        raise ValueError(f"ridge_probe: l2 must be finite and > 0, got {l2}")
    mu, ybar = total / n, cnt / n
    S = gram / n - np.outer(mu, mu)
    tr = float(np.trace(S))
    if not tr > 0.0:
        raise ValueError("ridge_probe: the training features are constant (zero variance)")
    A = S + float(l2) * (tr / D) * np.eye(D)
    return mu, np.linalg.solve(A, cs.T / n - np.outer(mu, ybar)), ybar


def ridge_probe(train_x, train_y, num_classes, l2=1e-3) -> RidgeProbe:
    """A ridge classifier: the closed-form least-squares map of the centred features onto centred one-hot targets, in
    fp64 -- NOT the SGD-trained logistic probe of Xiang et al. 2023.  It is deterministic and has no schedule to tune; its
    accuracies are comparable between checkpoints of this project, not with published linear-probe tables.
    train_x: float32 [n, D] on the GPU; train_y: n labels in [0, num_classes), every class present.  The moments come from
    ops.moments (the class sums by exact row selection); l2 scales with the mean feature variance (ridge_solve)."""
    from . import ops
    x, y, counts = _probe_sets(train_x, train_y, num_classes, "ridge_probe")
    total, gram = ops.moments(x)
    sums = torch.stack([ops.moments(x, index=torch.nonzero(y == c).flatten(), sums_only=True)[0]
                        for c in range(num_classes)])
    mu, W, ybar = ridge_solve(x.shape[0], total.cpu().numpy(), gram.cpu().numpy(), sums.cpu().numpy(),
                              counts.cpu().numpy(), l2)
    dev = x.device
    return RidgeProbe(torch.from_numpy(mu).to(dev), torch.from_numpy(W).to(dev), torch.from_numpy(ybar).to(dev), num_classes)


def _unit_rows(x):
    """rows scaled to unit L2 norm (norms in fp64; a zero row stays zero)"""
    nrm = x.double().pow(2).sum(dim=1, keepdim=True).sqrt()
    return (x.double() / torch.where(nrm > 0, nrm, torch.ones_like(nrm))).float().contiguous()


def knn_vote(neighbour_labels, num_classes) -> torch.Tensor:
    """neighbour_labels int64 [Q, k], nearest first -> the majority class; a tied vote goes to the class of the nearest
    neighbour among the tied classes"""
    lab = neighbour_labels
    Q, k = lab.shape
    votes = torch.zeros(Q, num_classes, dtype=torch.int64, device=lab.device).scatter_add_(1, lab, torch.ones_like(lab))
    winners = votes.gather(1, lab) == votes.max(dim=1, keepdim=True).values          # [Q, k]: this neighbour's class leads
    first = torch.where(winners, torch.arange(k, device=lab.device), k).min(dim=1, keepdim=True).values
    return lab.gather(1, first).flatten()


def knn_predict(train_x, train_y, test_x, k=20, *, num_classes) -> torch.Tensor:
    """the k-NN vote of every test row: the k nearest training rows by Euclidean distance between L2-normalised rows
    (ops.f32_knn: fp64 distances, ties to the lower index), then knn_vote"""
    from . import ops
    x, y, _ = _probe_sets(train_x, train_y, num_classes, "knn_accuracy")
    q = _rows(test_x, "test_x", "knn_accuracy")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(KNN_MAX_K, x.shape[0]):
        raise ValueError(f"knn_accuracy: k must be an integer in [1, min({KNN_MAX_K}, training rows = {x.shape[0]})], got {k!r}")
    if q.shape[1] != x.shape[1] or q.device != x.device:
        raise ValueError(f"knn_accuracy: test_x {tuple(q.shape)} on {q.device} does not match train_x {tuple(x.shape)} on {x.device}")
    _, idx = ops.f32_knn(_unit_rows(q), _unit_rows(x), k)
    return knn_vote(y[idx], num_classes)


def knn_accuracy(train_x, train_y, test_x, test_y, k=20, *, num_classes) -> float:
    pred = knn_predict(train_x, train_y, test_x, k, num_classes=num_classes)
    y = _labels(test_y, pred.shape[0], num_classes, "test_y", "knn_accuracy").to(pred.device)
    return float((pred == y).double().mean())


# ---------------------------------------------------------------------------------------------------- command line
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Denoiser activations as features: extract them, or probe them (--probe)")
    p.add_argument("--ckpt_path", type=str, nargs="+", required=True, help="the checkpoint (--probe: one or more to compare)")
    p.add_argument("--load_ema", action="store_true", help="use the EMA weights of the checkpoint(s)")
    p.add_argument("--dataset", choices=["cifar10", "mnist"], default=None, help="built-in dataset (with --data_dir)")
    p.add_argument("--data_dir", type=str, default=None)
    p.add_argument("--split", choices=["train", "test"], default=None, help="extract: the split of --dataset (default train)")
    p.add_argument("--image_dir", type=str, default=None, help="directory of <index>.png images (as generate writes them)")
    p.add_argument("--sigma", type=float, default=0.1, help="the noise level the features are taken at")
    p.add_argument("--taps", type=str, nargs="+", default=["mid"], help='block outputs: "enc<i>", "dec<i>" or "mid"')
    p.add_argument("--conditional", action="store_true", help="pass the class labels to a class-conditional checkpoint")
    p.add_argument("--labels_json", type=str, default=None,
                   help="--image_dir with --conditional: a JSON list of class indices, one per image in index order")
    p.add_argument("--out", type=str, default=None, metavar="FEATS.npy", help="extract: the float32 [n, dim] array")
    p.add_argument("--labels_out", type=str, default=None, metavar="LABELS.json", help="extract: the labels of the rows")
    p.add_argument("--network_dtype", type=str, default="f32x3", help="f32x3 or f32 (reference precision)")
    p.add_argument("--batch_size", type=int, default=512)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--num_images", type=int, default=None, help="extract: the first N images (default all)")
    p.add_argument("--probe", action="store_true", help="ridge and k-NN test accuracy of train-split features on the test split")
    p.add_argument("--sweep_sigmas", type=float, nargs="+", default=None, help="--probe: noise levels (default --sigma)")
    p.add_argument("--sweep_taps", type=str, nargs="+", default=None, help="--probe: taps, one at a time (default --taps)")
    p.add_argument("--k", type=int, default=20, help="--probe: neighbours of the k-NN vote")
    p.add_argument("--l2", type=float, default=1e-3, help="--probe: ridge strength, relative to the mean feature variance")
    p.add_argument("--num_train", type=int, default=None, help="--probe: the first N training images (default all)")
    p.add_argument("--num_test", type=int, default=None, help="--probe: the first M test images (default all)")
    p.add_argument("--report", type=str, default=None, metavar="PROBE.json")
    return p


def _count(v, flag):
    if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 1):
        raise ValueError(f"features: --{flag} must be an integer >= 1, got {v!r}")


def check_args(args) -> None:
    """every choice that needs nothing loaded, checked before a checkpoint or the GPU is touched"""
    if args.network_dtype not in NETWORK_DTYPES:
        raise ValueError(f"features: --network_dtype must be one of {NETWORK_DTYPES}: features are taken at reference "
                         f"precision (the bf16 forward has no taps), got {args.network_dtype!r}")
    if args.probe and args.image_dir is not None:
        raise ValueError("features: --probe needs the labelled train and test splits of --dataset; it does not take --image_dir")
    if (args.dataset is None) == (args.image_dir is None):
        raise ValueError("features: give exactly one data source: --dataset cifar10|mnist --data_dir DIR, or --image_dir DIR")
    if args.dataset is not None and args.data_dir is None:
        raise ValueError("features: --dataset needs --data_dir")
    if args.dataset is None and args.data_dir is not None:
        raise ValueError("features: --data_dir goes with --dataset")
    if args.dataset is None and args.split is not None:
        raise ValueError("features: --split goes with --dataset")
    if args.labels_json is not None and args.image_dir is None:
        raise ValueError("features: --labels_json goes with --image_dir (the built-in datasets carry their own labels)")
    if args.conditional and args.image_dir is not None and args.labels_json is None:
        raise ValueError("features: --conditional needs labels: give --labels_json with --image_dir (for generated samples, "
                         "the file generate --labels_to wrote)")
    if args.labels_out is not None and args.image_dir is not None and args.labels_json is None:
        raise ValueError("features: --labels_out has no labels to write: --image_dir came without --labels_json")
    check_sigma(args.sigma, "features: --sigma")
    for flag in ("batch_size", "num_images", "num_train", "num_test"):
        _count(getattr(args, flag), flag)
    if isinstance(args.seed, bool) or not isinstance(args.seed, int) or not 0 <= args.seed < 1 << 64:
        raise ValueError(f"features: --seed must be in [0, 2**64), got {args.seed!r}")
    if len(set(args.taps)) != len(args.taps):
        raise ValueError(f"features: --taps names a tap twice: {args.taps}")
    if args.probe:
        for flag in ("out", "labels_out", "split", "num_images"):
            if getattr(args, flag) is not None:
                raise ValueError(f"features: --{flag} belongs to extraction; --probe writes --report")
        if args.report is None:
            raise ValueError("features: --probe needs --report PROBE.json")
        if len(set(args.ckpt_path)) != len(args.ckpt_path):
            raise ValueError("features: --ckpt_path names a checkpoint twice")
        for s in args.sweep_sigmas or ():
            check_sigma(s, "features: --sweep_sigmas")
        for flag in ("sweep_sigmas", "sweep_taps"):
            v = getattr(args, flag)
            if v is not None and len(set(v)) != len(v):
                raise ValueError(f"features: --{flag} lists a value twice: {v}")
        if isinstance(args.k, bool) or not isinstance(args.k, int) or not 1 <= args.k <= KNN_MAX_K:
            raise ValueError(f"features: --k must be in [1, {KNN_MAX_K}], got {args.k!r}")
        if args.num_train is not None and args.k > args.num_train:
            raise ValueError(f"features: --k {args.k} needs at least that many training images, got --num_train {args.num_train}")
        if not (math.isfinite(args.l2) and args.l2 > 0.0):
            raise ValueError(f"features: --l2 must be finite and > 0, got {args.l2}")
    else:
        if args.out is None:
            raise ValueError("features: extraction needs --out FEATS.npy (or --probe with --report)")
        if len(args.ckpt_path) != 1:
            raise ValueError("features: extraction takes one --ckpt_path (several are compared with --probe)")
        for flag in ("sweep_sigmas", "sweep_taps", "num_train", "num_test", "report"):
            if getattr(args, flag) is not None:
                raise ValueError(f"features: --{flag} goes with --probe")


def _read_split(name, data_dir, train, limit):
    """(uint8 [n, H, W, C], int64 labels [n]) of a built-in split, the first `limit` images"""
    from .datamodules import read_cifar10, read_mnist
    x, y = (read_cifar10 if name == "cifar10" else read_mnist)(data_dir, train)
    x = np.asarray(x)
    x = x[:, None] if x.ndim == 3 else x
    n = x.shape[0] if limit is None else min(limit, x.shape[0])
    return np.ascontiguousarray(x[:n].transpose(0, 2, 3, 1)), np.asarray(y[:n], dtype=np.int64)


def _load_extract_data(args):
    """(uint8 [n, H, W, C], labels int64 [n] or None) of extract mode"""
    if args.dataset is not None:
        return _read_split(args.dataset, args.data_dir, args.split != "test", args.num_images)
    from .neighbors import load_images_u8
    x = load_images_u8(args.image_dir)
    x = x if args.num_images is None else x[:args.num_images]
    labels = None
    if args.labels_json is not None:
        with open(args.labels_json) as f:
            labels = json.load(f)
        if not isinstance(labels, list) or len(labels) < x.shape[0] or not all(
                isinstance(v, int) and not isinstance(v, bool) and v >= 0 for v in labels):
            raise ValueError(f"features: --labels_json must hold a list of at least {x.shape[0]} class indices")
        labels = np.asarray(labels[:x.shape[0]], dtype=np.int64)
    return np.ascontiguousarray(x.transpose(0, 2, 3, 1)), labels


def write_features(path, feats) -> None:
    """float32 [n, dim] as the .npy that neighbors.read_features (frechet / prdc / neighbors --features) reads"""
    a = np.ascontiguousarray(feats.detach().cpu().numpy() if isinstance(feats, torch.Tensor) else feats)
    if a.dtype != np.float32 or a.ndim != 2 or not np.isfinite(a).all():
        raise ValueError(f"features: expected finite float32 [n, dim] features, got {a.dtype} {a.shape}")
    with open(path, "wb") as f:          # (a file object: numpy appends no .npy to the name)
        np.save(f, a, allow_pickle=False)


def _load_model(path, load_ema, dev):
    from .edm import EDM
    return EDM.load_from_checkpoint(path, load_ema=load_ema).to(dev).eval()


def format_table(cells) -> str:
    lines = [f"{'checkpoint':<32s} {'sigma':>8s} {'tap':>6s} {'dim':>5s} {'ridge':>8s} {'knn':>8s}"]
    for c in cells:
        lines.append(f"{c['checkpoint'][-32:]:<32s} {c['sigma']:8.4g} {c['tap']:>6s} {c['dim']:5d} "
                     f"{c['ridge_accuracy']:8.4f} {c['knn_accuracy']:8.4f}")
    return "\n".join(lines)


def best_cell(cells, key="ridge_accuracy"):
    """the cell with the highest `key`, the first of equals"""
    if not cells:
        raise ValueError("features: no cells")
    return max(cells, key=lambda c: c[key])


def _probe(args, dev):
    xtr, ytr = _read_split(args.dataset, args.data_dir, True, args.num_train)
    xte, yte = _read_split(args.dataset, args.data_dir, False, args.num_test)
    num_classes = int(max(ytr.max(), yte.max())) + 1
    sigmas = args.sweep_sigmas or [args.sigma]
    tap_sets = [[t] for t in args.sweep_taps] if args.sweep_taps else [list(args.taps)]
    cells = []
    for path in args.ckpt_path:
        model = _load_model(path, args.load_ema, dev)
        for sigma in sigmas:
            for taps in tap_sets:
                ex = FeatureExtractor(model, sigma=sigma, taps=taps, seed=args.seed, batch_size=args.batch_size,
                                      network_dtype=args.network_dtype, conditional=args.conditional)
                # (train and test images draw from disjoint noise streams: ids continue behind the training set)
                ftr = ex.extract(xtr, ytr if args.conditional else None)
                fte = ex.extract(xte, yte if args.conditional else None,
                                 ids=np.arange(xtr.shape[0], xtr.shape[0] + xte.shape[0]))
                probe = ridge_probe(ftr, ytr, num_classes, args.l2)
                cells.append({"checkpoint": path, "sigma": float(sigma), "tap": "+".join(taps), "dim": ex.dim,
                              "ridge_accuracy": probe.accuracy(fte, yte),
                              "knn_accuracy": knn_accuracy(ftr, ytr, fte, yte, args.k, num_classes=num_classes)})
                print(format_table(cells[-1:]).splitlines()[-1], flush=True)
        del model
    best = best_cell(cells)
    report = {"dataset": args.dataset, "num_train": int(xtr.shape[0]), "num_test": int(xte.shape[0]),
              "num_classes": num_classes, "k": args.k, "l2": args.l2, "seed": args.seed, "network_dtype": args.network_dtype,
              "load_ema": bool(args.load_ema), "conditional": bool(args.conditional), "cells": cells, "best": best,
              "criterion": "ridge_accuracy"}
    with open(args.report, "w") as f:
        json.dump(report, f, indent=1)
    print(format_table(cells))
    print(f"best ridge accuracy: {best['checkpoint']} sigma {best['sigma']:.4g} tap {best['tap']} "
          f"({best['ridge_accuracy']:.4f}; k-NN {best['knn_accuracy']:.4f})")
    print(f"wrote {args.report}", flush=True)
    return report


def _extract(args, dev):
    images, labels = _load_extract_data(args)
    model = _load_model(args.ckpt_path[0], args.load_ema, dev)
    ex = FeatureExtractor(model, sigma=args.sigma, taps=args.taps, seed=args.seed, batch_size=args.batch_size,
                          network_dtype=args.network_dtype, conditional=args.conditional)
    feats = ex.extract(images, labels if args.conditional else None)
    write_features(args.out, feats)
    if args.labels_out is not None:
        with open(args.labels_out, "w") as f:
            json.dump([int(v) for v in labels], f)
    print(f"wrote {args.out}: float32 {tuple(feats.shape)} (sigma {args.sigma:g}, taps {' '.join(ex.taps)})", flush=True)
    return feats


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        check_args(args)
    except ValueError as e:
        parser.error(str(e))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dev = torch.device("cuda", torch.cuda.current_device())
    return _probe(args, dev) if args.probe else _extract(args, dev)


if __name__ == "__main__":
    main()
