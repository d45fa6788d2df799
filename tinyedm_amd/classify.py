"""Diffusion-classifier evaluation: the test accuracy of a class-conditional model, judged by the model itself (Li et al.
2023, "Your Diffusion Model is Secretly a Zero-Shot Classifier"; Clark & Jaini 2023).  A conditional denoiser defines a
classifier: the class under which the denoising error of an image is lowest is the class the model believes it has.

    python -m tinyedm.classify --ckpt_path cond_a.ckpt cond_b.ckpt --load_ema --dataset cifar10 \\
        --data_dir datasets/cifar --report acc.json

Definition.  For image x with id i, levels sigma_0 < ... < sigma_{L-1} (explicit `sigmas`, or `num_levels` quantile
midpoints of the training distribution, the choice of tinyedm.evaluate), draws d < R and classes c < C:

    se[d, l, i, c] = || D(x + sigma_l * n(seed, d, i, l); sigma_l, c) - x ||^2     (fp64, ops.eval_sqerr's fixed order)
    score[i, c]    = sum_l w_l * mean_d se[d, l, i, c] / CHW                        (sequential in l, fp64, on the host)
    pred[i]        = argmin_c score[i, c]       (a tie goes to the lower class index)
    margin[i]      = second-lowest score - lowest score

The noise n is the stream of ops.eval_diffuse and belongs to (seed, draw, image id, level): it is THE SAME FOR EVERY CLASS
of an (image, level, draw).  The classes are compared on paired draws, so the noise's own contribution to the error
cancels in the comparison; this is what makes a few levels and one draw sufficient.

`weighting` selects w_l:
  "edm" (default)  lambda(sigma_l) = (sigma_l^2 + sigma_data^2) / (sigma_l sigma_data)^2, the training loss.  With the
                   quantile-midpoint levels the score is the stratified estimate of the class-conditional expected
                   training loss: tinyedm.evaluate's `expected_loss` (times L), per class.
  "eps"            1 / sigma_l^2, the epsilon-prediction error of the cited papers.
  "uniform"        1.

Determinism.  One network call holds batch_size // C whole (image, level) pairs under all C classes, row p * C + c being
pair p under class c.  ops.eval_diffuse_classes draws the noise of a pair once and stores it to its C rows;
ops.eval_sqerr_classes reduces each row against the one clean image of its pair in an order that depends on the image
size alone.  The [R, L, n, C] fp64 matrix is filled on the device, copied to the host once and reduced there in a fixed
order, so a checkpoint gives the same bits whatever the batch size, the order of the images or the number of ranks.

Precision.  The default network precision is bf16.  Where the margins of a checkpoint are of the size of the bf16
evaluation error (about 1e-2 of ||D||), predictions can flip with the precision: `margin_quantiles` (min, 5 %, 50 %) is in
the result and the report to show which case a checkpoint is in; use `network_dtype="f32x3"` then.

With labels the result also holds accuracy (and its binomial standard error), the confusion matrix (true class = row),
the accuracy of each level alone, and `true_class_loss`, which is tinyedm.evaluate's `loss` on the same images, levels
and seed.  `label_gain=True` evaluates one more row per pair without a label and reports, per level, how much knowing the
label lowers the error.  Applied to generated samples and the labels they were drawn for (`generate --labels_to`), the
accuracy says how often a guidance weight produces what was asked for.

Under torch.distributed rank r takes the ids = r (mod world); the confusion matrix and the per-level correct counts are
merged with one int64 all-reduce, the per-level (count, sum, sum of squares) with the fp64 merge of tinyedm.evaluate.
`scores`, `pred`, `margin` and `se` stay per rank.

Not here: successive elimination of classes for large C, class subsets, calibrated posteriors, prior weighting."""
from __future__ import annotations

import argparse
import json
import math
import os

import numpy as np
import torch

from .evaluate import (NETWORK_DTYPES, NoiseLevelEvaluator, _load_data, check_data_args, check_images, edm_weight,
                       level_stats, level_sums)

WEIGHTINGS = ("edm", "eps", "uniform")
MAX_TABLE_CLASSES = 16          # the confusion matrix is printed up to this many classes


# ---------------------------------------------------------------------------------------------------- host arithmetic
def class_weights(sigmas, weighting: str = "edm", sigma_data: float = 0.5) -> np.ndarray:
    """w_l of the score: fp64 [L]"""
    if weighting not in WEIGHTINGS:
        raise ValueError(f"classify: weighting must be one of {WEIGHTINGS}, got {weighting!r}")
    try:
        s = np.asarray([float(v) for v in sigmas], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"classify: sigmas must be a sequence of numbers, got {sigmas!r}") from None
    sigma_data = float(sigma_data)
    if s.ndim != 1 or s.size < 1 or not (np.isfinite(s).all() and (s > 0.0).all()):
        raise ValueError(f"classify: sigmas must be finite and > 0, got {sigmas!r}")
    if not (math.isfinite(sigma_data) and sigma_data > 0.0):
        raise ValueError(f"classify: sigma_data must be finite and > 0, got {sigma_data}")
    if weighting == "edm":
        return np.asarray([edm_weight(float(v), sigma_data) for v in s], dtype=np.float64)
    if weighting == "eps":
        return 1.0 / (s * s)
    return np.ones_like(s)


def _se4(se, who: str) -> np.ndarray:
    se = np.asarray(se, dtype=np.float64)
    if se.ndim != 4 or se.shape[0] < 1 or se.shape[1] < 1 or se.shape[3] < 1:
        raise ValueError(f"{who}: expected a [draws, L, n, C] matrix, got {se.shape}")
    return se


def class_scores(se, chw: int, weights) -> np.ndarray:
    """se: fp64 [draws, L, n, C] -> score [n, C] = sum_l w_l * mean_d se / chw, the level sum taken sequentially in
    level order"""
    se = _se4(se, "class_scores")
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if isinstance(chw, bool) or int(chw) != chw or int(chw) < 1 or w.shape[0] != se.shape[1] or not np.isfinite(w).all():
        raise ValueError(f"class_scores: expected chw >= 1 and {se.shape[1]} finite weights, got {chw!r}, {w.shape}")
    v = se.mean(axis=0) / float(int(chw))                     # [L, n, C]
    out = np.zeros(se.shape[2:], dtype=np.float64)
    for l in range(se.shape[1]):
        out = out + w[l] * v[l]
    return out


def _argmin_margin(scores: np.ndarray):
    """the lowest class of each row (np.argmin: the first, i.e. lowest, index of a tie) and second-lowest - lowest"""
    pred = np.argmin(scores, axis=1).astype(np.int64)
    if scores.shape[1] < 2:
        return pred, np.full(scores.shape[0], np.inf, dtype=np.float64)
    two = np.partition(scores, 1, axis=1)[:, :2]
    return pred, two[:, 1] - two[:, 0]


def predict(scores):
    """scores [n, C] -> (pred int64 [n], margin fp64 [n]); one class alone has margin inf"""
    scores = np.asarray(scores, dtype=np.float64)
    if scores.ndim != 2 or scores.shape[1] < 1:
        raise ValueError(f"predict: expected an [n, C] matrix with C >= 1, got {scores.shape}")
    if not np.isfinite(scores).all():
        raise ValueError("predict: the scores are not all finite")
    return _argmin_margin(scores)


def level_predictions(se) -> np.ndarray:
    """se [draws, L, n, C] -> int64 [L, n]: the argmin over the classes of one level alone (mean over the draws), a tie
    to the lower class index"""
    se = _se4(se, "level_predictions")
    if not np.isfinite(se).all():
        raise ValueError("level_predictions: the squared errors are not all finite")
    return np.argmin(se.mean(axis=0), axis=2).astype(np.int64)


def _class_indices(v, C: int, name: str) -> np.ndarray:
    a = np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"classify: {name} must be integers, got {a.dtype}")
    a = a.astype(np.int64).reshape(-1)
    if a.size and (a.min() < 0 or a.max() >= C):
        raise ValueError(f"classify: {name} must lie in [0, {C}), got [{a.min()}, {a.max()}]")
    return a


def confusion_matrix(pred, labels, C: int) -> np.ndarray:
    """int64 [C, C]: entry [t, p] counts the images of true class t predicted as p"""
    if isinstance(C, bool) or not isinstance(C, (int, np.integer)) or C < 1:
        raise ValueError(f"confusion_matrix: C must be an integer >= 1, got {C!r}")
    C = int(C)
    pred, labels = _class_indices(pred, C, "pred"), _class_indices(labels, C, "labels")
    if pred.shape != labels.shape:
        raise ValueError(f"confusion_matrix: {pred.shape[0]} predictions for {labels.shape[0]} labels")
    out = np.zeros((C, C), dtype=np.int64)
    np.add.at(out, (labels, pred), 1)
    return out


def merge_counts(parts) -> np.ndarray:
    """the element-wise int64 sum of the count arrays of several shards (confusion matrices, per-level correct counts)"""
    parts = [np.asarray(p) for p in parts]
    if not parts or any(p.shape != parts[0].shape or not np.issubdtype(p.dtype, np.integer) for p in parts):
        raise ValueError("merge_counts: expected one or more integer arrays of one shape")
    out = np.zeros(parts[0].shape, dtype=np.int64)
    for p in parts:
        out = out + p.astype(np.int64)
    return out


def classification_stats(confusion) -> dict:
    """confusion [C, C] (true class = row) -> accuracy, accuracy_stderr = sqrt(a (1 - a) / n) (None below two images),
    per_class_accuracy (None for a class with no image) and count"""
    m = np.asarray(confusion)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1 or not np.issubdtype(m.dtype, np.integer) or (m < 0).any():
        raise ValueError(f"classification_stats: expected a square matrix of counts, got {m.shape} {m.dtype}")
    n = int(m.sum())
    if n < 1:
        raise ValueError("classification_stats: no image was classified")
    a = int(np.trace(m)) / n
    rows = m.sum(axis=1)
    return {"accuracy": a, "accuracy_stderr": math.sqrt(a * (1.0 - a) / n) if n >= 2 else None,
            "per_class_accuracy": [int(m[c, c]) / int(rows[c]) if rows[c] else None for c in range(m.shape[0])],
            "count": n}


def _quantiles(margin: np.ndarray):
    """(min, 5 %, 50 %) of the margins, or None where there is no finite margin (no image, or one class)"""
    if margin.size == 0 or not np.isfinite(margin).all():
        return None
    return {"min": float(margin.min()), "p05": float(np.quantile(margin, 0.05)), "p50": float(np.quantile(margin, 0.5))}


# ---------------------------------------------------------------------------------------------------- the classifier
class DiffusionClassifier:
    """classify(model, images, labels=None, ids=None) -> the classes the model assigns to `images` (see the module text).

    sigmas / num_levels / P_mean / P_std / seed / num_draws / network_dtype / sigma_data: as NoiseLevelEvaluator, whose
    checks they pass through.  batch_size is the number of network ROWS per call: each call holds batch_size // C whole
    (image, level) pairs under every class, and it changes no bit of `se`.  num_classes defaults to the model's
    (model.embedding.num_classes); a plain callable D(x, sigma, class) needs it given.  label_gain (with labels): also
    evaluate every pair without a label."""

    def __init__(self, sigmas=None, num_levels: int = 16, P_mean=None, P_std=None, seed: int = 0, num_draws: int = 1,
                 batch_size: int = 512, network_dtype: str = "bf16", weighting: str = "edm", num_classes=None,
                 label_gain: bool = False, sigma_data: float = 0.5):
        self.levels = NoiseLevelEvaluator(sigmas=sigmas, num_levels=num_levels, P_mean=P_mean, P_std=P_std, seed=seed,
                                          num_draws=num_draws, batch_size=batch_size, network_dtype=network_dtype,
                                          sigma_data=sigma_data)
        e = self.levels
        self.sigmas, self.num_levels, self.seed, self.num_draws = e.sigmas, e.num_levels, e.seed, e.num_draws
        self.batch_size, self.network_dtype, self.sigma_data = e.batch_size, e.network_dtype, e.sigma_data
        if weighting not in WEIGHTINGS:
            raise ValueError(f"classify: weighting must be one of {WEIGHTINGS}, got {weighting!r}")
        self.weighting = weighting
        if num_classes is not None:
            if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 1:
                raise ValueError(f"classify: num_classes must be an integer >= 1, got {num_classes!r}")
            self._check_batch(num_classes)
        self.num_classes = num_classes
        if not isinstance(label_gain, bool):
            raise ValueError(f"classify: label_gain must be a bool, got {label_gain!r}")
        self.label_gain = label_gain

    def _check_batch(self, C: int) -> None:
        if self.batch_size < C:
            raise ValueError(f"classify: batch_size = {self.batch_size} network rows cannot hold one (image, level) pair "
                             f"under {C} classes")

    def classes_for(self, model) -> int:
        """the number of classes swept on `model`"""
        emb = getattr(model, "embedding", None)
        if emb is None:
            if self.num_classes is None:
                raise ValueError("classify: a plain callable needs num_classes")
            return self.num_classes
        own = getattr(emb, "num_classes", None)
        if own is None or int(own) < 1:
            raise ValueError("classify: the model is unconditional: it has no classes to tell apart")
        if self.num_classes is not None and self.num_classes != int(own):
            raise ValueError(f"classify: num_classes = {self.num_classes}, but the model has {int(own)} classes")
        self._check_batch(int(own))
        return int(own)

    @torch.no_grad()
    def classify(self, model, images, labels=None, ids=None) -> dict:
        from . import ops
        from .callbacks import _eval_dtype
        images, labels, ids_h = check_images(images, labels, ids, "classify")
        N, dev = images.shape[0], images.device
        C = self.classes_for(model)
        labels_h = None if labels is None else _class_indices(labels, C, "labels")
        sigmas = [float(np.float32(s)) for s in self.levels.levels_for(model)]      # what the kernel and the network see
        L, R, chw = len(sigmas), self.num_draws, images[0].numel()
        sigma_data = float(getattr(model, "sigma_data", self.sigma_data))
        weights = class_weights(sigmas, self.weighting, sigma_data)
        gain = self.label_gain and labels is not None

        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank() if world > 1 else 0
        order = np.argsort(ids_h, kind="stable")                  # id order
        if world > 1:
            order = order[ids_h[order] % world == rank]
        n = int(order.shape[0])
        se_h = torch.zeros(R, L, n, C, dtype=torch.float64)
        none_h = torch.zeros(R, L, n, dtype=torch.float64)
        if n:
            # the work list, level-major, built on the host, uploaded once: pair t = (level t // n, image t % n)
            total, pairs = L * n, self.batch_size // C
            item_img = torch.from_numpy(np.tile(order, L)).to(dev)
            item_ids = torch.from_numpy(np.tile(ids_h[order].astype(np.uint32), L)).to(dev)
            item_level = torch.from_numpy(np.repeat(np.arange(L, dtype=np.int32), n)).to(dev)
            sig_dev = torch.tensor(sigmas, dtype=torch.float32, device=dev)
            classes = torch.arange(C, dtype=torch.int64, device=dev).repeat(min(pairs, total))     # row p * C + c -> c
            se = torch.empty(R, L, n, C, dtype=torch.float64, device=dev)
            se_none = torch.empty(R, L, n, dtype=torch.float64, device=dev) if gain else None
            is_module = isinstance(model, torch.nn.Module)
            was_training = is_module and model.training
            if is_module:
                model.eval()
            try:
                with _eval_dtype(model, self.network_dtype):
                    for d in range(R):
                        rec = ops.churn_record(self.seed, d, dev)
                        flat = se[d].view(-1)
                        for t0 in range(0, total, pairs):
                            t1 = min(total, t0 + pairs)
                            rows = (t1 - t0) * C
                            clean = images.index_select(0, item_img[t0:t1])
                            noisy, sigma = ops.eval_diffuse_classes(clean, item_ids[t0:t1], item_level[t0:t1], sig_dev,
                                                                    rec, C, check_levels=False)   # (levels: 0 .. L - 1)
                            D = model(noisy, sigma, classes[:rows])
                            if tuple(D.shape) != tuple(noisy.shape):
                                raise ValueError(f"classify: the model returned {tuple(D.shape)} for {tuple(noisy.shape)}")
                            ops.eval_sqerr_classes(D.float().contiguous(), clean, C, out=flat[t0 * C:t1 * C])
                            if gain:        # the pair once more, label-free: its row 0 is the pair's noisy image
                                noisy1 = noisy.view(t1 - t0, C, -1)[:, 0].reshape(clean.shape).contiguous()
                                D = model(noisy1, sigma[::C].contiguous(), None)
                                ops.eval_sqerr(D.float().contiguous(), clean, out=se_none[d].view(-1)[t0:t1])
            finally:
                if was_training:
                    model.train()
            se_h = se.cpu()                                         # the one device -> host copy (two with label_gain)
            if gain:
                none_h = se_none.cpu()
            ops.check_health(dev, "DiffusionClassifier.classify")
        se_np = se_h.numpy()
        scores = class_scores(se_np, chw, weights) if n else np.zeros((0, C))
        pred, margin = predict(scores)
        out = {"sigma": sigmas, "weights": weights.tolist(), "scores": torch.from_numpy(scores), "pred": torch.from_numpy(pred),
               "margin": torch.from_numpy(margin), "margin_quantiles": _quantiles(margin),
               "pred_histogram": np.bincount(pred, minlength=C).tolist(), "se": se_h, "ids": ids_h[order].tolist(),
               "num_classes": C, "num_draws": R, "seed": self.seed, "network_dtype": self.network_dtype,
               "weighting": self.weighting, "sigma_data": sigma_data, "batch_size": self.batch_size}
        if labels is None:
            return out
        y = labels_h[order]
        rows_i = np.arange(n)
        counts = np.concatenate([confusion_matrix(pred, y, C).reshape(-1),
                                 (level_predictions(se_np) == y[None, :]).sum(axis=1).astype(np.int64) if n
                                 else np.zeros(L, dtype=np.int64)])
        sums = np.zeros((2, 3, L), dtype=np.float64)              # (count, sum, sum of squares) of: true class, gain
        sums[:, 0] = float(n)
        if n:
            true_se = se_np[:, :, rows_i, y]                       # [R, L, n]
            sums[0] = level_sums(true_se, chw)
            if gain:
                sums[1] = level_sums(none_h.numpy() - true_se, chw)
        if world > 1:
            t = torch.from_numpy(counts).to(dev)
            dist.all_reduce(t)
            counts = t.cpu().numpy()
            t = torch.from_numpy(sums).to(dev)
            dist.all_reduce(t)
            sums = t.cpu().numpy()
        confusion = counts[:C * C].reshape(C, C)
        out.update(classification_stats(confusion))
        out["confusion"] = confusion.tolist()
        out["level_accuracy"] = [int(v) / out["count"] for v in counts[C * C:]]
        out["true_class_loss"] = level_stats(sums[0], sigmas, sigma_data)["loss"]
        if gain:
            st = level_stats(sums[1], sigmas, sigma_data)
            out["label_gain"], out["label_gain_stderr"] = st["mse"], st["mse_stderr"]
            out["se_unlabelled"] = none_h
        return out


_TENSORS = ("se", "se_unlabelled", "scores", "pred", "margin", "ids")


def report_entry(result: dict) -> dict:
    """the JSON-serialisable part of a classify() result (without the matrices, the predictions and the id list)"""
    return {k: v for k, v in result.items() if k not in _TENSORS}


def best_checkpoint(entries: dict):
    """the name of the entry with the highest accuracy, a tie to the first named; None without labels"""
    if not entries:
        raise ValueError("best_checkpoint: no entries")
    if any("accuracy" not in e for e in entries.values()):
        return None
    best = None
    for k, e in entries.items():
        if best is None or e["accuracy"] > entries[best]["accuracy"]:
            best = k
    return best


# ---------------------------------------------------------------------------------------------------- command line
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Diffusion-classifier accuracy of one or more class-conditional checkpoints")
    p.add_argument("--ckpt_path", type=str, nargs="+", required=True, help="one or more checkpoints to compare")
    p.add_argument("--load_ema", action="store_true", help="evaluate the EMA weights of the checkpoints")
    p.add_argument("--dataset", choices=["cifar10", "mnist"], default=None, help="built-in test split (with --data_dir)")
    p.add_argument("--data_dir", type=str, default=None)
    p.add_argument("--image_dir", type=str, default=None, help="directory of <index>.png images (as generate writes them)")
    p.add_argument("--labels_json", type=str, default=None,
                   help="--image_dir: a JSON list of class indices, one per image in index order (generate --labels_to)")
    p.add_argument("--mean", type=float, nargs="+", default=None)
    p.add_argument("--std", type=float, nargs="+", default=None)
    p.add_argument("--image_size", type=int, default=None)
    p.add_argument("--in_channels", type=int, default=None)
    p.add_argument("--num_levels", type=int, default=16, help="levels at the quantile midpoints of the training distribution")
    p.add_argument("--sigmas", type=float, nargs="+", default=None, help="explicit levels, strictly increasing")
    p.add_argument("--weighting", choices=list(WEIGHTINGS), default="edm")
    p.add_argument("--num_images", type=int, default=1000)
    p.add_argument("--num_draws", type=int, default=1)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--batch_size", type=int, default=512, help="network rows per call: batch_size // classes pairs")
    p.add_argument("--network_dtype", choices=list(NETWORK_DTYPES), default="bf16")
    p.add_argument("--label_gain", action="store_true", help="also report how much the label lowers the error, by level")
    p.add_argument("--report", type=str, required=True, metavar="OUT.json")
    return p


def check_args(args) -> DiffusionClassifier:
    """every choice that needs nothing loaded, checked before a checkpoint or the GPU is touched; returns the classifier"""
    check_data_args(args, "classify")
    if args.label_gain and args.image_dir is not None and args.labels_json is None:
        raise ValueError("classify: --label_gain needs labels (--labels_json with --image_dir)")
    return DiffusionClassifier(sigmas=args.sigmas, num_levels=args.num_levels, seed=args.seed, num_draws=args.num_draws,
                               batch_size=args.batch_size, network_dtype=args.network_dtype, weighting=args.weighting,
                               label_gain=bool(args.label_gain))


def format_table(entries: dict) -> str:
    names = list(entries)
    first = entries[names[0]]
    lines = []
    if "accuracy" in first:
        gain = all("label_gain" in entries[k] for k in names)
        lines.append("level      sigma  " + "  ".join(f"{'acc[' + str(i) + ']':>8s}" + (f" {'gain[' + str(i) + ']':>12s}" if gain else "")
                                                 for i in range(len(names))))
        for l, s in enumerate(first["sigma"]):
            lines.append(f"{l:5d} {s:10.4g}  " + "  ".join(
                f"{entries[k]['level_accuracy'][l]:8.4f}" + (f" {entries[k]['label_gain'][l]:12.6g}" if gain else "")
                for k in names))
    for i, k in enumerate(names):
        e = entries[k]
        q = e["margin_quantiles"]
        tail = "" if q is None else f", margin min {q['min']:.3g} / 5% {q['p05']:.3g} / 50% {q['p50']:.3g}"
        if "accuracy" in e:
            err = "" if e["accuracy_stderr"] is None else f" +- {e['accuracy_stderr']:.4f}"
            lines.append(f"[{i}] {k}: accuracy {e['accuracy']:.4f}{err} on {e['count']} images{tail}")
            if e["num_classes"] <= MAX_TABLE_CLASSES:
                lines.append("    confusion (true class = row, predicted = column)")
                lines.extend("    " + " ".join(f"{v:6d}" for v in row) for row in e["confusion"])
        else:
            lines.append(f"[{i}] {k}: predicted classes {e['pred_histogram']}{tail}")
    return "\n".join(lines)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        classifier = check_args(args)
    except ValueError as e:
        parser.error(str(e))
    from .edm import EDM
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dev = torch.device("cuda", torch.cuda.current_device())
    entries, levels, data = {}, None, None
    for path in args.ckpt_path:
        model = EDM.load_from_checkpoint(path, load_ema=args.load_ema).to(dev).eval()
        if not model.conditional:
            raise ValueError(f"classify: {path} is unconditional: it has no classes to tell apart")
        if data is None:
            data = _load_data(args, model, dev, "classify")
        images, labels = data
        res = classifier.classify(model, images, labels)
        if levels is not None and res["sigma"] != levels:
            raise ValueError(f"classify: {path} has another training distribution (P_mean / P_std) than the first "
                             "checkpoint; compare them at explicit --sigmas")
        levels = res["sigma"]
        entries[path] = report_entry(res)
        del model
    best = best_checkpoint(entries)
    report = {"sigmas": levels, "num_images": int(data[0].shape[0]), "num_draws": args.num_draws, "seed": args.seed,
              "network_dtype": args.network_dtype, "weighting": args.weighting, "batch_size": args.batch_size,
              "label_gain": bool(args.label_gain), "load_ema": bool(args.load_ema), "labelled": data[1] is not None,
              "checkpoints": entries, "best": best, "criterion": None if best is None else "accuracy"}
    if int(os.environ.get("RANK", "0")) == 0:
        with open(args.report, "w") as f:
            json.dump(report, f, indent=1)
        print(format_table(entries))
        if len(entries) > 1 and best is not None:
            print(f"highest accuracy: {best} ({entries[best]['accuracy']:.4f})")
        print(f"wrote {args.report}", flush=True)
    return report


if __name__ == "__main__":
    main()
