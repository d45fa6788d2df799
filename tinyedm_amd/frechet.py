"""Frechet distance and kernel inception distance between a set of samples and a set of references.

precision / recall / density / coverage (prdc) judge the support of a sample set and the nearest-neighbour search judges
single samples; both are blind to a shift in the first two moments (a colour cast, lost contrast, over-smoothing).  These
are the two distances between distributions that the literature reports:

    FD    = |mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a S_b)^(1/2)          (Dowson & Landau 1982; with Inception pool
            features this is the FID of Heusel et al. 2017)
    MMD^2 = sum_{i != j} k(x_i, x_j) / (m (m - 1)) + sum_{i != j} k(y_i, y_j) / (m (m - 1)) - 2 sum_ij k(x_i, y_j) / m^2,
            k(x, y) = (gamma x . y + coef0)^degree, averaged over random subsets: the KID of Binkowski et al. 2018
            (defaults: 100 subsets of 1000, degree 3, gamma 1 / D, coef0 1).

The features are either the pixels themselves (uint8 images, feature u / 255: a crude space, as for prdc, but one in which
the moments are exact integers and the result is unique) or float32 vectors extracted elsewhere (Inception, DINO, ...:
no such extractor ships here; tinyedm.features takes them from the project's own denoiser).  The two reductions over a
set -- the moments sum x, sum x x^T and the kernel sums -- run in fp64 on the device (csrc/moments.hip through ops.moments and ops.poly_kernel_sums); everything after them is numpy fp64 on the
host and needs no GPU: FeatureStats, frechet_distance, subset_indices, kid_from_sums, check_args.

FD is biased upwards at a finite number of samples; read the samples' number against the one fresh data gets (`--holdout`).

    python -m tinyedm.frechet --image_dir samples --dataset cifar10 --data_dir datasets/cifar --holdout --report fd.json
    python -m tinyedm.frechet --features samples.npy --ref_features train.npy --report fd.json
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from .neighbors import _read_dataset, load_images_u8

KINDS = ("u8", "f32")
PIXEL_SCALE = 255.0     # a uint8 feature is u / 255; the statistics keep the integers and the scale is applied on the host


# ---------------------------------------------------------------------------------------------------- host arithmetic
class FeatureStats:
    """The sufficient statistics of a feature set for its mean and covariance: n, sum = sum_i (x_i - shift) [D] and
    gram = sum_i (x_i - shift)(x_i - shift)^T [D, D] in fp64.  kind "u8": the rows are uint8 pixels, shift is None and sum
    and gram are the exact integers (the feature is u / 255; mean() and cov() apply the scale).  kind "f32": float features;
    shift [D] is the vector that was subtracted before the products (the set's mean in the two-pass scheme), None for 0.
    The statistics of a union are the sums of the statistics (merge): exact for uint8."""

    def __init__(self, n, sum, gram, kind, shift=None):
        if kind not in KINDS:
            raise ValueError(f"FeatureStats: kind must be one of {KINDS}, got {kind!r}")
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"FeatureStats: n must be an integer >= 1, got {n!r}")
        self.n, self.kind = int(n), kind
        self.sum = np.asarray(sum, dtype=np.float64)
        self.gram = np.asarray(gram, dtype=np.float64)
        D = self.sum.size
        if self.sum.ndim != 1 or D < 1 or self.gram.shape != (D, D):
            raise ValueError(f"FeatureStats: expected sum [D] and gram [D, D], got {self.sum.shape} and {self.gram.shape}")
        self.shift = None if shift is None else np.asarray(shift, dtype=np.float64)
        if self.shift is not None and (kind == "u8" or self.shift.shape != (D,)):
            raise ValueError("FeatureStats: shift is a [D] vector of a float set (pixel statistics stay integers)")
        if not (np.isfinite(self.sum).all() and np.isfinite(self.gram).all()
                and (self.shift is None or np.isfinite(self.shift).all())):
            raise ValueError("FeatureStats: non-finite statistics")

    @property
    def dim(self) -> int:
        return self.sum.size

    @property
    def scale(self) -> float:
        return PIXEL_SCALE if self.kind == "u8" else 1.0

    def mean(self) -> np.ndarray:
        m = self.sum / self.n
        return (m if self.shift is None else m + self.shift) / self.scale

    def cov(self, ddof=1) -> np.ndarray:
        """the covariance of the features, symmetric by construction; ddof as in numpy.cov"""
        if self.n - ddof < 1:
            raise ValueError(f"FeatureStats.cov: n = {self.n} needs ddof < n, got {ddof}")
        c = (self.gram - np.outer(self.sum, self.sum) / self.n) / ((self.n - ddof) * self.scale ** 2)
        return (c + c.T) / 2

    def _about(self, shift):
        """(sum, gram) taken about another shift vector"""
        mine = np.zeros(self.dim) if self.shift is None else self.shift
        d = mine - (np.zeros(self.dim) if shift is None else shift)
        if not d.any():
            return self.sum, self.gram
        cross = np.outer(d, self.sum)
        return self.sum + self.n * d, self.gram + cross + cross.T + self.n * np.outer(d, d)

    def merge(self, other) -> "FeatureStats":
        """the statistics of the union of the two sets (about this set's shift)"""
        if not isinstance(other, FeatureStats) or other.kind != self.kind or other.dim != self.dim:
            raise ValueError("FeatureStats.merge: the other set must be FeatureStats of the same kind and dimension")
        s, g = other._about(self.shift)
        return FeatureStats(self.n + other.n, self.sum + s, self.gram + g, self.kind, self.shift)

    def save(self, path) -> None:
        with open(path, "wb") as f:      # (a file object: numpy does not append ".npz" to the name)
            np.savez(f, n=np.int64(self.n), sum=self.sum, gram=self.gram, kind=np.str_(self.kind),
                     shift=np.zeros(0) if self.shift is None else self.shift)

    @classmethod
    def load(cls, path) -> "FeatureStats":
        with np.load(path, allow_pickle=False) as z:
            missing = {"n", "sum", "gram", "kind", "shift"} - set(z.files)
            if missing:
                raise ValueError(f"FeatureStats.load: {path} lacks {sorted(missing)}")
            shift = z["shift"]
            return cls(int(z["n"]), z["sum"], z["gram"], str(z["kind"]), None if shift.size == 0 else shift)


def _mean_difference(a: FeatureStats, b: FeatureStats) -> np.ndarray:
    if a.kind == "u8" and b.kind == "u8":     # one division of exact integers per element
        return (a.sum * b.n - b.sum * a.n) / (float(a.n) * b.n * PIXEL_SCALE)
    return a.mean() - b.mean()


def frechet_distance(a: FeatureStats, b: FeatureStats) -> dict:
    """-> {"fd", "mean_term", "trace_term", "clipped_eigenvalues", "rank_deficient"} with fd = mean_term + trace_term,
    mean_term = |mu_a - mu_b|^2 and trace_term = tr S_a + tr S_b - 2 tr (S_a S_b)^(1/2).  The last trace is the sum of
    sqrt(max(lambda, 0)) over the eigenvalues of S_a^(1/2) S_b S_a^(1/2), a symmetric matrix with the spectrum of S_a S_b: two
    symmetric eigendecompositions, no general matrix square root.  clipped_eigenvalues counts the negative eigenvalues that
    were set to 0 (of S_a for its root, and of the product); rank_deficient: n <= D in either set, so that a covariance is
    singular and the distance says little (reported, not refused)."""
    if not isinstance(a, FeatureStats) or not isinstance(b, FeatureStats):
        raise ValueError("frechet_distance: expected two FeatureStats")
    if a.dim != b.dim:
        raise ValueError(f"frechet_distance: the sets have {a.dim} and {b.dim} features")
    if a.n < 2 or b.n < 2:
        raise ValueError(f"frechet_distance: a covariance needs 2 rows in each set, got {a.n} and {b.n}")
    d = _mean_difference(a, b)
    sa, sb = a.cov(), b.cov()
    w, q = np.linalg.eigh(sa)
    root = (q * np.sqrt(np.maximum(w, 0.0))) @ q.T
    m = root @ sb @ root
    lam = np.linalg.eigvalsh((m + m.T) / 2)
    mean_term = float(d @ d)
    trace_term = float(np.trace(sa) + np.trace(sb) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())
    return {"fd": mean_term + trace_term, "mean_term": mean_term, "trace_term": trace_term,
            "clipped_eigenvalues": int((w < 0).sum() + (lam < 0).sum()),
            "rank_deficient": bool(a.n <= a.dim or b.n <= b.dim)}


def _count(v, name, low):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low:
        raise ValueError(f"frechet: {name} must be an integer >= {low}, got {v!r}")
    return int(v)


def subset_indices(n_x, n_y, num_subsets, subset_size, seed) -> tuple:
    """(ix, iy) int64 [num_subsets, subset_size]: for each subset in turn, subset_size rows of the n_x drawn without
    replacement and then subset_size of the n_y, from numpy.random.default_rng(seed)"""
    n_x, n_y = _count(n_x, "n_x", 1), _count(n_y, "n_y", 1)
    S, m = _count(num_subsets, "num_subsets", 1), _count(subset_size, "subset_size", 2)
    if m > min(n_x, n_y):
        raise ValueError(f"frechet: subset_size {m} exceeds the smaller set ({min(n_x, n_y)} rows)")
    rng = np.random.default_rng(seed)
    ix, iy = np.empty((S, m), dtype=np.int64), np.empty((S, m), dtype=np.int64)
    for s in range(S):
        ix[s] = rng.choice(n_x, m, replace=False)
        iy[s] = rng.choice(n_y, m, replace=False)
    return ix, iy


def kid_from_sums(sxx, syy, sxy, m) -> dict:
    """sxx, syy [S]: the kernel sums inside each set over the pairs i != j; sxy [S]: over all pairs across the sets; m: the
    subset size, or (m_x, m_y) -> the unbiased MMD^2 of every subset, their mean ("kid") and standard deviation ("std",
    ddof 0; over one subset: 0)"""
    mx, my = (m, m) if isinstance(m, (int, np.integer)) else m
    mx, my = _count(mx, "m", 2), _count(my, "m", 2)
    sxx, syy, sxy = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (sxx, syy, sxy))
    if not (sxx.size == syy.size == sxy.size >= 1):
        raise ValueError(f"kid_from_sums: expected three lists of one length, got {sxx.size}, {syy.size}, {sxy.size}")
    per = sxx / (mx * (mx - 1)) + syy / (my * (my - 1)) - 2.0 * sxy / (mx * my)
    return {"kid": float(per.mean()), "std": float(per.std()), "per_subset": per.tolist()}


def check_kernel(degree, gamma, coef0) -> None:
    if isinstance(degree, bool) or not isinstance(degree, (int, np.integer)) or not 1 <= degree <= 4:
        raise ValueError(f"frechet: degree must be an integer in [1, 4], got {degree!r}")
    if gamma is not None and not (np.isfinite(gamma) and gamma > 0):
        raise ValueError(f"frechet: gamma must be None (1 / D) or finite and > 0, got {gamma!r}")
    if not np.isfinite(coef0):
        raise ValueError(f"frechet: coef0 must be finite, got {coef0!r}")


# ---------------------------------------------------------------------------------------------------- the device path
def _to_device(x, device):
    """uint8 [n, ...] images or float32 [n, D] features (numpy or torch) -> a contiguous device tensor"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.float32) or t.dim() < 2 or t.numel() == 0:
        what = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"frechet: a set is uint8 [n, ...] images or float32 [n, D] features, got {what} (convert "
                         "features with .float())")
    t = t.to(device).contiguous()
    if t.dtype == torch.float32 and not bool(torch.isfinite(t).all()):
        raise ValueError("frechet: non-finite features")
    return t


def feature_stats(x, index=None) -> FeatureStats:
    """the FeatureStats of the rows of a device tensor (uint8 images or finite float32 features); index: an int64 numpy
    array or device tensor of the rows that take part (None: all).  uint8: one pass, exact integers.  float32: pass one
    takes the column sums and the mean, pass two the moments with shift = mean."""
    import torch
    from . import ops
    if index is not None:
        index = torch.as_tensor(np.asarray(index, dtype=np.int64) if not isinstance(index, torch.Tensor) else index,
                                device=x.device)
    n = x.shape[0] if index is None else int(index.shape[0])
    if x.dtype == torch.uint8:
        s, g = ops.moments(x, index)
        return FeatureStats(n, s.cpu().numpy(), g.cpu().numpy(), "u8")
    mean = ops.moments(x, index, sums_only=True)[0] / n
    s, g = ops.moments(x, index, shift=mean)
    return FeatureStats(n, s.cpu().numpy(), g.cpu().numpy(), "f32", mean.cpu().numpy())


def kid(x, y, num_subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=0) -> dict:
    """The kernel inception distance of two device tensors (both uint8 images or both float32 features of one row length):
    the unbiased MMD^2 under (gamma x . y + coef0)^degree over num_subsets random subsets of subset_size rows of each set
    (subset_indices), -> kid_from_sums plus the settings.  gamma None: 1 / D.  uint8 rows are the features u / 255 (the
    kernel gets gamma / 255^2).  num_subsets = 0: the full-set estimator, every row of each set once (the sets may differ
    in size)."""
    import torch
    from . import ops
    check_kernel(degree, gamma, coef0)
    if x.dtype != y.dtype or x.shape[1:] != y.shape[1:]:
        raise ValueError(f"frechet: the sets differ in kind or row shape: {x.dtype} {tuple(x.shape[1:])} and {y.dtype} "
                         f"{tuple(y.shape[1:])}")
    D = x[0].numel()
    g = (1.0 / D if gamma is None else float(gamma)) / (PIXEL_SCALE ** 2 if x.dtype == torch.uint8 else 1.0)
    S = _count(num_subsets, "num_subsets", 0)
    if S == 0:
        if min(x.shape[0], y.shape[0]) < 2:
            raise ValueError("frechet: the full-set estimator needs 2 rows in each set")
        ix = iy = None
        m = (int(x.shape[0]), int(y.shape[0]))
    else:
        hx, hy = subset_indices(x.shape[0], y.shape[0], S, subset_size, seed)
        ix, iy = torch.from_numpy(hx).to(x.device), torch.from_numpy(hy).to(x.device)
        m = int(subset_size)
    sxx = ops.poly_kernel_sums(x, ix, x, ix, g, coef0, int(degree), True).cpu().numpy()
    syy = ops.poly_kernel_sums(y, iy, y, iy, g, coef0, int(degree), True).cpu().numpy()
    sxy = ops.poly_kernel_sums(x, ix, y, iy, g, coef0, int(degree), False).cpu().numpy()
    out = kid_from_sums(sxx, syy, sxy, m)
    out.update(num_subsets=S, subset_size=None if S == 0 else m, degree=int(degree),
               gamma=1.0 / D if gamma is None else float(gamma), coef0=float(coef0), seed=seed)
    return out


_kid = kid       # (DistributionDistance.score has a flag of that name)


def _labels(labels, n, name):
    a = np.asarray(labels)
    if a.shape != (n,) or a.dtype.kind not in "iu":
        raise ValueError(f"frechet: {name} must be {n} integer class indices, got {a.dtype} {a.shape}")
    return a.astype(np.int64)


class DistributionDistance:
    """Frechet distance and KID of sample sets against one resident reference set.  refs: uint8 [M, ...] images or float32
    [M, D] features (numpy or torch; moved to `device`).  The references' FeatureStats are taken here once (or passed in as
    ref_stats, e.g. FeatureStats.load of an earlier run)."""

    def __init__(self, refs, device=None, ref_stats=None):
        import torch
        if device is None:
            on_gpu = isinstance(refs, torch.Tensor) and refs.is_cuda
            device = refs.device if on_gpu else torch.device("cuda", torch.cuda.current_device())
        self.refs = _to_device(refs, device)
        self.stats = feature_stats(self.refs) if ref_stats is None else ref_stats
        kind = "u8" if self.refs.dtype == torch.uint8 else "f32"
        if (not isinstance(self.stats, FeatureStats) or self.stats.kind != kind or self.stats.n != self.refs.shape[0]
                or self.stats.dim != self.refs[0].numel()):
            raise ValueError("DistributionDistance: ref_stats are not the statistics of this reference set")

    def score(self, samples, labels=None, ref_labels=None, kid=True, **kid_args) -> dict:
        """-> {"num_refs", "num_samples", "fd": frechet_distance, "kid": kid(...) unless kid is False, "per_class":
        {label: frechet_distance of the two sets restricted to the class, or {"skipped": reason, ...} where either set holds
        fewer than 2 images of it} with both label arrays}.  kid_args go to kid()."""
        if (labels is None) != (ref_labels is None):
            raise ValueError("DistributionDistance.score: give both labels and ref_labels, or neither")
        x = _to_device(samples, self.refs.device)
        if x.dtype != self.refs.dtype or x.shape[1:] != self.refs.shape[1:]:
            raise ValueError(f"DistributionDistance.score: samples {x.dtype} {tuple(x.shape[1:])} and references "
                             f"{self.refs.dtype} {tuple(self.refs.shape[1:])} differ")
        if x.shape[0] < 2 or self.refs.shape[0] < 2:
            raise ValueError("DistributionDistance.score: a covariance needs 2 rows in each set")
        out = {"num_refs": int(self.refs.shape[0]), "num_samples": int(x.shape[0]),
               "fd": frechet_distance(feature_stats(x), self.stats)}
        if kid:
            out["kid"] = _kid(x, self.refs, **kid_args)
        if labels is not None:
            sl, rl = _labels(labels, x.shape[0], "labels"), _labels(ref_labels, self.refs.shape[0], "ref_labels")
            table = {}
            for c in sorted(set(sl.tolist()) | set(rl.tolist())):
                si, ri = np.nonzero(sl == c)[0], np.nonzero(rl == c)[0]
                if min(si.size, ri.size) < 2:
                    table[int(c)] = {"skipped": "a covariance needs 2 images of the class in each set",
                                     "num_refs": int(ri.size), "num_samples": int(si.size)}
                else:
                    table[int(c)] = dict(frechet_distance(feature_stats(x, si), feature_stats(self.refs, ri)),
                                         num_refs=int(ri.size), num_samples=int(si.size))
            out["per_class"] = table
        return out


# ---------------------------------------------------------------------------------------------------- command line
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Frechet distance and KID of generated samples, in pixel space or on given features")
    p.add_argument("--image_dir", type=str, default=None, help="directory of <index>.png samples (as generate writes them)")
    p.add_argument("--dataset", choices=["cifar10", "mnist"], default=None, help="references: built-in train split")
    p.add_argument("--data_dir", type=str, default=None)
    p.add_argument("--ref_image_dir", type=str, default=None, help="references: a directory of <index>.png images")
    p.add_argument("--features", type=str, default=None, metavar="A.npy", help="samples as a float32 [n, D] array")
    p.add_argument("--ref_features", type=str, default=None, metavar="B.npy", help="references as a float32 [n, D] array")
    p.add_argument("--holdout", action="store_true",
                   help="with --dataset: also score the test split against the same references (the number to read the "
                        "samples against: FD is biased upwards at a finite number of samples)")
    p.add_argument("--labels_json", type=str, default=None,
                   help="a JSON list of the samples' class indices in index order (generate --labels_to): adds the per-class "
                        "table; the references' labels come from --dataset")
    p.add_argument("--num_subsets", type=int, default=100, help="KID subsets (0: the full-set estimator)")
    p.add_argument("--subset_size", type=int, default=1000)
    p.add_argument("--degree", type=int, default=3)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--no_kid", action="store_true", help="the Frechet distance only")
    p.add_argument("--ref_stats", type=str, default=None, metavar="IN.npz", help="the references' statistics of an earlier run")
    p.add_argument("--save_ref_stats", type=str, default=None, metavar="OUT.npz")
    p.add_argument("--report", type=str, required=True, metavar="OUT.json")
    return p


def check_args(args) -> None:
    """every choice that needs nothing loaded, checked before a file or the GPU is touched"""
    pixel = args.image_dir is not None or args.dataset is not None or args.ref_image_dir is not None
    feat = args.features is not None or args.ref_features is not None
    if pixel and feat:
        raise ValueError("frechet: give images (--image_dir with --dataset or --ref_image_dir) or features (--features with "
                         "--ref_features), not both")
    if feat:
        if args.features is None or args.ref_features is None:
            raise ValueError("frechet: the feature form needs both --features and --ref_features")
        if args.holdout or args.labels_json is not None or args.data_dir is not None:
            raise ValueError("frechet: --holdout, --labels_json and --data_dir go with --dataset")
    else:
        if args.image_dir is None:
            raise ValueError("frechet: give the samples with --image_dir (or --features)")
        if (args.dataset is None) == (args.ref_image_dir is None):
            raise ValueError("frechet: give exactly one source of references: --dataset cifar10|mnist --data_dir DIR, or "
                             "--ref_image_dir DIR")
        if args.dataset is not None and args.data_dir is None:
            raise ValueError("frechet: --dataset needs --data_dir")
        if args.dataset is None and args.data_dir is not None:
            raise ValueError("frechet: --data_dir goes with --dataset")
        if args.holdout and args.dataset is None:
            raise ValueError("frechet: --holdout takes the test split of --dataset")
        if args.labels_json is not None and args.dataset is None:
            raise ValueError("frechet: --labels_json needs a labelled set of references (--dataset): a directory of images "
                             "has no labels")
    if args.ref_stats is not None and args.save_ref_stats is not None:
        raise ValueError("frechet: give --ref_stats or --save_ref_stats, not both")
    _count(args.num_subsets, "--num_subsets", 0)
    _count(args.subset_size, "--subset_size", 2)
    check_kernel(args.degree, None, 1.0)
    if isinstance(args.seed, bool) or not isinstance(args.seed, int) or args.seed < 0:
        raise ValueError(f"frechet: --seed must be an integer >= 0, got {args.seed!r}")


def _read_features(path, name):
    a = np.load(path, allow_pickle=False)
    if a.dtype != np.float32 or a.ndim != 2 or a.shape[0] < 2 or a.shape[1] < 1:
        raise ValueError(f"frechet: {name} must hold a float32 [n >= 2, D] array, got {a.dtype} {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"frechet: {name} holds non-finite features")
    return a


def check_sets(refs, sets, num_subsets, subset_size) -> None:
    """the loaded sets against each other and against the KID subsets, still before the GPU is touched"""
    for name, x in sets.items():
        if x.shape[1:] != refs.shape[1:]:
            raise ValueError(f"frechet: {name} rows are {tuple(x.shape[1:])}, the references {tuple(refs.shape[1:])}")
        if min(x.shape[0], refs.shape[0]) < 2:
            raise ValueError(f"frechet: a covariance needs 2 rows in each set (references and {name})")
        if num_subsets > 0 and subset_size > min(x.shape[0], refs.shape[0]):
            raise ValueError(f"frechet: --subset_size {subset_size} exceeds the smaller of references and {name} "
                             f"({min(x.shape[0], refs.shape[0])} rows)")


def format_table(report) -> str:
    lines = [f"{'set':12s} {'FD':>12s} {'mean term':>12s} {'trace term':>12s} {'KID':>12s} {'KID std':>12s}"]
    for name in ("samples", "holdout"):
        if name in report:
            r = report[name]
            k = r.get("kid")
            tail = f" {k['kid']:12.6g} {k['std']:12.6g}" if k else ""
            lines.append(f"{name:12s} {r['fd']['fd']:12.6g} {r['fd']['mean_term']:12.6g} {r['fd']['trace_term']:12.6g}" + tail)
    for label, c in report.get("samples", {}).get("per_class", {}).items():
        row = "skipped: " + c["skipped"] if "skipped" in c else f"{c['fd']:12.6g} {c['mean_term']:12.6g} {c['trace_term']:12.6g}"
        lines.append(f"{'class ' + label:12s} {row}")
    return "\n".join(lines)


def _json_keys(score) -> dict:
    score = dict(score)
    if "per_class" in score:
        score["per_class"] = {str(c): v for c, v in score["per_class"].items()}
    return score


def main(argv=None):
    from .prdc import _read_dataset_labels, _read_sample_labels
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        check_args(args)
        ref_labels = None
        if args.features is not None:
            refs = _read_features(args.ref_features, "--ref_features")
            sets = {"samples": _read_features(args.features, "--features")}
            space = "features as given (float32)"
        else:
            refs = _read_dataset(args.dataset, args.data_dir, True) if args.dataset is not None else load_images_u8(args.ref_image_dir)
            if args.labels_json is not None:
                ref_labels = _read_dataset_labels(args.dataset, args.data_dir)
            sets = {"samples": load_images_u8(args.image_dir, refs.shape[2:], refs.shape[1])}
            if args.holdout:
                sets["holdout"] = _read_dataset(args.dataset, args.data_dir, False)
            space = "pixels / 255 (exact integer moments): read the samples against the holdout entry"
        check_sets(refs, sets, args.num_subsets, args.subset_size)
        labels = None if args.labels_json is None else _read_sample_labels(args.labels_json, sets["samples"].shape[0])
        ref_stats = None if args.ref_stats is None else FeatureStats.load(args.ref_stats)
    except ValueError as e:
        parser.error(str(e))
    import torch
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    try:
        dd = DistributionDistance(refs, ref_stats=ref_stats)
    except ValueError as e:
        parser.error(str(e))
    if args.save_ref_stats is not None:
        dd.stats.save(args.save_ref_stats)
    kid_args = dict(num_subsets=args.num_subsets, subset_size=args.subset_size, degree=args.degree, seed=args.seed)
    report = {"space": space, "num_refs": int(refs.shape[0]), "feature_dim": int(dd.stats.dim)}
    for name, x in sets.items():
        with_labels = name == "samples" and labels is not None
        report[name] = _json_keys(dd.score(x, labels if with_labels else None, ref_labels if with_labels else None,
                                           kid=not args.no_kid, **kid_args))
    with open(args.report, "w") as f:
        json.dump(report, f, indent=1)
    print(format_table(report))
    print(f"wrote {args.report}", flush=True)
    return report


if __name__ == "__main__":
    main()
