"""Precision, recall, density and coverage of a set of samples against a set of real images, in pixel space and exact.

The other evaluation tools judge a checkpoint or single images; these four numbers judge a set of samples as a
distribution.  Around every real image lies the closed ball that reaches its k-th nearest other real image, and likewise
around every sample.  With X the M reals, Y the N samples, d2 the exact integer squared pixel distance, rX[i] the k-th
smallest d2(X_i, X_i') over i' != i and rY[j] the same inside Y (exclusion by index: an exact duplicate is a neighbour at
distance 0, so a radius can be 0):

    hitsX[j] = #{ i : d2(Y_j, X_i) <= rX[i] }      hitsY[i] = #{ j : d2(X_i, Y_j) <= rY[j] }      nearY[i] = min_j d2(X_i, Y_j)
    precision = #{ j : hitsX[j] > 0 } / N          density  = sum_j hitsX[j] / (k N)
    recall    = #{ i : hitsY[i] > 0 } / M          coverage = #{ i : nearY[i] <= rX[i] } / M

(improved precision and recall: Kynkaanniemi et al. 2019; density and coverage: Naeem et al. 2020).  Precision and density
ask whether the samples lie where the data lies (fidelity); recall and coverage whether they reach all of it (diversity:
mode dropping, a class collapsed under strong guidance).  Everything is an integer until the final ratio, so the result
is unique: the counts come from csrc/neighbors.hip (ops.u8_knn, ops.u8_ball_count) and are tested bit for bit.

Pixel space is a cruder yardstick than the feature spaces these metrics were defined in: two images of the same object a
few pixels apart are far from each other, so the numbers are low in absolute terms and say little about perceptual
quality.  At 28 x 28 and 32 x 32 they do separate a loss of fidelity from a loss of modes.  Read them against the score
that fresh data gets (`--holdout`: at finite sample sizes real against real is below 1), never against 1.

    python -m tinyedm.prdc --image_dir samples --dataset cifar10 --data_dir datasets/cifar --k 3 5 10 --holdout \\
        --report prdc.json

The feature-space form, the one the two papers define: float32 [n, D] features extracted elsewhere (the arrays
`tinyedm.frechet --features` takes; tinyedm.features writes them from the project's own denoiser) in place of the images.
The same definitions then run on fp64 squared Euclidean distances (csrc/neighbors_f32.hip: ops.f32_knn, ops.f32_ball_count; the k-th neighbour radius of the search
is bit for bit the number the ball count compares against), and only the ratios' inputs are floats:

    python -m tinyedm.prdc --features samples.npy --ref_features train.npy --holdout_features test.npy \\
        --labels_json drawn.json --ref_labels train_labels.json --k 3 5 10 --report prdc.json

check_k, radii_from_knn, metrics_from_counts, per_class and check_args are plain numpy on the host and need no GPU.
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from .neighbors import FEATURE_SPACE, MAX_K, _read_dataset, as_set, feature_form, load_images_u8, read_feature_sets

RATIOS = ("precision", "recall", "density", "coverage")


# ---------------------------------------------------------------------------------------------------- host arithmetic
def check_k(k, num_real=None, num_fake=None) -> tuple:
    """k: an integer or a sequence of integers, each in [1, 32] and at most min(num_real, num_fake) - 1 (a set size that is
    None is not checked) -> the distinct values, ascending"""
    ks = (k,) if isinstance(k, (int, np.integer)) and not isinstance(k, bool) else k
    try:
        ks = tuple(ks)
    except TypeError:
        raise ValueError(f"prdc: k must be an integer or a sequence of integers, got {k!r}") from None
    if not ks:
        raise ValueError("prdc: no k given")
    for v in ks:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_K:
            raise ValueError(f"prdc: k must be an integer in [1, {MAX_K}], got {v!r}")
    sizes = [int(n) for n in (num_real, num_fake) if n is not None]
    if sizes and max(ks) > min(sizes) - 1:
        raise ValueError(f"prdc: k = {max(ks)} needs at least {max(ks) + 1} images in each set (the k-th neighbour besides the "
                         f"image itself), got {' and '.join(str(n) for n in sizes)}")
    return tuple(sorted({int(v) for v in ks}))


def radii_from_knn(dist, ks) -> dict:
    """dist [n, kmax]: the ascending distances of a self-search with exclude_self (numpy or torch) -> {k: dist[:, k - 1]}:
    a k-nearest list is a prefix of a longer one, so one search at max(ks) serves every k"""
    ks = check_k(ks)
    if len(dist.shape) != 2 or dist.shape[1] < max(ks):
        raise ValueError(f"radii_from_knn: dist must be [n, >= {max(ks)}], got {tuple(dist.shape)}")
    return {k: dist[:, k - 1] for k in ks}


def metrics_from_counts(hits_x, hits_y, near_y, r_x, k: int) -> dict:
    """hits_x [N] (per sample, the real balls that hold it), hits_y [M] (per real, the sample balls that hold it), near_y [M]
    (per real, d2 to its nearest sample), r_x [M] (the reals' radii at this k) -> the four ratios, their integer numerators
    and the set sizes.  Float near_y and r_x (the feature form: fp64 distances as the search returned them) are compared as
    fp64, both lists then being floats; integer ones as int64."""
    hx, hy = np.asarray(hits_x, dtype=np.int64).reshape(-1), np.asarray(hits_y, dtype=np.int64).reshape(-1)
    ny, rx = np.asarray(near_y), np.asarray(r_x)
    if ny.dtype.kind == "f" or rx.dtype.kind == "f":
        if ny.dtype.kind != "f" or rx.dtype.kind != "f":
            raise ValueError("metrics_from_counts: near_y and r_x must both be float (feature) or both integer (pixel) distances")
        ny, rx = ny.astype(np.float64).reshape(-1), rx.astype(np.float64).reshape(-1)
        if not (np.isfinite(ny).all() and np.isfinite(rx).all()):
            raise ValueError("metrics_from_counts: non-finite distances")
    else:
        ny, rx = ny.astype(np.int64).reshape(-1), rx.astype(np.int64).reshape(-1)
    (k,) = check_k(k)
    N, M = int(hx.size), int(hy.size)
    if N < 1 or M < 1 or ny.size != M or rx.size != M:
        raise ValueError(f"metrics_from_counts: expected hits_x [N], hits_y / near_y / r_x [M], got {hx.size}, {hy.size}, "
                         f"{ny.size}, {rx.size}")
    if (hx < 0).any() or (hy < 0).any() or (ny < 0).any() or (rx < 0).any():
        raise ValueError("metrics_from_counts: counts, distances and radii are non-negative")
    num = {"precision_count": int((hx > 0).sum()), "recall_count": int((hy > 0).sum()), "density_sum": int(hx.sum()),
           "coverage_count": int((ny <= rx).sum())}
    return {"k": k, "num_real": M, "num_fake": N,
            "precision": num["precision_count"] / N, "recall": num["recall_count"] / M,
            "density": num["density_sum"] / (k * N), "coverage": num["coverage_count"] / M, **num}


def _labels(labels, n, name):
    a = np.asarray(labels)
    if a.shape != (n,) or a.dtype.kind not in "iu":
        raise ValueError(f"prdc: {name} must be {n} integer class indices, got {a.dtype} {a.shape}")
    return a.astype(np.int64)


def per_class(score, real, fake, real_labels, fake_labels, ks) -> dict:
    """Every class on its own: both sets restricted to the images of one label, radii and all.  score(real_c, fake_c, ks)
    -> {k: metrics} is what scores a pair of sets (ManifoldMetrics passes its device path); real / fake are indexed by
    integer arrays.  -> {k: {label: metrics}}; a class with fewer than k + 1 images in either set has no k-th neighbour
    and is reported as {"skipped": reason, "num_real", "num_fake"}, not as zero."""
    ks = check_k(ks)
    rl, fl = _labels(real_labels, len(real), "real_labels"), _labels(fake_labels, len(fake), "fake_labels")
    out = {k: {} for k in ks}
    for c in sorted(set(rl.tolist()) | set(fl.tolist())):
        ri, fi = np.nonzero(rl == c)[0], np.nonzero(fl == c)[0]
        usable = tuple(k for k in ks if k <= min(ri.size, fi.size) - 1)
        got = score(real[ri], fake[fi], usable) if usable else {}
        for k in ks:
            out[k][int(c)] = got[k] if k in usable else {
                "skipped": f"k = {k} needs {k + 1} images of the class in each set", "num_real": int(ri.size),
                "num_fake": int(fi.size)}
    return out


# ---------------------------------------------------------------------------------------------------- the device path
def _to_device(x, device):
    """uint8 [n, ...] images or finite float32 [n, D] features, on the device"""
    return as_set(x, "prdc").to(device).contiguous()


def _search_ops(t):
    """(knn, ball_count) for a set's kind: the exact integer kernels for uint8 images, the fp64 ones for float32 features"""
    import torch
    from . import ops
    return (ops.f32_knn, ops.f32_ball_count) if t.dtype == torch.float32 else (ops.u8_knn, ops.u8_ball_count)


def _score_sets(real, fake, ks, ref_chunk, real_dist=None, per_sample=False) -> dict:
    """real, fake: both uint8 or both float32, on one device; real_dist: the reals' self-search at >= max(ks), if the caller
    holds it.  Radii and distances stay what the search returned (int64 or fp64) up to the compares."""
    knn, ball_count = _search_ops(real)
    kmax = max(ks)
    if real_dist is None:
        real_dist = knn(real, real, kmax, exclude_self=True, ref_chunk=ref_chunk)[0]
    r_x = radii_from_knn(real_dist, ks)
    r_y = radii_from_knn(knn(fake, fake, kmax, exclude_self=True, ref_chunk=ref_chunk)[0], ks)
    near_y = knn(real, fake, 1, ref_chunk=ref_chunk)[0][:, 0].cpu().numpy()
    out = {}
    for k in ks:
        hits_x = ball_count(fake, real, r_x[k], ref_chunk=ref_chunk).cpu().numpy()
        hits_y = ball_count(real, fake, r_y[k], ref_chunk=ref_chunk).cpu().numpy()
        out[k] = metrics_from_counts(hits_x, hits_y, near_y, r_x[k].cpu().numpy(), k)
        if per_sample:
            out[k]["per_sample"] = {"hits_x": hits_x.tolist(), "real_reached": (hits_y > 0).tolist()}
    return out


class ManifoldMetrics:
    """Precision, recall, density and coverage of sample sets against one resident set of reals.  real_u8: uint8 [M, ...]
    images (exact integer pixel distances) or float32 [M, D] features (fp64 Euclidean distances, the space the metrics were
    defined in), numpy or torch, moved to `device`; the samples must be of the same kind.  k: an integer or a sequence.  The reals' radii for every k come from one self-search
    at max(k), run here once."""

    def __init__(self, real_u8, k=5, ref_chunk=None, device=None):
        import torch
        if ref_chunk is not None and (isinstance(ref_chunk, bool) or not isinstance(ref_chunk, int) or ref_chunk < 1):
            raise ValueError(f"ManifoldMetrics: ref_chunk must be None or an integer >= 1, got {ref_chunk!r}")
        self.ks = check_k(k, num_real=len(real_u8))
        if device is None:
            on_gpu = isinstance(real_u8, torch.Tensor) and real_u8.is_cuda
            device = real_u8.device if on_gpu else torch.device("cuda", torch.cuda.current_device())
        self.real = _to_device(real_u8, device)
        self.ref_chunk = ref_chunk
        self.real_dist = _search_ops(self.real)[0](self.real, self.real, max(self.ks), exclude_self=True, ref_chunk=ref_chunk)[0]
        self.r_x = radii_from_knn(self.real_dist, self.ks)

    def score(self, fake_u8, real_labels=None, fake_labels=None, per_sample=False) -> dict:
        """-> {k: metrics}.  Per call: one self-search of the samples, one ball count each way per k, one 1-NN search from
        the reals to the samples.  With both label arrays metrics["per_class"] = {label: metrics or a skipped entry}, both
        sets restricted to the class.  per_sample adds metrics["per_sample"] = {"hits_x": per sample, the real balls that hold
        it (0: outside the data manifold), "real_reached": per real, whether a sample ball holds it (false: missed)}."""
        if (real_labels is None) != (fake_labels is None):
            raise ValueError("ManifoldMetrics.score: give both real_labels and fake_labels, or neither")
        check_k(self.ks, self.real.shape[0], len(fake_u8))
        fake = _to_device(fake_u8, self.real.device)
        if fake.dtype != self.real.dtype:
            raise ValueError(f"ManifoldMetrics.score: the samples are {fake.dtype}, the reals {self.real.dtype}: both sets must "
                             "be uint8 images or both float32 features")
        if fake.shape[1:] != self.real.shape[1:]:
            raise ValueError(f"ManifoldMetrics.score: samples {tuple(fake.shape[1:])} and reals {tuple(self.real.shape[1:])} "
                             "differ in shape")
        out = _score_sets(self.real, fake, self.ks, self.ref_chunk, self.real_dist, per_sample)
        if real_labels is not None:
            classes = per_class(lambda r, f, ks: _score_sets(r, f, ks, self.ref_chunk),
                                _Rows(self.real), _Rows(fake), real_labels, fake_labels, self.ks)
            for k in self.ks:
                out[k]["per_class"] = classes[k]
        return out


class _Rows:
    """a device tensor that per_class can index with a numpy integer array"""

    def __init__(self, t):
        self.t = t

    def __len__(self):
        return self.t.shape[0]

    def __getitem__(self, idx):
        import torch
        return self.t[torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(self.t.device)]


# ---------------------------------------------------------------------------------------------------- command line
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Exact pixel-space precision, recall, density and coverage of generated samples")
    p.add_argument("--image_dir", type=str, default=None, help="directory of <index>.png samples (as generate writes them)")
    p.add_argument("--dataset", choices=["cifar10", "mnist"], default=None, help="reals: built-in train split")
    p.add_argument("--data_dir", type=str, default=None)
    p.add_argument("--ref_image_dir", type=str, default=None, help="reals: a directory of <index>.png images")
    p.add_argument("--num_real", type=int, default=None, help="use the first N reals only")
    p.add_argument("--k", type=int, nargs="+", default=[5])
    p.add_argument("--holdout", action="store_true",
                   help="with --dataset: also score the test split against the same reals (the number to read the samples against)")
    p.add_argument("--holdout_image_dir", type=str, default=None, help="held-out images as a directory of <index>.png")
    p.add_argument("--labels_json", type=str, default=None,
                   help="a JSON list of the samples' class indices in index order (generate --labels_to): adds the per-class "
                        "table; the reals' labels come from --dataset")
    p.add_argument("--features", type=str, default=None, metavar="A.npy", help="samples as a float32 [n, D] array")
    p.add_argument("--ref_features", type=str, default=None, metavar="B.npy", help="reals as a float32 [n, D] array")
    p.add_argument("--holdout_features", type=str, default=None, metavar="C.npy",
                   help="held-out rows as a float32 [n, D] array, scored against the same reals")
    p.add_argument("--ref_labels", type=str, default=None,
                   help="with --ref_features and --labels_json: a JSON list of the reals' class indices in row order")
    p.add_argument("--ref_chunk", type=int, default=None, help="search the references this many rows at a time")
    p.add_argument("--per_sample", action="store_true", help="add the per-sample and per-real membership to the report")
    p.add_argument("--report", type=str, required=True, metavar="OUT.json")
    return p


def _check_common(args) -> tuple:
    ks = check_k(args.k)
    if args.num_real is not None:
        if isinstance(args.num_real, bool) or not isinstance(args.num_real, int) or args.num_real < 2:
            raise ValueError(f"prdc: --num_real must be an integer >= 2, got {args.num_real!r}")
        check_k(ks, num_real=args.num_real)
    if args.ref_chunk is not None and (isinstance(args.ref_chunk, bool) or not isinstance(args.ref_chunk, int)
                                       or args.ref_chunk < 1):
        raise ValueError(f"prdc: --ref_chunk must be an integer >= 1, got {args.ref_chunk!r}")
    return ks


def _check_feature_args(args) -> None:
    """the feature form of check_args; leaves the arrays it had to read in args.feature_sets"""
    if args.features is None or args.ref_features is None:
        raise ValueError("prdc: the feature form needs both --features and --ref_features")
    if (args.labels_json is None) != (args.ref_labels is None):
        raise ValueError("prdc: with features the per-class table needs both --labels_json (samples) and --ref_labels (reals)")
    ks = _check_common(args)
    args.feature_sets = read_feature_sets(args, "prdc", min_rows=2)
    real = args.feature_sets["ref_features"]
    if args.num_real is not None and args.num_real > real.shape[0]:
        raise ValueError(f"prdc: --num_real {args.num_real} exceeds the {real.shape[0]} reals")
    real = real[:args.num_real]
    check_sets(ks, real, {f: x for f, x in args.feature_sets.items() if f != "ref_features"})


def check_args(args) -> None:
    """every choice that needs nothing loaded, checked before an image or the GPU is touched (the feature form also reads
    its arrays: their dtype, shape and finiteness are part of the check)"""
    if feature_form(args, "prdc"):
        return _check_feature_args(args)
    if getattr(args, "ref_labels", None) is not None:
        raise ValueError("prdc: --ref_labels goes with --ref_features; the labels of --dataset are its own")
    if args.image_dir is None:
        raise ValueError("prdc: give the samples with --image_dir")
    if (args.dataset is None) == (args.ref_image_dir is None):
        raise ValueError("prdc: give exactly one source of reals: --dataset cifar10|mnist --data_dir DIR, or --ref_image_dir DIR")
    if args.dataset is not None and args.data_dir is None:
        raise ValueError("prdc: --dataset needs --data_dir")
    if args.dataset is None and args.data_dir is not None:
        raise ValueError("prdc: --data_dir goes with --dataset")
    _check_common(args)
    if args.holdout and args.dataset is None:
        raise ValueError("prdc: --holdout takes the test split of --dataset; use --holdout_image_dir with --ref_image_dir")
    if args.holdout and args.holdout_image_dir is not None:
        raise ValueError("prdc: give one held-out set: --holdout or --holdout_image_dir")
    if args.labels_json is not None and args.dataset is None:
        raise ValueError("prdc: --labels_json needs a labelled set of reals (--dataset): a directory of images has no labels")


def check_sets(ks, real, sets) -> None:
    """the loaded sets against k and against each other, still before the GPU is touched.  sets: {name: uint8 [n, C, H, W]}"""
    for name, x in sets.items():
        if x.shape[1:] != real.shape[1:]:
            raise ValueError(f"prdc: {name} images are {tuple(x.shape[1:])}, the reals {tuple(real.shape[1:])}")
        try:
            check_k(ks, real.shape[0], x.shape[0])
        except ValueError as e:
            raise ValueError(f"{e} (reals and {name})") from None


def _read_sample_labels(path, n, flag="--labels_json"):
    with open(path) as f:
        labels = json.load(f)
    if not isinstance(labels, list) or len(labels) < n or not all(
            isinstance(v, int) and not isinstance(v, bool) and v >= 0 for v in labels):
        raise ValueError(f"prdc: {flag} must hold a list of at least {n} class indices")
    return np.asarray(labels[:n], dtype=np.int64)


def _read_dataset_labels(name, data_dir):
    from .datamodules import read_cifar10, read_mnist
    return np.asarray((read_cifar10 if name == "cifar10" else read_mnist)(data_dir, True)[1], dtype=np.int64)


def format_table(report) -> str:
    """the entries of a report as lines of text: one row per entry and k, then the per-class rows"""
    lines = [f"{'set':10s} {'k':>3s} {'precision':>10s} {'recall':>10s} {'density':>10s} {'coverage':>10s}"]
    for name in ("samples", "holdout"):
        for k, m in report.get(name, {}).items():
            lines.append(f"{name:10s} {k:>3s} " + " ".join(f"{m[r]:10.4f}" for r in RATIOS))
    for k, m in report.get("samples", {}).items():
        for label, c in m.get("per_class", {}).items():
            row = "skipped: " + c["skipped"] if "skipped" in c else " ".join(f"{c[r]:10.4f}" for r in RATIOS)
            lines.append(f"{'class ' + label:10s} {k:>3s} {row}")
    return "\n".join(lines)


def _json_keys(scores) -> dict:
    """{k: metrics} with string keys all the way down, as JSON has them"""
    out = {}
    for k, m in scores.items():
        m = dict(m)
        if "per_class" in m:
            m["per_class"] = {str(c): v for c, v in m["per_class"].items()}
        out[str(k)] = m
    return out


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        check_args(args)
        ks = check_k(args.k)
        feats = getattr(args, "feature_sets", None)
        if feats is not None:
            real = feats["ref_features"]
            real_labels = None if args.ref_labels is None else _read_sample_labels(args.ref_labels, real.shape[0], "--ref_labels")
        else:
            real = _read_dataset(args.dataset, args.data_dir, True) if args.dataset is not None else load_images_u8(args.ref_image_dir)
            real_labels = _read_dataset_labels(args.dataset, args.data_dir) if args.labels_json is not None else None
        if args.num_real is not None:
            if args.num_real > real.shape[0]:
                raise ValueError(f"prdc: --num_real {args.num_real} exceeds the {real.shape[0]} reals")
            real = real[:args.num_real]
            real_labels = None if real_labels is None else real_labels[:args.num_real]
        shape = real.shape[1:]
        if feats is not None:
            sets = {"samples": feats["features"]}
            if "holdout_features" in feats:
                sets["holdout"] = feats["holdout_features"]
        else:
            sets = {"samples": load_images_u8(args.image_dir, shape[1:], shape[0])}
            if args.holdout:
                sets["holdout"] = _read_dataset(args.dataset, args.data_dir, False)
            elif args.holdout_image_dir is not None:
                sets["holdout"] = load_images_u8(args.holdout_image_dir, shape[1:], shape[0])
        check_sets(ks, real, sets)
        fake_labels = None if args.labels_json is None else _read_sample_labels(args.labels_json, sets["samples"].shape[0])
    except ValueError as e:
        parser.error(str(e))
    import torch
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    mm = ManifoldMetrics(real, k=ks, ref_chunk=args.ref_chunk)
    report = {"k": list(ks), "num_real": int(real.shape[0])}
    if feats is not None:
        report.update({"feature_dim": int(shape[0]), "space": FEATURE_SPACE})
    else:
        report.update({"image_shape": [int(v) for v in shape],
                       "space": "pixels (exact integer distances): read the samples against the holdout entry, not against 1"})
    report.update({"num_samples": int(sets["samples"].shape[0]),
                   "samples": _json_keys(mm.score(sets["samples"], real_labels, fake_labels, per_sample=args.per_sample))})
    if "holdout" in sets:
        report["num_holdout"] = int(sets["holdout"].shape[0])
        report["holdout"] = _json_keys(mm.score(sets["holdout"]))
    with open(args.report, "w") as f:
        json.dump(report, f, indent=1)
    print(format_table(report))
    print(f"wrote {args.report}", flush=True)
    return report


if __name__ == "__main__":
    main()
