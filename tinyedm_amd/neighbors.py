"""Nearest training images of generated samples, in pixel space and exact, or nearest rows in a feature space.

The first question about a diffusion model trained on 50 000 images is whether its samples are new or copies.  This module
holds a set of uint8 images against a reference set: for every query the k references with the smallest squared pixel
distance, an exact integer (csrc/neighbors.hip: int8 MFMA, int32 accumulation, ties to the lower index).  The same search
finds duplicates inside a set (`--self`) and, with a held-out set, runs the data-copying test of Meehan et al. 2020
("A Non-Parametric Test to Detect Data-Copying in Generative Models") in pixel space: are the samples closer to the training
set than fresh data is?

    python -m tinyedm.neighbors --image_dir samples --dataset cifar10 --data_dir data --holdout --report nn.json \\
        --grid nn.png --grid_rows 16

The same questions in a feature space: float32 [n, D] features extracted elsewhere (the arrays `tinyedm.frechet --features`
takes) are searched by squared Euclidean distance in fp64 (csrc/neighbors_f32.hip: fp64 MFMA, ties to the lower index,
identical rows at distance 0.0 exactly).  Distances are then floats and --max_d2 is a float.

    python -m tinyedm.neighbors --features A.npy --ref_features B.npy --holdout_features C.npy --k 5 --report nn.json

The statistics (rms, summarize, closer_than_holdout, duplicates) are plain numpy on the host and need no GPU.
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

PERCENTILES = (1, 5, 25, 50, 75, 95)
FEATURE_SPACE = "features as given (float32)"
MAX_K = 32          # ops.KNN_MAX_K, repeated here so that the argument check needs no GPU library


# ---------------------------------------------------------------------------------------------------- host arithmetic
def _d2(x):
    """distances as they arrive: fp64 for the feature form (any float array), int64 for exact pixel distances"""
    a = np.asarray(x)
    return a.astype(np.float64) if a.dtype.kind == "f" else a.astype(np.int64)


def rms(d2, D: int, scale: float = 255.0):
    """squared distance over D elements -> root-mean-square difference per element in units of `scale` (255: pixels in
    [0, 1] units; 1: features as given)"""
    if D < 1:
        raise ValueError(f"rms: D must be >= 1, got {D}")
    return np.sqrt(np.asarray(d2, dtype=np.float64) / float(D)) / scale


def summarize(d2_nearest) -> dict:
    """min, the 1/5/25/50/75/95 percentiles (linear interpolation) and the mean of a list of nearest distances"""
    a = np.asarray(d2_nearest, dtype=np.float64).reshape(-1)
    if a.size == 0:
        raise ValueError("summarize: no distances")
    out = {"n": int(a.size), "min": float(a.min())}
    for p, v in zip(PERCENTILES, np.percentile(a, PERCENTILES)):
        out[f"p{p}"] = float(v)
    out["mean"] = float(a.mean())
    return out


def closer_than_holdout(sample_d2, holdout_d2) -> float:
    """The share of (sample, held-out image) pairs in which the sample is nearer to the training set than the held-out
    image is; a tie counts one half.  Exact, from ranks: 0.5 = samples sit as far from the training data as fresh data
    does, towards 1 = copying (Meehan et al. 2020, in pixel space).  Integer distances are compared as integers, float (feature)
    distances as fp64."""
    s = _d2(sample_d2).reshape(-1)
    h = np.sort(_d2(holdout_d2).reshape(-1))
    if s.dtype != h.dtype:
        raise ValueError("closer_than_holdout: one list holds pixel distances (integers), the other feature distances (floats)")
    if s.size == 0 or h.size == 0:
        raise ValueError("closer_than_holdout: both lists must be non-empty")
    lo = np.searchsorted(h, s, side="left")
    hi = np.searchsorted(h, s, side="right")
    greater = int((h.size - hi).sum())        # held-out images strictly farther than the sample
    equal = int((hi - lo).sum())
    return (2 * greater + equal) / (2 * int(s.size) * int(h.size))


def duplicates(dist, idx, max_d2) -> list:
    """the pairs (query i, reference j, d2) with d2 <= max_d2, in order of i and then of rank; d2 an int for integer (pixel)
    distances and a float for float (feature) distances"""
    d = _d2(dist)
    j = np.asarray(idx, dtype=np.int64)
    num = float if d.dtype.kind == "f" else int
    if d.shape != j.shape or d.ndim != 2:
        raise ValueError(f"duplicates: dist {d.shape} and idx {j.shape} must be equal [Q, k] arrays")
    if max_d2 < 0:
        raise ValueError(f"duplicates: max_d2 must be >= 0, got {max_d2}")
    qi, ri = np.nonzero(d <= max_d2)
    return [(int(a), int(j[a, b]), num(d[a, b])) for a, b in zip(qi, ri)]


# ---------------------------------------------------------------------------------------------------- images
def read_png_dir(image_dir, who, where, image_size=None, channels=None) -> list:
    """the <index>.png files of a directory (as generate writes them) as uint8 [H, W, C] arrays in numeric index order.
    who / where: the caller's name and its name for the directory, for the messages.  image_size: an int for square
    images or (H, W); image_size / channels None: taken from the first image.  Every image must agree."""
    from PIL import Image
    names = [f for f in os.listdir(image_dir) if f.lower().endswith(".png")]
    bad = [f for f in names if not os.path.splitext(f)[0].isdigit()]
    if bad:
        raise ValueError(f"{who}: {where} holds PNGs that are not named <index>.png: {sorted(bad)[:3]}")
    if not names:
        raise ValueError(f"{who}: no PNG in {image_dir}")
    out, want = [], None
    for f in sorted(names, key=lambda f: int(os.path.splitext(f)[0])):
        a = np.asarray(Image.open(os.path.join(image_dir, f)))
        a = a[:, :, None] if a.ndim == 2 else a
        if want is None:
            hw = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size or a.shape[:2])
            want = (int(hw[0]), int(hw[1]), channels or a.shape[2])
        if a.dtype != np.uint8 or a.shape != want:
            raise ValueError(f"{who}: {f} is {a.dtype} {a.shape}, expected uint8 {want}")
        out.append(a)
    return out


def load_images_u8(image_dir, image_size=None, channels=None) -> np.ndarray:
    """read_png_dir as raw uint8 [n, C, H, W]"""
    return np.stack([np.ascontiguousarray(a.transpose(2, 0, 1))
                     for a in read_png_dir(image_dir, "neighbors", image_dir, image_size, channels)])


# ---------------------------------------------------------------------------------------------------- the search
def as_set(x, who):
    """a set as it is taken in: uint8 [n, ...] images or finite float32 [n, D] features (numpy or torch) -> a torch tensor"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.float32) or t.dim() < 2 or (
            t.dtype == torch.float32 and t.dim() != 2):
        what = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(x).__name__
        raise ValueError(f"{who}: a set is uint8 [n, ...] images or float32 [n, D] features, got {what} (convert features "
                         "with .float())")
    if t.dtype == torch.float32 and not bool(torch.isfinite(t).all()):
        raise ValueError(f"{who}: non-finite features")
    return t


class NearestNeighbors:
    """k nearest reference rows of a set of queries.  refs_u8: uint8 [R, ...] images, searched by exact integer pixel
    distance, or float32 [R, D] features, searched by fp64 Euclidean distance (numpy or torch; moved to `device`).
    References beyond ref_chunk rows are searched chunk by chunk; the per-chunk key lists are merged on the device by the
    same (d2, index) key, so the result is bit-identical to the unchunked call."""

    def __init__(self, refs_u8, k: int = 5, ref_chunk=None, device=None):
        import torch
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
            raise ValueError(f"NearestNeighbors: k must be an integer in [1, {MAX_K}], got {k!r}")
        if ref_chunk is not None and (isinstance(ref_chunk, bool) or not isinstance(ref_chunk, int) or ref_chunk < 1):
            raise ValueError(f"NearestNeighbors: ref_chunk must be None or an integer >= 1, got {ref_chunk!r}")
        refs = as_set(refs_u8, "NearestNeighbors")
        if device is None:
            device = refs.device if refs.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.refs = refs.to(device).contiguous()
        self.k, self.ref_chunk = k, ref_chunk
        self.features = self.refs.dtype == torch.float32

    def search(self, queries_u8, exclude_self: bool = False, k=None):
        """-> (dist [Q, k], idx int64 [Q, k]) on the device, ascending by (dist, idx); dist int64 for images, fp64 for
        features; k: fewer than the object's.  The queries must be of the references' kind."""
        from . import ops
        q = queries_u8 if queries_u8 is self.refs else as_set(queries_u8, "NearestNeighbors.search")
        if q.dtype != self.refs.dtype:
            raise ValueError(f"NearestNeighbors.search: the queries are {q.dtype}, the references {self.refs.dtype}: both "
                             "sets must be uint8 images or both float32 features")
        knn = ops.f32_knn if self.features else ops.u8_knn
        return knn(q.to(self.refs.device).contiguous(), self.refs, self.k if k is None else k, exclude_self,
                   ref_chunk=self.ref_chunk)


# ---------------------------------------------------------------------------------------------------- command line
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Exact pixel-space nearest training images of generated samples")
    p.add_argument("--image_dir", type=str, default=None, help="directory of <index>.png samples (as generate writes them)")
    p.add_argument("--dataset", choices=["cifar10", "mnist"], default=None, help="reference: built-in train split")
    p.add_argument("--data_dir", type=str, default=None)
    p.add_argument("--ref_image_dir", type=str, default=None, help="reference: a directory of <index>.png images")
    p.add_argument("--holdout", action="store_true", help="with --dataset: compare with the test split's distances")
    p.add_argument("--holdout_image_dir", type=str, default=None, help="held-out images as a directory of <index>.png")
    p.add_argument("--k", type=int, default=5)
    p.add_argument("--features", type=str, default=None, metavar="A.npy", help="samples as a float32 [n, D] array")
    p.add_argument("--ref_features", type=str, default=None, metavar="B.npy", help="references as a float32 [n, D] array")
    p.add_argument("--holdout_features", type=str, default=None, metavar="C.npy",
                   help="held-out rows as a float32 [n, D] array")
    p.add_argument("--max_d2", type=_int_or_float, default=None,
                   help="list samples whose nearest neighbour is at or under this d2 (an integer for images, a float for "
                        "features)")
    p.add_argument("--self", dest="self_search", action="store_true",
                   help="search the reference set against itself and list the pairs at or under --max_d2 (default 0) among each "
                        "image's --k nearest: an image with more than --k such partners shows only its --k closest")
    p.add_argument("--report", type=str, required=True, metavar="OUT.json")
    p.add_argument("--grid", type=str, default=None, metavar="OUT.png")
    p.add_argument("--grid_rows", type=int, default=16)
    return p


def _int_or_float(text):
    try:
        return int(text)
    except ValueError:
        return float(text)


FEATURE_FLAGS = ("features", "ref_features", "holdout_features")
IMAGE_FLAGS = ("image_dir", "dataset", "data_dir", "ref_image_dir", "holdout", "holdout_image_dir")


def feature_form(args, who) -> bool:
    """whether the feature flags are in use; refuses a mix with the image flags"""
    feat = [f for f in FEATURE_FLAGS if getattr(args, f, None) is not None]
    img = [f for f in IMAGE_FLAGS if getattr(args, f, None) not in (None, False)]
    if feat and img:
        raise ValueError(f"{who}: give images or features, not both: --{' --'.join(feat)} do not go with "
                         f"--{' --'.join(img)}")
    return bool(feat)


def read_features(path, flag, who, min_rows=1) -> np.ndarray:
    """a .npy file as a finite float32 [n >= min_rows, D >= 1] array"""
    a = np.load(path, allow_pickle=False)
    if a.dtype != np.float32 or a.ndim != 2 or a.shape[0] < min_rows or a.shape[1] < 1:
        raise ValueError(f"{who}: {flag} must hold a float32 [n >= {min_rows}, D] array, got {a.dtype} {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{who}: {flag} holds non-finite features")
    return np.ascontiguousarray(a)


def read_feature_sets(args, who, min_rows=1) -> dict:
    """the arrays of the feature flags that are set, {flag: float32 [n, D]}, all of one D"""
    sets = {f: read_features(getattr(args, f), "--" + f, who, min_rows) for f in FEATURE_FLAGS
            if getattr(args, f, None) is not None}
    dims = {f: a.shape[1] for f, a in sets.items()}
    if len(set(dims.values())) > 1:
        raise ValueError(f"{who}: the feature arrays differ in D: " + ", ".join(f"--{f} {d}" for f, d in dims.items()))
    return sets


def _check_feature_args(args) -> None:
    """the feature form of check_args; leaves the arrays it had to read in args.feature_sets"""
    if isinstance(args.k, bool) or not isinstance(args.k, int) or not 1 <= args.k <= MAX_K:
        raise ValueError(f"neighbors: --k must be in [1, {MAX_K}], got {args.k!r}")
    if args.max_d2 is not None and not (np.isfinite(args.max_d2) and args.max_d2 >= 0):
        raise ValueError(f"neighbors: --max_d2 must be finite and >= 0, got {args.max_d2}")
    if args.grid is not None:
        raise ValueError("neighbors: --grid draws images; there are none with --features / --ref_features")
    if args.self_search:
        if (args.features is None) == (args.ref_features is None):
            raise ValueError("neighbors: --self searches one set against itself: give --features or --ref_features, not both")
        if args.holdout_features is not None:
            raise ValueError("neighbors: --self goes without --holdout_features")
    elif args.features is None or args.ref_features is None:
        raise ValueError("neighbors: the feature form needs both --features and --ref_features (or --self with one of them)")
    args.feature_sets = read_feature_sets(args, "neighbors")
    refs = args.feature_sets["ref_features" if args.ref_features is not None else "features"]
    if args.k > refs.shape[0] - (1 if args.self_search else 0):
        raise ValueError(f"neighbors: --k {args.k} needs at least that many reference rows"
                         f"{' besides the row itself' if args.self_search else ''}, got {refs.shape[0]}")


def check_args(args) -> None:
    """every choice that needs nothing loaded, checked before an image or the GPU is touched (the feature form also reads
    its arrays: their dtype, shape and finiteness are part of the check)"""
    if feature_form(args, "neighbors"):
        return _check_feature_args(args)
    if isinstance(args.max_d2, float):
        raise ValueError(f"neighbors: --max_d2 is an integer for images (exact pixel distances), got {args.max_d2}")
    if (args.dataset is None) == (args.ref_image_dir is None):
        raise ValueError("neighbors: give exactly one reference source: --dataset cifar10|mnist --data_dir DIR, or "
                         "--ref_image_dir DIR")
    if args.dataset is not None and args.data_dir is None:
        raise ValueError("neighbors: --dataset needs --data_dir")
    if args.dataset is None and args.data_dir is not None:
        raise ValueError("neighbors: --data_dir goes with --dataset")
    if isinstance(args.k, bool) or not isinstance(args.k, int) or not 1 <= args.k <= MAX_K:
        raise ValueError(f"neighbors: --k must be in [1, {MAX_K}], got {args.k!r}")
    if args.max_d2 is not None and args.max_d2 < 0:
        raise ValueError(f"neighbors: --max_d2 must be >= 0, got {args.max_d2}")
    if args.holdout and args.dataset is None:
        raise ValueError("neighbors: --holdout takes the test split of --dataset; use --holdout_image_dir with --ref_image_dir")
    if args.holdout and args.holdout_image_dir is not None:
        raise ValueError("neighbors: give one held-out set: --holdout or --holdout_image_dir")
    if args.self_search:
        if args.image_dir is not None:
            raise ValueError("neighbors: --self searches the reference set against itself and takes no --image_dir")
        if args.holdout or args.holdout_image_dir is not None or args.grid is not None:
            raise ValueError("neighbors: --self goes without --holdout, --holdout_image_dir and --grid")
    elif args.image_dir is None:
        raise ValueError("neighbors: give the samples with --image_dir (or --self for duplicates inside the reference set)")
    if args.grid is not None and args.grid_rows < 1:
        raise ValueError(f"neighbors: --grid_rows must be >= 1, got {args.grid_rows}")


def _read_dataset(name, data_dir, train):
    from .datamodules import read_cifar10, read_mnist
    x, _ = (read_cifar10 if name == "cifar10" else read_mnist)(data_dir, train)
    x = np.asarray(x)
    return np.ascontiguousarray(x[:, None] if x.ndim == 3 else x)


def neighbour_rows(dist, idx, D: int) -> list:
    """per query its neighbours as [{"index", "d2", "rms"}, ...]; float (feature) distances stay floats, rms in their units"""
    d, j = _d2(dist), np.asarray(idx, dtype=np.int64)
    feat = d.dtype.kind == "f"
    num = float if feat else int
    r = rms(d, D, 1.0 if feat else 255.0)
    return [[{"index": int(j[a, b]), "d2": num(d[a, b]), "rms": float(r[a, b])} for b in range(d.shape[1])]
            for a in range(d.shape[0])]


def write_grid(path, samples, refs, dist, idx, rows: int) -> tuple:
    """one row per sample for the `rows` samples with the smallest nearest distance (ties: lower index): the sample, then
    its neighbours in order.  samples / refs uint8 [n, C, H, W] on the host.  Returns the (width, height) written."""
    from PIL import Image
    d, j = np.asarray(dist, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    order = np.lexsort((np.arange(d.shape[0]), d[:, 0]))[:rows]
    C, H, W = samples.shape[1:]
    k = d.shape[1]
    canvas = np.zeros((len(order) * H, (k + 1) * W, C), dtype=np.uint8)
    for r, a in enumerate(order):
        canvas[r * H:(r + 1) * H, :W] = samples[a].transpose(1, 2, 0)
        for b in range(k):
            canvas[r * H:(r + 1) * H, (b + 1) * W:(b + 2) * W] = refs[j[a, b]].transpose(1, 2, 0)
    Image.fromarray(canvas[:, :, 0] if C == 1 else canvas).save(path)
    return canvas.shape[1], canvas.shape[0]


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        check_args(args)
    except ValueError as e:
        parser.error(str(e))
    import torch
    feats = getattr(args, "feature_sets", None)
    scale = 255.0 if feats is None else 1.0        # rms in [0, 1] pixel units, or in the features' own units
    if feats is not None:
        refs = feats["ref_features" if args.ref_features is not None else "features"]
    else:
        refs = _read_dataset(args.dataset, args.data_dir, True) if args.dataset is not None else load_images_u8(args.ref_image_dir)
    shape = refs.shape[1:]
    D = int(np.prod(shape))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    nn = NearestNeighbors(refs, k=args.k)
    report = {"k": args.k, "num_references": int(refs.shape[0])}
    report.update({"image_shape": [int(v) for v in shape]} if feats is None else {"feature_dim": D, "space": FEATURE_SPACE})
    if args.self_search:
        dist, idx = (t.cpu().numpy() for t in nn.search(nn.refs, exclude_self=True))
        max_d2 = 0 if args.max_d2 is None else args.max_d2
        pairs = sorted({(min(i, j), max(i, j), d) for i, j, d in duplicates(dist, idx, max_d2)})
        report.update({"max_d2": max_d2, "nearest": summarize(dist[:, 0]),
                       "pairs_searched": f"the {args.k} nearest images of each image: raise --k if an image reaches it",
                       "images_with_k_pairs": [int(i) for i in np.nonzero(dist[:, -1] <= max_d2)[0]],
                       "duplicate_pairs": [{"i": i, "j": j, "d2": d, "rms": float(rms(d, D, scale))} for i, j, d in pairs]})
    else:
        samples = feats["features"] if feats is not None else load_images_u8(args.image_dir, shape[1:], shape[0])
        dist, idx = (t.cpu().numpy() for t in nn.search(samples))
        report.update({"num_samples": int(samples.shape[0]), "neighbours": neighbour_rows(dist, idx, D),
                       "nearest": summarize(dist[:, 0])})
        hold = None if feats is None else feats.get("holdout_features")
        if args.holdout:
            hold = _read_dataset(args.dataset, args.data_dir, False)
        elif args.holdout_image_dir is not None:
            hold = load_images_u8(args.holdout_image_dir, shape[1:], shape[0])
        if hold is not None:
            hd = nn.search(hold, k=1)[0][:, 0].cpu().numpy()
            report.update({"num_holdout": int(hold.shape[0]), "holdout_nearest": summarize(hd),
                           "closer_than_holdout": closer_than_holdout(dist[:, 0], hd)})
        if args.max_d2 is not None:
            report.update({"max_d2": args.max_d2,
                           "at_or_under_max_d2": [{"sample": i, "index": j, "d2": d, "rms": float(rms(d, D, scale))}
                                                  for i, j, d in duplicates(dist[:, :1], idx[:, :1], args.max_d2)]})
        if args.grid is not None:
            report["grid"] = {"path": args.grid, "size": list(write_grid(args.grid, samples, refs, dist, idx, args.grid_rows))}
    with open(args.report, "w") as f:
        json.dump(report, f, indent=1)
    near = report["nearest"]
    fmt = ".0f" if feats is None else ".6g"
    print(f"nearest d2: min {near['min']:{fmt}}  median {near['p50']:{fmt}}  mean {near['mean']:{'.1f' if feats is None else fmt}}"
          f"  (rms of the median {float(rms(near['p50'], D, scale)):.4f})")
    if "closer_than_holdout" in report:
        print(f"closer_than_holdout {report['closer_than_holdout']:.4f}  (0.5: as far from the training set as fresh data)")
    print(f"wrote {args.report}", flush=True)
    return report


if __name__ == "__main__":
    main()
