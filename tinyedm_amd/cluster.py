"""k-means on features: clusters as pseudo-labels and the mode coverage of a sample set.

    python -m tinyedm.cluster --fit --features train.npy --k 100 --n_init 4 --out clusters.npz --labels_out train_labels.json
    python -m tinyedm.cluster --clusters clusters.npz --features samples.npy --ref_features train.npy \
        --holdout_features test.npy --labels_out drawn.json --report modes.json

The label files are plain JSON lists in row order: what `tinyedm.prdc` and `tinyedm.frechet` read as --labels_json and
--ref_labels (their per-class tables become per-cluster tables with no change), and what the datamodules read as
labels_path (self-guided training, Hu et al. 2023).

A Lloyd iteration has two halves.  Assignment is nearest-centroid search, ops.f32_knn with k = 1 (fp64 distances on the
matrix pipe, ties to the lower cluster).  The update is ops.f32_cluster_sums (csrc/kmeans.hip): per-cluster fp64 sums of
the gathered rows in an order that depends on the cluster's member list alone, so a fit gives the same bits every time.
Everything between the two is integer bookkeeping; the empty-cluster rule and the k-means++ draws run on the host.
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

INITS = ("k-means++",)


# ---------------------------------------------------------------------------------------------------- host-side rules
def fill_empty_clusters(labels, d2, K):
    """The empty-cluster rule, on host arrays (labels int64 [n], d2 fp64 [n]; both are changed in place) -> the clusters
    that stay empty.  Empty clusters are taken in ascending index.  Each takes the row with the largest d2, ties to the
    lower row, among the rows that were not moved before, whose cluster would keep another member, and whose d2 is > 0 (a
    row at distance 0 would only duplicate the centroid it sits on).  That row's label becomes the empty cluster and its d2
    becomes 0.  If no row qualifies the cluster stays empty."""
    counts = np.bincount(labels, minlength=K)
    empty = np.flatnonzero(counts == 0)
    if empty.size == 0:
        return []
    order = np.lexsort((np.arange(labels.shape[0]), -d2))      # largest d2 first, ties to the lower row
    moved = np.zeros(labels.shape[0], bool)
    left = []
    for e in empty.tolist():
        r = None
        for cand in order:
            if moved[cand]:
                continue
            if not d2[cand] > 0.0:                              # every later unmoved row is at 0 too
                break
            if counts[labels[cand]] > 1:
                r = int(cand)
                break
        if r is None:
            left.append(e)
            continue
        counts[labels[r]] -= 1
        counts[e] += 1
        labels[r], d2[r], moved[r] = e, 0.0, True
    return left


def draw_d2(weights, u):
    """The D^2 draw: the first index whose fp64 prefix sum (numpy cumsum: one row after the other) exceeds u * total; None
    when the total is 0.  A row of weight 0 is never drawn."""
    cs = np.cumsum(np.asarray(weights, dtype=np.float64))
    total = float(cs[-1])
    if not total > 0.0:
        return None
    i = int(np.searchsorted(cs, u * total, side="right"))
    if i >= cs.shape[0]:                                        # u * total rounded up to the total: the last row of weight > 0
        i = int(np.flatnonzero(np.asarray(weights) > 0)[-1])
    return i


def host_sum(values) -> float:
    """fp64 values added one at a time in ascending index (the inertia of a fit from its cluster inertias)"""
    s = 0.0
    for v in np.asarray(values, dtype=np.float64).tolist():
        s += v
    return s


# ---------------------------------------------------------------------------------------------------- the iteration
def _set(x, name, who):
    import torch
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.numel() == 0:
        what = f"{x.dtype} {tuple(x.shape)}" if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"{who}: {name} must be a non-empty float32 [n, D] tensor, got {what}")
    if not x.is_cuda:
        raise ValueError(f"{who}: {name}: expected a CUDA/HIP tensor -- tinyedm_amd has no CPU path")
    return x.contiguous()


def assign(x, centroids):
    """(labels int64 [n], d2 fp64 [n]): the nearest centroid of every row by ops.f32_knn, ties to the lower cluster"""
    from . import ops
    dist, idx = ops.f32_knn(x, centroids, 1)
    return idx[:, 0].contiguous(), dist[:, 0].contiguous()


def lloyd_step(x, centroids):
    """One Lloyd iteration on x float32 [n, D] from centroids float32 [K, D] -> (labels int64 [n], d2 fp64 [n],
    new_centroids float32 [K, D], counts int64 [K], cluster_inertia fp64 [K]).  labels and d2 are those of
    ops.f32_knn(x, centroids, 1) after the empty-cluster rule (fill_empty_clusters); new_centroids = sums / counts in fp64
    rounded to float32 once, with the sums of ops.f32_cluster_sums; a cluster that stays empty keeps its centroid with
    count 0; cluster_inertia[k] = the sum of d2 over the members in the same order.  The step waits for the device once, for
    the K cluster counts: they show whether the host rule has work to do (only then labels and d2 travel to the host and
    back) and they are what the chunk tables of f32_cluster_sums are made from."""
    import torch
    from . import ops
    x, centroids = _set(x, "x", "lloyd_step"), _set(centroids, "centroids", "lloyd_step")
    if centroids.shape[1] != x.shape[1] or centroids.device != x.device:
        raise ValueError(f"lloyd_step: expected [K, {x.shape[1]}] centroids on {x.device}, got {tuple(centroids.shape)} on "
                         f"{centroids.device}")
    K = centroids.shape[0]
    labels, d2 = assign(x, centroids)
    counts = torch.bincount(labels, minlength=K).cpu().numpy()      # the one wait of a step
    if not counts.all():
        lab, dd = labels.cpu().numpy(), d2.cpu().numpy()
        fill_empty_clusters(lab, dd, K)
        labels, d2 = torch.from_numpy(lab).to(x.device), torch.from_numpy(dd).to(x.device)
        counts = np.bincount(lab, minlength=K)
    sums, counts, inertia = ops.f32_cluster_sums(x, labels, K, d2, counts=counts)
    mean = sums / counts.clamp(min=1).double().unsqueeze(1)
    return labels, d2, torch.where((counts > 0).unsqueeze(1), mean.float(), centroids), counts, inertia


def kmeans_plus_plus(x, K, seed):
    """D^2 seeding (Arthur & Vassilvitskii 2007) -> int64 [K] row indices (a numpy array).  The draws come from
    numpy.random.default_rng(seed): the first row is rng.integers(n); every further row is draw_d2(min d2 to the chosen
    rows, rng.random()), the minimum kept on the device and updated with one ops.f32_knn against the new row (identical
    rows are at +0.0 exactly, so a duplicate of a chosen row is never drawn); when every remaining row is a duplicate the
    lowest unchosen row index is taken."""
    import torch
    from . import ops
    x = _set(x, "x", "kmeans_plus_plus")
    n = x.shape[0]
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= n:
        raise ValueError(f"kmeans_plus_plus: K must be an integer in [1, n = {n}], got {K!r}")
    rng = np.random.default_rng(seed)
    chosen = [int(rng.integers(n))]
    taken = np.zeros(n, bool)
    taken[chosen[0]] = True
    mind2 = ops.f32_knn(x, x[chosen[0]:chosen[0] + 1], 1)[0][:, 0]
    for _ in range(1, K):
        w = mind2.cpu().numpy()
        w[taken] = 0.0
        i = draw_d2(w, rng.random())
        if i is None:
            i = int(np.flatnonzero(~taken)[0])
        chosen.append(i)
        taken[i] = True
        mind2 = torch.minimum(mind2, ops.f32_knn(x, x[i:i + 1], 1)[0][:, 0])
    return np.asarray(chosen, dtype=np.int64)


class KMeans:
    """Lloyd's k-means on float32 features with k-means++ seeding; deterministic (same arguments, same bits).

    fit(x) checks once that x (float32 [n, D] on the GPU) is finite, scales the rows to unit length when `normalize` is
    set, runs n_init seedings (seed, seed + 1, ...) and keeps the run of least inertia (ties to the earlier run).  A run
    iterates lloyd_step until no label changes (`converged`), the relative decrease of the inertia is <= tol, or max_iter
    steps were taken (per step fit waits for the device three times: the counts inside lloyd_step, the cluster inertias,
    the label comparison).  init: "k-means++" or a float32 [K, D] tensor (then n_init must be 1); with `normalize` its
    rows are scaled to unit length like those of x.

    After fit: centroids float32 [K, D], labels_ int64 [n] (= predict(x)[0]), counts int64 [K], cluster_inertia fp64 [K],
    inertia (the cluster inertias added in ascending cluster order on the host), inertia_history (one entry per step),
    n_iter, converged, empty_clusters (clusters without a member: fewer distinct usable rows than clusters)."""

    def __init__(self, n_clusters, *, n_init=1, max_iter=100, tol=0.0, seed=0, normalize=False, init="k-means++"):
        import torch
        for name, v in (("n_clusters", n_clusters), ("n_init", n_init), ("max_iter", max_iter)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"KMeans: {name} must be an integer >= 1, got {v!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or seed < 0:
            raise ValueError(f"KMeans: seed must be an integer >= 0, got {seed!r}")
        if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not 0.0 <= float(tol) < 1.0:
            raise ValueError(f"KMeans: tol must be in [0, 1), got {tol!r}")
        if isinstance(init, torch.Tensor):
            if init.dtype != torch.float32 or init.dim() != 2 or init.shape[0] != n_clusters:
                raise ValueError(f"KMeans: an init tensor must be float32 [{n_clusters}, D], got {init.dtype} "
                                 f"{tuple(init.shape)}")
            if n_init != 1:
                raise ValueError("KMeans: a given init leaves nothing to draw: n_init must be 1")
        elif init not in INITS:
            raise ValueError(f"KMeans: init must be 'k-means++' or a float32 [K, D] tensor, got {init!r}")
        self.n_clusters, self.n_init, self.max_iter, self.tol = n_clusters, n_init, max_iter, float(tol)
        self.seed, self.normalize, self.init = seed, bool(normalize), init
        self.centroids = None

    def _prepare(self, x, who):
        from .features import _unit_rows
        x = _set(x, "x", who)
        return _unit_rows(x) if self.normalize else x

    def _run(self, x, c):
        import torch
        prev_labels, prev, hist, converged = None, None, [], False
        for it in range(1, self.max_iter + 1):
            labels, d2, new_c, counts, cin = lloyd_step(x, c)
            inertia = host_sum(cin.cpu().numpy())
            hist.append(inertia)
            if prev_labels is not None and bool(torch.equal(labels, prev_labels)):
                converged = True                                # the same members: new_c has the bits of c
                break
            small = prev is not None and prev - inertia <= self.tol * prev
            prev_labels, prev, c = labels, inertia, new_c
            if small:
                break
        if not converged:                                       # the attributes describe the centroids that are kept
            labels, d2 = assign(x, c)
            from . import ops
            _, counts, cin = ops.f32_cluster_sums(x, labels, c.shape[0], d2)
            inertia = host_sum(cin.cpu().numpy())
        return {"centroids": c, "labels_": labels, "counts": counts, "cluster_inertia": cin, "inertia": inertia,
                "inertia_history": hist, "n_iter": it, "converged": converged,
                "empty_clusters": np.flatnonzero(counts.cpu().numpy() == 0).tolist()}

    def fit(self, x):
        import torch
        x = _set(x, "x", "KMeans.fit")
        if not bool(torch.isfinite(x).all()):
            raise ValueError("KMeans.fit: x holds non-finite features")
        if x.shape[0] < self.n_clusters:
            raise ValueError(f"KMeans.fit: {self.n_clusters} clusters need at least that many rows, got {x.shape[0]}")
        x = self._prepare(x, "KMeans.fit")
        best = None
        for run in range(self.n_init):
            if isinstance(self.init, torch.Tensor):
                c = _set(self.init.to(x.device), "init", "KMeans.fit")
                if c.shape[1] != x.shape[1] or not bool(torch.isfinite(c).all()):
                    raise ValueError(f"KMeans.fit: init must be finite [K, {x.shape[1]}], got {tuple(c.shape)}")
                c = self._prepare(c, "KMeans.fit")
            else:
                rows = kmeans_plus_plus(x, self.n_clusters, self.seed + run)
                c = x[torch.from_numpy(rows).to(x.device)].contiguous()
            out = self._run(x, c)
            if best is None or out["inertia"] < best["inertia"]:
                best = out
        for k, v in best.items():
            setattr(self, k, v)
        return self

    def predict(self, x):
        """(labels int64 [n], d2 fp64 [n]) of x against the fitted centroids (rows normalised as in fit)"""
        if self.centroids is None:
            raise ValueError("KMeans.predict: fit or load first")
        x = self._prepare(x, "KMeans.predict")
        if x.shape[1] != self.centroids.shape[1] or x.device != self.centroids.device:
            raise ValueError(f"KMeans.predict: expected [n, {self.centroids.shape[1]}] features on {self.centroids.device}, "
                             f"got {tuple(x.shape)} on {x.device}")
        return assign(x, self.centroids)

    def save(self, path) -> None:
        """an .npz of centroids, counts, cluster inertia, normalize and the arguments"""
        if self.centroids is None:
            raise ValueError("KMeans.save: fit first")
        args = {"n_clusters": self.n_clusters, "n_init": self.n_init, "max_iter": self.max_iter, "tol": self.tol,
                "seed": self.seed, "init": self.init if isinstance(self.init, str) else "given", "n_iter": int(self.n_iter),
                "converged": bool(self.converged), "inertia": float(self.inertia)}
        with open(path, "wb") as f:
            np.savez(f, centroids=self.centroids.cpu().numpy(), counts=self.counts.cpu().numpy(),
                     cluster_inertia=self.cluster_inertia.cpu().numpy(), normalize=np.asarray(self.normalize),
                     arguments=np.asarray(json.dumps(args)))

    @classmethod
    def load(cls, path, device="cuda") -> "KMeans":
        """The clusters of a saved fit, ready for predict: centroids, counts, cluster_inertia, inertia, n_iter, converged,
        empty_clusters, normalize and the scalar arguments.  What the file does not hold is not restored: labels_ and
        inertia_history stay unset, and a tensor init is not kept (init reads "k-means++")."""
        import torch
        a = read_clusters(path)
        args = a["arguments"]
        km = cls(args["n_clusters"], n_init=args["n_init"], max_iter=args["max_iter"], tol=args["tol"], seed=args["seed"],
                 normalize=a["normalize"])
        km.centroids = torch.from_numpy(a["centroids"]).to(device)
        km.counts = torch.from_numpy(a["counts"]).to(device)
        km.cluster_inertia = torch.from_numpy(a["cluster_inertia"]).to(device)
        km.inertia, km.n_iter, km.converged = args["inertia"], args["n_iter"], args["converged"]
        km.empty_clusters = np.flatnonzero(a["counts"] == 0).tolist()
        return km


def read_clusters(path) -> dict:
    """the arrays of KMeans.save, checked, on the host: centroids float32 [K, D], counts int64 [K], cluster_inertia fp64 [K],
    normalize bool, arguments dict"""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ("centroids", "counts", "cluster_inertia", "normalize", "arguments") if k not in z.files]
        if missing:
            raise ValueError(f"cluster: {path} is not a file of KMeans.save (no {', '.join(missing)})")
        c, counts, cin = z["centroids"], z["counts"], z["cluster_inertia"]
        normalize, args = bool(z["normalize"]), json.loads(str(z["arguments"]))
    if c.dtype != np.float32 or c.ndim != 2 or c.size == 0 or not np.isfinite(c).all():
        raise ValueError(f"cluster: {path}: centroids must be a finite float32 [K, D] array, got {c.dtype} {c.shape}")
    K = c.shape[0]
    if counts.dtype != np.int64 or counts.shape != (K,) or cin.dtype != np.float64 or cin.shape != (K,) or (counts < 0).any():
        raise ValueError(f"cluster: {path}: counts and cluster_inertia must be int64 and float64 [{K}]")
    return {"centroids": np.ascontiguousarray(c), "counts": counts, "cluster_inertia": cin, "normalize": normalize,
            "arguments": args}


# ---------------------------------------------------------------------------------------------------- mode coverage
def _counts(v, name, K=None):
    a = np.asarray(v)
    if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iu" or (a < 0).any() or (K is not None and a.size != K):
        raise ValueError(f"mode_report: {name} must be {'a' if K is None else str(K)} non-negative integer count(s) per "
                         f"cluster, got {a.dtype} {a.shape}")
    if int(a.sum()) == 0:
        raise ValueError(f"mode_report: {name} counts nothing")
    return a.astype(np.int64)


def _xlogy(p, q):
    """sum p log(p / q) in nats with 0 log 0 = 0"""
    m = p > 0
    return float(np.sum(p[m] * np.log(p[m] / q[m])))


def _mode_block(ref, p, counts):
    n = int(counts.sum())
    q = counts / n
    occ = ref > 0
    missing = np.flatnonzero(occ & (counts == 0))
    mid = 0.5 * (p + q)
    expect = n * p[occ]
    return {"n": n,
            "share": q.tolist(),
            "ratio": [float(q[k] / p[k]) if occ[k] else None for k in range(len(p))],
            "missing": missing.tolist(),
            "coverage": 1.0 - len(missing) / int(occ.sum()),
            "total_variation": float(0.5 * np.abs(p - q).sum()),
            "js_divergence": 0.5 * _xlogy(p, mid) + 0.5 * _xlogy(q, mid),
            "chi2": float(((counts[occ] - expect) ** 2 / expect).sum()),
            "outside_reference": int(counts[~occ].sum())}


def mode_report(ref_counts, sample_counts, holdout_counts=None) -> dict:
    """The histogram of a sample set over the clusters of a reference set, against the references' own histogram.  All
    arguments are integer counts per cluster.  With p the reference shares and q the sample shares, the block `samples`
    holds: share (q) and ratio (q / p; None where the references have none) per cluster; missing, the clusters the
    references occupy and no sample hits; coverage = 1 - missing / occupied; total_variation = 1/2 sum |p - q|;
    js_divergence in nats with 0 log 0 = 0; chi2, Pearson's sum (count - n p)^2 / (n p) over the occupied clusters; and
    outside_reference, the samples in clusters the references leave empty (they enter total_variation and js_divergence,
    not chi2).  holdout_counts adds the same block for a held-out split of real data: a finite real sample is not at 0
    either, so read the samples against that entry."""
    ref = _counts(ref_counts, "ref_counts")
    K = ref.shape[0]
    p = ref / int(ref.sum())
    out = {"clusters": K, "occupied": int((ref > 0).sum()), "n_ref": int(ref.sum()), "reference_share": p.tolist(),
           "samples": _mode_block(ref, p, _counts(sample_counts, "sample_counts", K))}
    if holdout_counts is not None:
        out["holdout"] = _mode_block(ref, p, _counts(holdout_counts, "holdout_counts", K))
    return out


def format_table(report) -> str:
    """a mode report as lines of text: the summary rows, then one row per cluster"""
    sets = [s for s in ("samples", "holdout") if s in report]
    lines = [f"{'set':10s} {'n':>8s} {'coverage':>9s} {'missing':>8s} {'TV':>8s} {'JS':>9s} {'chi2':>11s}"]
    for s in sets:
        b = report[s]
        lines.append(f"{s:10s} {b['n']:8d} {b['coverage']:9.4f} {len(b['missing']):8d} {b['total_variation']:8.4f} "
                     f"{b['js_divergence']:9.5f} {b['chi2']:11.2f}")
    lines.append(f"{'cluster':>7s} {'reference':>10s} " + " ".join(f"{s:>10s} {'ratio':>7s}" for s in sets))
    for k, p in enumerate(report["reference_share"]):
        cells = []
        for s in sets:
            r = report[s]["ratio"][k]
            cells.append(f"{report[s]['share'][k]:10.5f} {'-' if r is None else format(r, '7.3f'):>7s}")
        lines.append(f"{k:7d} {p:10.5f} " + " ".join(cells))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------- command line
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="k-means on features: fit clusters, or assign rows to them and report mode coverage")
    p.add_argument("--fit", action="store_true", help="fit clusters on --features and write them to --out")
    p.add_argument("--clusters", type=str, default=None, metavar="IN.npz", help="assign --features to these clusters")
    p.add_argument("--features", type=str, default=None, metavar="A.npy",
                   help="float32 [n, D]: the set to fit on (--fit) or the samples to assign (--clusters)")
    p.add_argument("--ref_features", type=str, default=None, metavar="B.npy",
                   help="with --clusters: the set the clusters were fitted on (default: the counts stored in the file)")
    p.add_argument("--holdout_features", type=str, default=None, metavar="C.npy",
                   help="with --clusters: held-out real rows, reported beside the samples")
    p.add_argument("--k", type=int, nargs="+", default=None, help="with --fit: the number(s) of clusters")
    p.add_argument("--n_init", type=int, default=None, help="with --fit: seedings to try (default 1)")
    p.add_argument("--max_iter", type=int, default=None, help="with --fit: Lloyd steps at the most (default 100)")
    p.add_argument("--tol", type=float, default=None, help="with --fit: stop at this relative inertia decrease (default 0)")
    p.add_argument("--seed", type=int, default=None, help="with --fit: the first seeding's seed (default 0)")
    p.add_argument("--normalize", action="store_true", help="with --fit: scale rows to unit length (stored in the file)")
    p.add_argument("--out", type=str, default=None, metavar="OUT.npz",
                   help="with --fit: the cluster file; several --k write OUT_k<K>.npz")
    p.add_argument("--labels_out", type=str, default=None, metavar="OUT.json",
                   help="the cluster of every row of --features as a JSON list in row order (several --k: OUT_k<K>.json)")
    p.add_argument("--report", type=str, default=None, metavar="OUT.json", help="with --clusters: the mode report")
    return p


FIT_ONLY = ("k", "n_init", "max_iter", "tol", "seed", "out")
ASSIGN_ONLY = ("ref_features", "holdout_features", "report")


def check_args(args) -> None:
    """every contradiction between the flags, before a file is read or the GPU is touched"""
    if args.fit == (args.clusters is not None):
        raise ValueError("cluster: give exactly one of --fit (fit clusters) and --clusters IN.npz (assign to them)")
    if args.features is None:
        raise ValueError("cluster: --features is required")
    if args.fit:
        bad = [f for f in ASSIGN_ONLY if getattr(args, f) is not None]
        if bad:
            raise ValueError(f"cluster: --{' --'.join(bad)} go with --clusters, not with --fit")
        if args.k is None or args.out is None:
            raise ValueError("cluster: --fit needs --k and --out")
        if any(isinstance(k, bool) or not isinstance(k, int) or k < 1 for k in args.k) or len(set(args.k)) != len(args.k):
            raise ValueError(f"cluster: --k takes distinct integers >= 1, got {args.k!r}")
        if not args.out.endswith(".npz"):
            raise ValueError(f"cluster: --out must end in .npz, got {args.out!r}")
        for name, low in (("n_init", 1), ("max_iter", 1), ("seed", 0)):
            v = getattr(args, name)
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < low):
                raise ValueError(f"cluster: --{name} must be an integer >= {low}, got {v!r}")
        if args.tol is not None and not 0.0 <= args.tol < 1.0:
            raise ValueError(f"cluster: --tol must be in [0, 1), got {args.tol!r}")
    else:
        bad = [f for f in FIT_ONLY if getattr(args, f) is not None] + (["normalize"] if args.normalize else [])
        if bad:
            raise ValueError(f"cluster: --{' --'.join(bad)} go with --fit; --clusters takes them from the file")
    if args.labels_out is not None and not args.labels_out.endswith(".json"):
        raise ValueError(f"cluster: --labels_out must end in .json, got {args.labels_out!r}")


def _per_k(path, k, several):
    if path is None or not several:
        return path
    stem, ext = os.path.splitext(path)
    return f"{stem}_k{k}{ext}"


def _write_labels(path, labels) -> None:
    with open(path, "w") as f:
        json.dump([int(v) for v in labels.cpu().tolist()], f)
    print(f"wrote {path}", flush=True)


def _fit(args, dev):
    import torch
    from .neighbors import read_features
    x = torch.from_numpy(read_features(args.features, "--features", "cluster", min_rows=max(args.k))).to(dev)
    out = {}
    for k in args.k:
        km = KMeans(k, n_init=args.n_init or 1, max_iter=args.max_iter or 100, tol=args.tol or 0.0, seed=args.seed or 0,
                    normalize=args.normalize).fit(x)
        path = _per_k(args.out, k, len(args.k) > 1)
        km.save(path)
        print(f"k {k:6d}  inertia {km.inertia:.9g}  steps {km.n_iter}  converged {km.converged}  "
              f"empty {len(km.empty_clusters)}  -> {path}", flush=True)
        if args.labels_out is not None:
            _write_labels(_per_k(args.labels_out, k, len(args.k) > 1), km.labels_)
        out[k] = {"inertia": km.inertia, "n_iter": km.n_iter, "converged": km.converged, "path": path}
    return out


def _assign(args, dev):
    import torch
    from .neighbors import read_features
    km = KMeans.load(args.clusters, device=dev)
    K, D = km.centroids.shape

    def hist(flag):
        a = read_features(getattr(args, flag), "--" + flag, "cluster")
        if a.shape[1] != D:
            raise ValueError(f"cluster: --{flag} has D = {a.shape[1]}, the clusters D = {D}")
        labels = km.predict(torch.from_numpy(a).to(dev))[0]
        return labels, torch.bincount(labels, minlength=K).cpu().numpy()

    labels, counts = hist("features")
    if args.labels_out is not None:
        _write_labels(args.labels_out, labels)
    ref = km.counts.cpu().numpy() if args.ref_features is None else hist("ref_features")[1]
    report = mode_report(ref, counts, None if args.holdout_features is None else hist("holdout_features")[1])
    report.update({"clusters_file": args.clusters, "normalize": km.normalize, "feature_dim": int(D)})
    print(format_table(report))
    if args.report is not None:
        with open(args.report, "w") as f:
            json.dump(report, f, indent=1)
        print(f"wrote {args.report}", flush=True)
    return report


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        check_args(args)
    except ValueError as e:
        parser.error(str(e))
    import torch
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dev = torch.device("cuda", torch.cuda.current_device())
    try:
        return _fit(args, dev) if args.fit else _assign(args, dev)
    except ValueError as e:
        parser.error(str(e))


if __name__ == "__main__":
    main()
