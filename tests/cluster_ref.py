"""fp64 numpy restatement of feature clustering (csrc/kmeans.hip, tinyedm_amd/cluster.py), written from the stated rules and
taking nothing from tinyedm_amd:

    cluster_sums    the kernel's addition order (include/tinyedm_hip.h): cluster k's rows in ascending row number; the row
                    at position p is in chunk p // BLOCK; a chunk's partial is ((+0.0 + row_0) + row_1) + ... in ascending
                    position; the cluster's sum is ((+0.0 + partial_0) + partial_1) + ... in ascending chunk number.  Every
                    add is one IEEE fp64 addition, so numpy reproduces the bits on any finite input.
    lloyd_step      assignment by the DIRECT distance form of fknn_ref (ties to the lower cluster), the empty-cluster rule,
                    the sums above, centroid = sum / count in fp64 rounded to float32 once
    seeding         the D^2 draw from a distance vector: first index whose prefix sum exceeds u * total
    mode_report     the histogram comparison, from the definitions
"""
import math
import os
import re

import numpy as np

import fknn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "tinyedm_hip.h")) as _f:
    BLOCK = int(re.search(r"#define EDM_CLUSTER_BLOCK (\d+)", _f.read()).group(1))
U = 2.0 ** -53


def cluster_sums(x, labels, K, d2=None, block=None):
    """(sums fp64 [K, D], counts int64 [K], d2sums fp64 [K] or None) in the kernel's order"""
    block = BLOCK if block is None else block
    x = np.asarray(x, dtype=np.float32).reshape(len(x), -1).astype(np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    D = x.shape[1]
    cols = x if d2 is None else np.concatenate([x, np.asarray(d2, dtype=np.float64).reshape(-1, 1)], axis=1)
    out = np.zeros((K, cols.shape[1]), np.float64)
    counts = np.zeros(K, np.int64)
    for k in range(K):
        rows = np.flatnonzero(labels == k)                     # ascending row number
        counts[k] = rows.size
        total = np.zeros(cols.shape[1], np.float64)
        for a in range(0, rows.size, block):
            part = np.zeros(cols.shape[1], np.float64)
            for r in rows[a:a + block]:
                part = part + cols[r]
            total = total + part
        out[k] = total
    return out[:, :D].copy(), counts, (None if d2 is None else out[:, D].copy())


def wide(seed, n, D):
    """float32 [n, D] spread over 60 binades.  A sum of a few thousand float32 values of ONE magnitude is exact in fp64
    (24 of 53 bits used) whatever the order; with this spread almost every addition rounds, so the order shows in the bits."""
    r = np.random.default_rng(seed)
    return (r.standard_normal((n, D)) * 2.0 ** r.integers(-30, 31, (n, D))).astype(np.float32)


def fill_empty(labels, d2, K):
    """the empty-cluster rule, in place -> the clusters left empty.  Empty clusters in ascending index; each takes the row
    of largest d2 (ties to the lower row) among the rows not moved before whose cluster keeps another member and whose d2
    is > 0; its label becomes the empty cluster, its d2 becomes 0."""
    n = labels.shape[0]
    moved = np.zeros(n, bool)
    left = []
    for e in range(K):
        counts = np.bincount(labels, minlength=K)
        if counts[e] > 0:
            continue
        ok = ~moved & (counts[labels] > 1) & (d2 > 0)
        if not ok.any():
            left.append(e)
            continue
        best = d2[ok].max()
        r = int(np.flatnonzero(ok & (d2 == best))[0])
        labels[r], d2[r], moved[r] = e, 0.0, True
    return left


def gap_bound(x, c):
    """f32_knn's float-tier bound (tests/test_fknn_gpu.py, twice its error term) per (row, centroid): 2 (D + 2) u (|q| + |r|)^2"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    D = x.shape[1]
    return 2.0 * (D + 2) * U * (np.sqrt((x * x).sum(1))[:, None] + np.sqrt((c * c).sum(1))[None, :]) ** 2


def lloyd_step(x, c, require_gap=False):
    """(labels, d2, new centroids float32, counts, cluster inertia, left empty).  require_gap: assert that the nearest and
    second-nearest centroid of every row are farther apart than gap_bound, and that no cluster runs empty -- the
    conditions under which the device's labels must be these."""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    K = c.shape[0]
    d = R.dist_matrix(x, c)
    labels = np.argmin(d, axis=1).astype(np.int64)               # first minimum: ties to the lower cluster
    rows = np.arange(len(x))
    d2 = d[rows, labels].copy()
    if require_gap:
        assert K >= 2
        two = np.partition(d, 1, axis=1)[:, :2]
        bound = gap_bound(x, c).max(1)
        assert ((two[:, 1] - two[:, 0]) > bound).all(), "a row sits between two centroids closer than the search can tell"
        assert (np.bincount(labels, minlength=K) > 0).all(), "a cluster ran empty"
    left = fill_empty(labels, d2, K)
    sums, counts, inertia = cluster_sums(x, labels, K, d2)
    new = c.copy()
    has = counts > 0
    new[has] = (sums[has] / counts[has, None].astype(np.float64)).astype(np.float32)
    return labels, d2, new, counts, inertia, left


def host_sum(v):
    s = 0.0
    for a in np.asarray(v, np.float64).tolist():
        s += a
    return s


def lloyd(x, init, max_iter=100, require_gap=False):
    """the trajectory [(labels, d2, new centroids, counts, cluster inertia)] until no label changes (that step included)"""
    c, prev, traj = np.asarray(init, np.float32), None, []
    for _ in range(max_iter):
        labels, d2, new, counts, inertia, _ = lloyd_step(x, c, require_gap=require_gap)
        traj.append((labels, d2, new, counts, inertia))
        if prev is not None and np.array_equal(labels, prev):
            break
        prev, c = labels, new
    return traj


def lloyd_inputs(n, D, K, seed):
    """the trajectory inputs: r = default_rng(seed); x = r.standard_normal((n, D)) as float32; init = K distinct rows"""
    r = np.random.default_rng(seed)
    x = r.standard_normal((n, D)).astype(np.float32)
    return x, x[r.choice(n, K, replace=False)]


LLOYD_CASES = [(700, 33, 7, 1), (1200, 24, 6, 2), (515, 67, 9, 3), (300, 3, 5, 4)]


def draw(weights, u):
    """first index whose fp64 prefix sum (row after row) exceeds u * total; None when the total is 0; if u * total rounds
    up to the total, the last row of weight > 0"""
    w = np.asarray(weights, np.float64)
    s, total = 0.0, 0.0
    for v in w.tolist():
        total += v
    if not total > 0.0:
        return None
    target = u * total
    for i, v in enumerate(w.tolist()):
        s += v
        if s > target:
            return i
    return int(np.flatnonzero(w > 0)[-1])


def kmeans_plus_plus(x, K, seed):
    """D^2 seeding with the draws of default_rng(seed): integers(n), then one random() per further row; distances by the
    direct form (exact on dyadic inputs)"""
    x = np.asarray(x, np.float32)
    n = len(x)
    rng = np.random.default_rng(seed)
    chosen = [int(rng.integers(n))]
    mind2 = R.dist_matrix(x, x[chosen[0]:chosen[0] + 1])[:, 0]
    for _ in range(1, K):
        w = mind2.copy()
        w[chosen] = 0.0
        i = draw(w, rng.random())
        if i is None:
            i = min(set(range(n)) - set(chosen))
        chosen.append(i)
        mind2 = np.minimum(mind2, R.dist_matrix(x, x[i:i + 1])[:, 0])
    return np.asarray(chosen, np.int64)


def _block(ref, counts):
    K, n, nref = len(ref), sum(counts), sum(ref)
    p = [r / nref for r in ref]
    q = [c / n for c in counts]
    occ = [k for k in range(K) if ref[k] > 0]
    missing = [k for k in occ if counts[k] == 0]
    js = 0.0
    for a in (p, q):
        for k in range(K):
            if a[k] > 0:
                js += 0.5 * a[k] * math.log(a[k] / (0.5 * (p[k] + q[k])))
    return {"n": n, "share": q, "ratio": [q[k] / p[k] if ref[k] > 0 else None for k in range(K)], "missing": missing,
            "coverage": 1.0 - len(missing) / len(occ), "total_variation": 0.5 * sum(abs(p[k] - q[k]) for k in range(K)),
            "js_divergence": js, "chi2": sum((counts[k] - n * p[k]) ** 2 / (n * p[k]) for k in occ),
            "outside_reference": sum(counts[k] for k in range(K) if ref[k] == 0)}


def mode_report(ref, samples, holdout=None):
    ref = [int(v) for v in ref]
    out = {"clusters": len(ref), "occupied": sum(1 for r in ref if r > 0), "n_ref": sum(ref),
           "reference_share": [r / sum(ref) for r in ref], "samples": _block(ref, [int(v) for v in samples])}
    if holdout is not None:
        out["holdout"] = _block(ref, [int(v) for v in holdout])
    return out


def planted(seed=0, blobs=6, D=16, per=100, scale=20.0):
    """the planted mixture: `blobs` unit-variance blobs of `per` points around scale * e_i in D dimensions, rows shuffled ->
    (x float32 [blobs * per, D], the planted label of every row)"""
    r = np.random.default_rng(seed)
    y = np.repeat(np.arange(blobs), per)
    x = r.standard_normal((blobs * per, D))
    x[np.arange(len(y)), y] += scale
    order = r.permutation(len(y))
    return x[order].astype(np.float32), y[order]


def same_partition(a, b):
    """whether two labelings are equal up to a relabelling"""
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))
