"""numpy restatement of the exact nearest-neighbour search (csrc/neighbors.hip) and of the host statistics of
tinyedm_amd/neighbors.py, in int64 and written independently of both: the full distance matrix, np.lexsort on
(index, distance), diagonal masking for exclude_self."""
import numpy as np


def dist_matrix(q, r):
    """exact d2 [Q, R] int64 of uint8 [Q, ...] against uint8 [R, ...]"""
    q = np.asarray(q).reshape(len(q), -1).astype(np.int64)
    r = np.asarray(r).reshape(len(r), -1).astype(np.int64)
    # |q|^2 + |r|^2 - 2 q.r in int64: exact (every term below 2^31 for D <= 32768) and cheaper than the [Q, R, D] differences
    return (q * q).sum(1)[:, None] + (r * r).sum(1)[None, :] - 2 * (q @ r.T)


def knn(q, r, k, exclude_self=False):
    """-> (dist int64 [Q, k], idx int64 [Q, k]): per query the k smallest (d2, index) keys, ascending"""
    d = dist_matrix(q, r)
    Q, R = d.shape
    cols = np.arange(R)
    dist, idx = np.empty((Q, k), np.int64), np.empty((Q, k), np.int64)
    for i in range(Q):
        order = np.lexsort((cols, d[i]))            # last key is primary: distance, then index
        if exclude_self:
            order = order[order != i]
        idx[i] = order[:k]
        dist[i] = d[i, order[:k]]
    return dist, idx


def rms(d2, D):
    return np.sqrt(np.asarray(d2, np.float64) / D) / 255.0


def summarize(d2):
    a = np.sort(np.asarray(d2, np.float64).reshape(-1))
    out = {"n": int(a.size), "min": float(a[0])}
    for p in (1, 5, 25, 50, 75, 95):
        pos = (a.size - 1) * p / 100.0               # linear interpolation between order statistics
        lo = int(np.floor(pos))
        hi = min(lo + 1, a.size - 1)
        out[f"p{p}"] = float(a[lo] + (a[hi] - a[lo]) * (pos - lo))
    out["mean"] = float(a.sum() / a.size)
    return out


def closer_than_holdout(sample_d2, holdout_d2):
    """pair by pair, in integers"""
    twice = 0
    for s in np.asarray(sample_d2).reshape(-1).tolist():
        for h in np.asarray(holdout_d2).reshape(-1).tolist():
            twice += 2 if s < h else (1 if s == h else 0)
    return twice / (2 * len(np.asarray(sample_d2).reshape(-1)) * len(np.asarray(holdout_d2).reshape(-1)))


def duplicates(dist, idx, max_d2):
    out = []
    for i in range(len(dist)):
        for b in range(len(dist[i])):
            if dist[i][b] <= max_d2:
                out.append((i, int(idx[i][b]), int(dist[i][b])))
    return out
