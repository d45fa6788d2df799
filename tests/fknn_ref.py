"""fp64 numpy restatement of the feature-space search (csrc/neighbors_f32.hip) and of precision, recall, density and
coverage on float features, written straight from the definitions and taking nothing from tinyedm_amd:

    d2(q, r) = sum_j (q_j - r_j)^2 in fp64, the DIRECT form (no |q|^2 + |r|^2 - 2 q.r expansion, so no cancellation)
    neighbours ordered by (d2, reference index); exclude_self leaves out r == q by index (a duplicate row stays, at d2 = 0)
    every ball closed (<=), a radius per reference

For dyadic inputs (small integers / 8) every product and sum is exact in fp64, so this is the unique answer bit for bit;
for general float32 inputs it is within D ulps of the largest term of the true value.
"""
import numpy as np


def dist_matrix(q, r):
    """d2 [Q, R] fp64 by the direct form, a block of queries at a time"""
    q = np.asarray(q).reshape(len(q), -1).astype(np.float64)
    r = np.asarray(r).reshape(len(r), -1).astype(np.float64)
    out = np.empty((len(q), len(r)), np.float64)
    step = max(1, (1 << 22) // max(1, r.size))
    for a in range(0, len(q), step):
        out[a:a + step] = ((q[a:a + step, None, :] - r[None, :, :]) ** 2).sum(-1)
    return out


def knn(q, r, k, exclude_self=False, d=None):
    """(dist fp64 [Q, k], idx int64 [Q, k]) ascending by (d2, index)"""
    d = dist_matrix(q, r) if d is None else d
    Q, R = d.shape
    dist, idx = np.empty((Q, k), np.float64), np.empty((Q, k), np.int64)
    cols = np.arange(R)
    for i in range(Q):
        keep = cols != i if exclude_self else np.ones(R, bool)
        c = cols[keep]
        order = np.lexsort((c, d[i, c]))[:k]
        idx[i], dist[i] = c[order], d[i, c[order]]
    return dist, idx


def ball_count(q, r, radii, exclude_self=False, d=None):
    """int64 [Q]: per query the references r with d2(q, r) <= radii[r] in fp64; exclude_self leaves out r == q (by index)"""
    d = dist_matrix(q, r) if d is None else d
    inside = d <= np.asarray(radii, dtype=np.float64).reshape(1, -1)
    if exclude_self:
        n = min(d.shape)
        inside[np.arange(n), np.arange(n)] = False
    return inside.sum(1).astype(np.int64)


def radii(x, k, d=None):
    """fp64 [n]: the k-th smallest distance from each row to the other rows (d: dist_matrix(x, x), if the caller holds it)"""
    return knn(x, x, k, exclude_self=True, d=d)[0][:, k - 1]


def counts(X, Y, k):
    """(hitsX [N], hitsY [M], nearY [M], rX [M], rY [N])"""
    rX, rY = radii(X, k), radii(Y, k)
    return ball_count(Y, X, rX), ball_count(X, Y, rY), dist_matrix(X, Y).min(1), rX, rY


def ratios(hx, hy, near, rX, k):
    """the four ratios from float distances: the coverage compare runs in fp64"""
    near, rX = np.asarray(near, np.float64), np.asarray(rX, np.float64)
    N, M = len(hx), len(hy)
    num = {"precision_count": int((hx > 0).sum()), "recall_count": int((hy > 0).sum()), "density_sum": int(hx.sum()),
           "coverage_count": int((near <= rX).sum())}
    return {"k": k, "num_real": M, "num_fake": N, "precision": num["precision_count"] / N,
            "recall": num["recall_count"] / M, "density": num["density_sum"] / (k * N),
            "coverage": num["coverage_count"] / M, **num}


def prdc(X, Y, k):
    hx, hy, near, rX, _ = counts(X, Y, k)
    return ratios(hx, hy, near, rX, k)


def prdc_per_class(X, Y, lx, ly, k):
    """{label: prdc of the two subsets, or None where a subset has fewer than k + 1 rows}"""
    lx, ly = np.asarray(lx), np.asarray(ly)
    out = {}
    for c in sorted(set(lx.tolist()) | set(ly.tolist())):
        Xc, Yc = np.asarray(X)[lx == c], np.asarray(Y)[ly == c]
        out[int(c)] = prdc(Xc, Yc, k) if min(len(Xc), len(Yc)) >= k + 1 else None
    return out


def dyadic(seed, n, D):
    """float32 [n, D] of small integers / 8: every product and sum of such rows is exact in fp64 whatever the order"""
    return (np.random.default_rng(seed).integers(-24, 25, (n, D)) / 8).astype(np.float32)
