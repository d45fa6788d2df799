"""int64 numpy restatement of the ball count (csrc/neighbors.hip, k_u8_ball_count) and of precision, recall, density and
coverage in pixel space, written straight from the definitions and taking nothing from tinyedm_amd:

    X reals uint8 [M, D], Y samples uint8 [N, D], d2 the exact integer squared distance, every ball closed (<=)
    rX[i] = k-th smallest d2(X_i, X_i') over i' != i (by index: a duplicate is a neighbour at distance 0), rY[j] likewise
    hitsX[j] = #{i : d2(Y_j, X_i) <= rX[i]}   hitsY[i] = #{j : d2(X_i, Y_j) <= rY[j]}   nearY[i] = min_j d2(X_i, Y_j)
    precision = #{j : hitsX[j] > 0} / N   density = sum_j hitsX[j] / (k N)
    recall = #{i : hitsY[i] > 0} / M      coverage = #{i : nearY[i] <= rX[i]} / M
"""
import numpy as np


def dist_matrix(q, r):
    """exact d2 [Q, R] int64"""
    q = np.asarray(q).reshape(len(q), -1).astype(np.int64)
    r = np.asarray(r).reshape(len(r), -1).astype(np.int64)
    return (q * q).sum(1)[:, None] + (r * r).sum(1)[None, :] - 2 * (q @ r.T)


def ball_count(q, r, radii, exclude_self=False):
    """int64 [Q]: per query the references r with d2(q, r) <= radii[r]; exclude_self leaves out r == q (by index)"""
    d = dist_matrix(q, r)
    inside = d <= np.asarray(radii, dtype=np.int64).reshape(1, -1)
    if exclude_self:
        n = min(d.shape)
        inside[np.arange(n), np.arange(n)] = False
    return inside.sum(1).astype(np.int64)


def radii(x, k):
    """int64 [n]: the k-th smallest distance from each row to the other rows"""
    d = dist_matrix(x, x)
    out = np.empty(len(d), np.int64)
    for i in range(len(d)):
        out[i] = np.sort(np.delete(d[i], i))[k - 1]
    return out


def counts(X, Y, k):
    """(hitsX [N], hitsY [M], nearY [M], rX [M], rY [N])"""
    rX, rY = radii(X, k), radii(Y, k)
    return ball_count(Y, X, rX), ball_count(X, Y, rY), dist_matrix(X, Y).min(1), rX, rY


def prdc(X, Y, k):
    hx, hy, near, rX, _ = counts(X, Y, k)
    N, M = len(hx), len(hy)
    num = {"precision_count": int((hx > 0).sum()), "recall_count": int((hy > 0).sum()), "density_sum": int(hx.sum()),
           "coverage_count": int((near <= rX).sum())}
    return {"k": k, "num_real": M, "num_fake": N, "precision": num["precision_count"] / N,
            "recall": num["recall_count"] / M, "density": num["density_sum"] / (k * N),
            "coverage": num["coverage_count"] / M, **num}


def prdc_per_class(X, Y, lx, ly, k):
    """{label: prdc of the two subsets, or None where a subset has fewer than k + 1 images}"""
    lx, ly = np.asarray(lx), np.asarray(ly)
    out = {}
    for c in sorted(set(lx.tolist()) | set(ly.tolist())):
        Xc, Yc = np.asarray(X)[lx == c], np.asarray(Y)[ly == c]
        out[int(c)] = prdc(Xc, Yc, k) if min(len(Xc), len(Yc)) >= k + 1 else None
    return out
