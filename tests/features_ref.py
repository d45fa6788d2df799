"""Numpy restatement of tinyedm_amd/features.py for the tests: the pooled mean (fp64 sum, / HW, rounded to fp32 once), the
ridge probe's closed form, and the k-NN vote.  Plain and slow on purpose; nothing here imports the code under test."""
import numpy as np


# ------------------------------------------------------------------------------------------------ pooled mean
def pool(x) -> np.ndarray:
    """x [B, H, W, C] float32 -> [B, C] float32: (float)((sum_p (double)x) / HW)"""
    x = np.asarray(x, dtype=np.float32)
    B, H, W, C = x.shape
    return (x.reshape(B, H * W, C).astype(np.float64).sum(axis=1) / float(H * W)).astype(np.float32)


def eighths(seed, shape) -> np.ndarray:
    """float32 values k / 8 with integer |k| <= 64: every partial sum of up to 2^40 of them is exact in fp32 and fp64,
    in any order, so sum / HW rounded to fp32 is one defined number"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-64, 65, size=shape).astype(np.float32) / np.float32(8.0)).astype(np.float32)


def pool_bound(x) -> np.ndarray:
    """per element [B, C]: 2^-24 |mean| (the one rounding to fp32) + HW 2^-52 mean_p |x| (the fp64 accumulation: each of the
    HW - 1 additions rounds a partial sum of at most sum_p |x| by 2^-53)"""
    x = np.asarray(x, dtype=np.float64)
    B, H, W, C = x.shape
    x = x.reshape(B, H * W, C)
    return 2.0 ** -24 * np.abs(x.mean(axis=1)) + (H * W) * 2.0 ** -52 * np.abs(x).mean(axis=1)


# ------------------------------------------------------------------------------------------------ ridge probe
def ridge_fit(x, y, num_classes, l2=1e-3):
    """(mu [D], W [D, K], ybar [K]) of the least-squares map of centred rows onto centred one-hot targets, fp64:
    (S + l2 (tr S / D) I) W = X^T Y / n - mu ybar^T with S = X^T X / n - mu mu^T"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    n, D = x.shape
    Y = np.zeros((n, num_classes))
    Y[np.arange(n), y] = 1.0
    mu, ybar = x.sum(0) / n, Y.sum(0) / n
    S = x.T @ x / n - np.outer(mu, mu)
    A = S + l2 * (np.trace(S) / D) * np.eye(D)
    return mu, np.linalg.solve(A, x.T @ Y / n - np.outer(mu, ybar)), ybar


def ridge_predict(fit, x) -> np.ndarray:
    """argmax_c ((x - mu) W + ybar)_c, ties to the lower class (numpy's argmax returns the first maximum)"""
    mu, W, ybar = fit
    return np.argmax((np.asarray(x, dtype=np.float64) - mu) @ W + ybar, axis=1)


# ------------------------------------------------------------------------------------------------ k-NN vote
def unit_rows(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    nrm = np.sqrt((x * x).sum(1, keepdims=True))
    return (x / np.where(nrm > 0, nrm, 1.0)).astype(np.float32)


def knn_indices(train_x, test_x, k) -> np.ndarray:
    """[Q, k] the k nearest L2-normalised training rows by fp64 squared distance, ties to the lower index"""
    a, b = unit_rows(test_x).astype(np.float64), unit_rows(train_x).astype(np.float64)
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    return np.stack([np.lexsort((np.arange(b.shape[0]), row))[:k] for row in d2])


def vote(neighbour_labels, num_classes) -> np.ndarray:
    """[Q, k] labels, nearest first -> majority class; a tied vote goes to the class of the nearest neighbour among the
    tied classes"""
    out = []
    for row in np.asarray(neighbour_labels, dtype=np.int64):
        counts = np.bincount(row, minlength=num_classes)
        tied = set(np.nonzero(counts == counts.max())[0].tolist())
        out.append(next(int(c) for c in row if int(c) in tied))
    return np.array(out, dtype=np.int64)


def knn_predict(train_x, train_y, test_x, k, num_classes) -> np.ndarray:
    return vote(np.asarray(train_y, dtype=np.int64)[knn_indices(train_x, test_x, k)], num_classes)


def blobs(num_classes=3, D=8, per_class=20, std=0.5, sep=4.0, seed=0):
    """Gaussian blobs with means sep * e_c -> (float32 [n, D], int64 [n]), classes interleaved"""
    rng = np.random.default_rng(seed)
    y = np.arange(num_classes * per_class, dtype=np.int64) % num_classes
    x = rng.normal(0.0, std, size=(y.shape[0], D))
    x[np.arange(y.shape[0]), y] += sep
    return x.astype(np.float32), y
