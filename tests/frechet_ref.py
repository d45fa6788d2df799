"""numpy restatement of the fp64 moments, the polynomial-kernel sums, the Frechet distance and KID (tinyedm_amd/frechet.py,
csrc/moments.hip), with the error bounds the tests hold the device to.

uint8 moments are x.astype(float64).T @ x.astype(float64): every product is at most 65025 and every sum stays below 2^53,
so the fp64 matmul is exact whatever order BLAS adds in, and fast.  The host arithmetic after the reductions
(FeatureStats, frechet_distance, kid_from_sums) is the package's own: it is shared, not restated, so that exact moments give
an equal Frechet distance bit for bit; its own correctness is test_frechet_cpu.py's subject (closed forms, numpy.cov, a
brute-force MMD^2)."""
import numpy as np

from tinyedm_amd import frechet as F

EPS = 2.0 ** -53


def _rows(x, index=None, shift=None):
    y = np.asarray(x).reshape(len(x), -1)
    y = (y if index is None else y[np.asarray(index)]).astype(np.float64)
    return y if shift is None else y - np.asarray(shift, dtype=np.float64)


def moments(x, index=None, shift=None):
    """(sum [D], gram [D, D]) of the rows x[index] - shift in fp64"""
    y = _rows(x, index, shift)
    return y.sum(0), y.T @ y


def moments_bound(x, index=None, shift=None):
    """per entry of (sum, gram): 8 N 2^-53 times the sum of the absolute values of the terms.  The terms themselves are
    exact for float32 rows (24 + 24 bits) and rounded once (2^-53 relative) after a shift; an N-term sum in any order is off
    by at most (N - 1) 2^-53 times the sum of the absolute values, to first order: a factor 8 covers both and the reference's
    own rounding."""
    y = np.abs(_rows(x, index, shift))
    n = y.shape[0]
    return 8 * n * EPS * y.sum(0), 8 * n * EPS * (y.T @ y)


def poly_sums(a, idx_a, b, idx_b, gamma, coef0, degree, exclude):
    """(sums [S], the same sums over |k|, the number of terms of a subset): idx None = every row in order, one subset"""
    a2, b2 = np.asarray(a).reshape(len(a), -1), np.asarray(b).reshape(len(b), -1)
    ia = np.arange(len(a2))[None] if idx_a is None else np.asarray(idx_a)
    ib = np.arange(len(b2))[None] if idx_b is None else np.asarray(idx_b)
    sums, mags = [], []
    for ra, rb in zip(ia, ib):
        v = gamma * (a2[ra].astype(np.float64) @ b2[rb].astype(np.float64).T) + coef0
        k = v.copy()
        for _ in range(degree - 1):
            k *= v
        if exclude:
            k = np.where(ra[:, None] == rb[None, :], 0.0, k)
        sums.append(k.sum())
        mags.append(np.abs(k).sum())
    return np.array(sums), np.array(mags), ia.shape[1] * ib.shape[1]


def poly_bound(mags, terms, D):
    """8 (T + 3 D) 2^-53 sum |k|: T terms are added (T 2^-53), each a power of a D-term dot product (D 2^-53 relative for
    data of one sign, times the degree <= 3 used here)"""
    return 8 * (terms + 3 * D) * EPS * mags


def stats(x):
    """FeatureStats of a uint8 [n, ...] set from the exact numpy moments"""
    s, g = moments(x)
    return F.FeatureStats(len(x), s, g, "u8")


def fd(samples, refs):
    return F.frechet_distance(stats(samples), stats(refs))


def kid_sums(x, y, num_subsets, subset_size, degree, seed, coef0=1.0):
    """the three kernel sums of kid() on uint8 sets with gamma = 1 / D, each with its |k| sums and term count"""
    D = np.asarray(x)[0].size
    g = 1.0 / D / 255.0 ** 2
    ix, iy = (None, None) if num_subsets == 0 else F.subset_indices(len(x), len(y), num_subsets, subset_size, seed)
    return (poly_sums(x, ix, x, ix, g, coef0, degree, True), poly_sums(y, iy, y, iy, g, coef0, degree, True),
            poly_sums(x, ix, y, iy, g, coef0, degree, False))


def kid(x, y, num_subsets, subset_size, degree=3, seed=0):
    """(kid_from_sums of the reference sums, the bound on |kid - the device's| that follows from the three sum bounds)"""
    (sxx, axx, txx), (syy, ayy, tyy), (sxy, axy, txy) = kid_sums(x, y, num_subsets, subset_size, degree, seed)
    D = np.asarray(x)[0].size
    mx, my = (len(x), len(y)) if num_subsets == 0 else (subset_size, subset_size)
    per = (poly_bound(axx, txx, D) / (mx * (mx - 1)) + poly_bound(ayy, tyy, D) / (my * (my - 1))
           + 2 * poly_bound(axy, txy, D) / (mx * my))
    return F.kid_from_sums(sxx, syy, sxy, (mx, my)), float(per.mean())


def trace_term_bound(cov_a, cov_b):
    """A bound on |trace_term| of frechet_distance when the two covariances are equal up to rounding.  The exact term is
    the squared Bures distance, at most |sqrt(A) - sqrt(B)|_F^2 <= |A - B|_1 <= sqrt(D) |A - B|_F (Powers & Stormer 1970).
    The computed term adds the rounding of tr A + tr B (D 2^-53 relative, generously 4 D) and of the D eigenvalues of
    A^(1/2) B A^(1/2): each is off by at most delta = 16 D 2^-53 |A|_2 |B|_2 (two backward-stable eigensolvers and three
    products), and |sqrt(max(l + d, 0)) - sqrt(l)| <= sqrt(|d|), whether or not the eigenvalue was clipped."""
    D = cov_a.shape[0]
    na, nb = np.linalg.norm(cov_a, 2), np.linalg.norm(cov_b, 2)
    delta = 16 * D * EPS * na * nb
    return (np.sqrt(D) * np.linalg.norm(cov_a - cov_b) + 2 * D * np.sqrt(delta)
            + 4 * D * EPS * (np.trace(cov_a) + np.trace(cov_b)))
