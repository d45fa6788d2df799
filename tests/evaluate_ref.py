"""numpy restatements for the loss-by-noise-level tests: the noise of ops.eval_diffuse (Philox4x32-10 + Box-Muller in
uint64 / fp64 with its counter layout), the training-distribution levels, the per-level statistics and their merge."""
import math
import statistics

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
EVAL_TAG = 0x45560000


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = c[0] * np.uint64(0xD2511F53)
        p1 = c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def box_muller(a, b):
    u1 = ((a >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    u2 = ((b >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)


def eval_noise(shape, ids, levels, seed, draw):
    """fp64 [B, ...]: element j of sample b is normal j % 4 of
    philox((j / 4, ids[b], 0x45560000 ^ levels[b], draw), (seed_lo, seed_hi))"""
    B, CHW = shape[0], int(np.prod(shape[1:]))
    assert len(ids) == len(levels) == B
    j = np.arange(CHW, dtype=np.uint64)[None, :]
    one = np.ones((B, 1), dtype=np.uint64)
    i = np.asarray(ids, dtype=np.uint64)[:, None]
    tag = (np.uint64(EVAL_TAG) ^ np.asarray(levels, dtype=np.uint64))[:, None]
    r = philox4x32_10(j // np.uint64(4) * one, i + 0 * j, tag + 0 * j, np.uint64(draw) + 0 * j * one,
                      seed & 0xFFFFFFFF, seed >> 32)
    n0, n1 = box_muller(r[0], r[1])
    n2, n3 = box_muller(r[2], r[3])
    n = np.stack([n0, n1, n2, n3], axis=2)                  # [B, CHW, 4]
    k = (np.arange(CHW) % 4)[None, :, None]
    return np.take_along_axis(n, np.broadcast_to(k, (B, CHW, 1)), axis=2)[..., 0].reshape(shape)


def level_sigmas(P_mean, P_std, L):
    nd = statistics.NormalDist()
    return [math.exp(P_mean + P_std * nd.inv_cdf((l + 0.5) / L)) for l in range(L)]


def level_sums(se, chw):
    """se [draws, L, n] -> [3, L]: count, sum and sum of squares over the images of mean_draws(se) / chw"""
    v = np.asarray(se, dtype=np.float64).mean(axis=0) / chw
    return np.stack([np.full(v.shape[0], float(v.shape[1])), v.sum(axis=1), (v * v).sum(axis=1)])


def merge_level_sums(parts):
    return np.sum(np.stack([np.asarray(p, dtype=np.float64) for p in parts]), axis=0)


def level_stats(se, chw, sigmas, sigma_data):
    """straight from the matrix: mse, the standard error of the mean over the images, lambda(sigma) * mse"""
    v = np.asarray(se, dtype=np.float64).mean(axis=0) / chw            # [L, n]
    n = v.shape[1]
    mse = v.mean(axis=1)
    stderr = v.std(axis=1, ddof=1) / math.sqrt(n) if n > 1 else None
    lam = np.array([(s * s + sigma_data ** 2) / (s * sigma_data) ** 2 for s in sigmas])
    return {"count": [n] * v.shape[0], "mse": mse, "mse_stderr": stderr, "loss": lam * mse}
