"""numpy / fp64 restatements of the training step's own fp32 kernels (csrc/optim.hip k_diffuse, k_diffuse_given and the
Adam + EMA forms, csrc/common.h dropout_keep8 behind edm_dropout_mask), for tests/test_step_exact_gpu.py and
tests/test_step_ref_cpu.py.  Philox4x32-10 and Box-Muller are those of tests/evaluate_ref.py (their known-answer vectors
live in tests/test_evaluate_cpu.py); this file only states the counter layouts and the arithmetic.

Streams, all keyed by (seed_lo, seed_hi) of the seed THE KERNEL receives:
  Diffuser noise   counter (q lo, q hi, 0xD1FF, step), q = e // 4 over the flat [B * CHW] array: element e is normal e % 4
                   (Box-Muller of words (0, 1) gives normals 0, 1; of words (2, 3) normals 2, 3)
  Diffuser sigma   counter (b, 0, 0x5167, step): sample b's sigma is exp(P_mean + P_std * normal 0)
  dropout          counter (i8 lo, i8 hi, sub, step), i8 = e // 8: element e takes the 16 bits 16 * (j & 1) .. of word
                   j >> 1, j = e % 8, and is kept iff they are >= thr = round(p * 65536)
"""
import math

import numpy as np

from evaluate_ref import box_muller, philox4x32_10

NOISE_TAG, SIGMA_TAG = 0xD1FF, 0x5167
U32 = 0xFFFFFFFF


def f32(x):
    """the fp32 value a kernel receives for the Python number x, widened to a Python float"""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ Diffuser
def noise_counters(idx, step):
    """counter tuples (c0, c1, c2, c3) of the noise stream for the flat element indices idx"""
    q = np.asarray(idx, dtype=np.uint64) // np.uint64(4)
    return q & np.uint64(U32), q >> np.uint64(32), np.full_like(q, NOISE_TAG), np.full_like(q, int(step) & U32)


def sigma_counters(B, step):
    b = np.arange(B, dtype=np.uint64)
    return b, np.zeros_like(b), np.full_like(b, SIGMA_TAG), np.full_like(b, int(step) & U32)


def diffuse_unit_noise(idx, seed, step):
    """fp64 unit normals of the flat elements idx (any integer array) of a diffuse(seed, step) call"""
    idx = np.asarray(idx, dtype=np.uint64)
    r = philox4x32_10(*noise_counters(idx, step), seed & U32, seed >> 32)
    n0, n1 = box_muller(r[0], r[1])
    n2, n3 = box_muller(r[2], r[3])
    return np.choose((idx % np.uint64(4)).astype(np.int64), [n0, n1, n2, n3])


def diffuse_sigma(B, P_mean, P_std, seed, step):
    """(sigma64 [B], n0 [B]): the per-sample noise levels and the normals they were drawn from"""
    r = philox4x32_10(*sigma_counters(B, step), seed & U32, seed >> 32)
    n0, _ = box_muller(r[0], r[1])
    return np.exp(f32(P_mean) + f32(P_std) * n0), n0


def diffuse_ref(clean64, P_mean, P_std, seed, step):
    """(noisy64, sigma64, unit_noise64) of ops.diffuse(clean, P_mean, P_std, seed, step), clean64 [B, ...] fp64"""
    clean64 = np.asarray(clean64, dtype=np.float64)
    B = clean64.shape[0]
    sigma, _ = diffuse_sigma(B, P_mean, P_std, seed, step)
    unit = diffuse_unit_noise(np.arange(clean64.size), seed, step).reshape(clean64.shape)
    return clean64 + sigma.reshape((B,) + (1,) * (clean64.ndim - 1)) * unit, sigma, unit


# ------------------------------------------------------------------------------------------------ dropout mask
def dropout_threshold(p):
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def dropout_keep_ref(n, p, seed, sub, step, elems=None):
    """(keep uint8, scale) of ops.dropout_mask(n, p, seed, sub, step); elems: only these element indices (default all n)"""
    idx = np.arange(n, dtype=np.uint64) if elems is None else np.asarray(elems, dtype=np.uint64)
    if p <= 0:
        return np.ones(idx.shape, dtype=np.uint8), 1.0
    thr = dropout_threshold(p)
    i8 = idx // np.uint64(8)
    r = philox4x32_10(i8 & np.uint64(U32), i8 >> np.uint64(32), np.full_like(i8, int(sub) & U32),
                      np.full_like(i8, int(step) & U32), seed & U32, seed >> 32)
    j = (idx % np.uint64(8)).astype(np.int64)
    word = np.choose(j >> 1, r)
    bits = (word >> (np.uint64(16) * (j & 1).astype(np.uint64))) & np.uint64(0xFFFF)
    return (bits >= np.uint64(thr)).astype(np.uint8), 65536.0 / (65536 - thr)


# ------------------------------------------------------------------------------------------------ Adam + EMA
def bias_corrections(b1, b2, step):
    """(bc1, bc2sqrt) as edm_adam_ema forms them: in double from the fp32 betas, rounded to fp32 once"""
    bc1 = np.float32(1.0 - math.pow(f32(b1), step))
    bc2sqrt = np.float32(math.sqrt(1.0 - math.pow(f32(b2), step)))
    return float(bc1), float(bc2sqrt)


def adam_ema_ref(theta, grad, m, v, ema, profiles, betas, *, lr, b1, b2, eps, bc1, bc2sqrt, ema_beta, grad_scale):
    """The update of k_adam_ema (and of every other form) in fp64.  Arrays: fp32-valued, any float dtype; ema may be None,
    profiles / betas are sequences (possibly empty).  Every hyper-parameter is rounded to fp32 first and widened, as the
    kernel receives it (1 - float32(0.999) is 3e-5 away from 1 - 0.999); bc1 and bc2sqrt are taken as given (the kernel's:
    bias_corrections) and grad_scale may be any double (the guarded forms multiply it by the record's coef).
    Returns a dict: the new theta / m / v / ema / profiles, and the magnitudes the error bounds are stated in:
      mag_m = |b1 m| + |(1 - b1) g_s|, mag_v = |b2 v| + |(1 - b2) g_s^2|, dtheta = the update theta' - theta,
      mag_ema = |beta e| + |(1 - beta) theta'|, mag_profiles[k] likewise with betas[k]."""
    theta, grad, m, v = (np.asarray(a, dtype=np.float64) for a in (theta, grad, m, v))
    lr, b1, b2, eps, ema_beta = (f32(x) for x in (lr, b1, b2, eps, ema_beta))
    bc1, bc2sqrt = float(bc1), float(bc2sqrt)
    gs = grad * float(grad_scale)
    m1, v1 = b1 * m + (1.0 - b1) * gs, b2 * v + (1.0 - b2) * gs * gs
    dtheta = -(lr / bc1) * m1 / (np.sqrt(v1) / bc2sqrt + eps)
    t1 = theta + dtheta
    out = dict(theta=t1, m=m1, v=v1, dtheta=dtheta, ema=None, mag_ema=None,
               mag_m=np.abs(b1 * m) + np.abs((1.0 - b1) * gs), mag_v=np.abs(b2 * v) + np.abs((1.0 - b2) * gs * gs))

    def lerp(beta, e):
        e = np.asarray(e, dtype=np.float64)
        return beta * e + (1.0 - beta) * t1, np.abs(beta * e) + np.abs((1.0 - beta) * t1)

    if ema is not None:
        out["ema"], out["mag_ema"] = lerp(ema_beta, ema)
    pairs = [lerp(f32(bk), p) for bk, p in zip(betas, profiles)]
    out["profiles"], out["mag_profiles"] = [p for p, _ in pairs], [g for _, g in pairs]
    return out


U = 2.0 ** -24


def adam_state(n, seed, K=0):
    """fp32 arenas of a running optimizer: theta, grad, m, v > 0, ema and K profiles, all random and non-zero, plus two
    forced elements when n >= 3: element n // 2 has g = m = v = 0 (its update must be exactly 0) and element 0 has
    v = 1e-30.  m carries its gradient's sign, as a running mean of gradients does: theta's bound is stated relative to the
    update, which presumes that b1 m + (1 - b1) g does not cancel (m's own bound is in the magnitudes of its terms and
    presumes nothing; theta, ema and the profiles have independent signs)."""
    g = np.random.default_rng(seed)
    F = np.float32
    grad = g.standard_normal(n).astype(F)
    grad[grad == 0] = F(1)
    st = dict(theta=g.standard_normal(n).astype(F), grad=grad,
              m=((0.01 + 0.1 * np.abs(g.standard_normal(n))) * np.sign(grad)).astype(F),
              v=(0.01 * g.random(n) + 1e-4).astype(F), ema=g.standard_normal(n).astype(F),
              profiles=[g.standard_normal(n).astype(F) for _ in range(K)])
    if n >= 3:
        z = n // 2
        st["grad"][z] = st["m"][z] = st["v"][z] = 0
        st["v"][0] = F(1e-30)
    return st


def adam_ema_bounds(ref, theta, ema_beta, betas=()):
    """the elementwise error bounds of an fp32 evaluation against adam_ema_ref's result `ref` (theta: the OLD weights):
    twice the rounding count of each expression, u = 2^-24, in the magnitudes of its terms"""
    b = dict(m=2 * 3 * U * ref["mag_m"], v=2 * 4 * U * ref["mag_v"])
    b["theta"] = 2 * U * np.abs(np.asarray(theta, dtype=np.float64)) + 2 * 8 * U * np.abs(ref["dtheta"])
    if ref["ema"] is not None:
        b["ema"] = 2 * 3 * U * ref["mag_ema"] + (1.0 - f32(ema_beta)) * b["theta"]
    b["profiles"] = [2 * 3 * U * g + (1.0 - f32(bk)) * b["theta"] for g, bk in zip(ref["mag_profiles"], betas)]
    return b


def adam_ema_f32(theta, grad, m, v, ema, *, lr, b1, b2, eps, bc1, bc2sqrt, ema_beta, grad_scale, fma):
    """The same expressions in numpy float32, in the kernels' order of operations; fma: every a * b + c is one rounding
    (the product of two floats is exact in double), else two.  The yardstick a bound is judged by before a kernel is."""
    F = np.float32
    theta, grad, m, v = (np.asarray(a, dtype=F) for a in (theta, grad, m, v))
    lr, b1, b2, eps, bc1, bc2sqrt, ema_beta, grad_scale = (F(x) for x in (lr, b1, b2, eps, bc1, bc2sqrt, ema_beta, grad_scale))

    def mad(a, x, c):
        if fma:
            return (np.asarray(a, dtype=np.float64) * np.asarray(x, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)
        return (a * x + c).astype(F)

    gj = grad * grad_scale
    m1 = mad(b1, m, (F(1) - b1) * gj)
    v1 = mad(b2, v, (F(1) - b2) * gj * gj)
    t1 = theta - (lr / bc1) * m1 / (np.sqrt(v1) / bc2sqrt + eps)
    e1 = None if ema is None else mad(ema_beta, np.asarray(ema, dtype=F), (F(1) - ema_beta) * t1)
    return dict(theta=t1, m=m1, v=v1, ema=e1)
