"""The inputs of the ideal-denoiser GPU tests, built once per shape and shared (numpy only, so that the effective counts
and the tolerances can be worked out without a GPU).

Soft data.  Uniform random uint8 images are one-hot at every sigma below ~5, so the soft cases use clustered data: group g
of the references (rows j with j % 4 == g) is one random base image plus a uniform integer perturbation of +-spread_g, the
spread matched to the sigma of the group, and a query of level sigma_g is a reference of group g plus sigma_g * N(0, 1).
Every soft case asserts on the fp64 restatement alone that its mean effective count lies in [2, R / 2]."""
import numpy as np

import ideal_ref as IR

SOFT_SIGMAS = (0.2, 0.5, 2.0, 10.0)
SOFT_SPREAD = {0.2: 1, 0.5: 3, 2.0: 12, 10.0: 60}       # at K = 3072; scaled by sqrt(3072 / K), see soft_case
SMALL_SPREAD = 40                                     # R < 16, found by trial on the fp64 restatement (K = 35, R = 5)
HARD_SIGMAS = (0.002, 0.05, 80.0)

# (Q, R, C, H, W, ref_chunk, misaligned)
SHAPES = {
    "one": (1, 1, 1, 1, 1, None, False),                 # smallest possible
    "tails": (3, 5, 1, 5, 7, None, False),               # K = 35: every tail at once
    "chunks": (17, 200, 3, 8, 8, 64, False),             # four chunks, a tail of 8
    "cifar": (130, 333, 3, 32, 32, None, False),         # real width; Q and R cross tile edges
    "unaligned": (17, 200, 3, 8, 8, 64, True),           # "chunks" with the set at an odd byte, the queries at an odd element
}
_cache = {}


def _spread(sigma, K):
    return max(1, int(round(SOFT_SPREAD[sigma] * np.sqrt(3072.0 / K))))


def soft_case(name):
    """clustered data with per-row sigma cycling through SOFT_SIGMAS -> (data uint8 [R, C, H, W], x fp32 [Q, C, H, W],
    sigma fp32 [Q])"""
    Q, R, C, H, W, _, _ = SHAPES[name]
    rng = np.random.default_rng(1000 + Q * 7 + R)
    K = C * H * W
    G = len(SOFT_SIGMAS) if R >= 16 else 1               # a handful of references: one cluster for every level
    data = np.zeros((R, C, H, W), dtype=np.uint8)
    for g in range(G):
        rows = np.arange(g, R, G)
        base = rng.integers(40, 216, (C, H, W))
        s = _spread(SOFT_SIGMAS[g], K) if G > 1 else SMALL_SPREAD
        data[rows] = np.clip(base[None] + rng.integers(-s, s + 1, (len(rows), C, H, W)), 0, 255).astype(np.uint8)
    sig = np.array([SOFT_SIGMAS[q % len(SOFT_SIGMAS)] for q in range(Q)], dtype=np.float32)
    pick = np.array([rng.choice(np.arange(q % G, R, G)) for q in range(Q)])
    y = IR.normalize(data).reshape(R, C, H, W)
    x = (y[pick] + sig[:, None, None, None].astype(np.float64) * rng.standard_normal((Q, C, H, W))).astype(np.float32)
    return data, x, sig


def hard_case(name):
    """uniform random data with per-row sigma cycling through HARD_SIGMAS, x = y_j + sigma * n -> (data, x, sigma, j)"""
    Q, R, C, H, W, _, _ = SHAPES[name]
    rng = np.random.default_rng(2000 + Q * 7 + R)
    data = rng.integers(0, 256, (R, C, H, W), dtype=np.uint8)
    sig = np.array([HARD_SIGMAS[q % 3] for q in range(Q)], dtype=np.float32)
    pick = rng.integers(0, R, Q)
    y = IR.normalize(data).reshape(R, C, H, W)
    x = (y[pick] + sig[:, None, None, None].astype(np.float64) * rng.standard_normal((Q, C, H, W))).astype(np.float32)
    return data, x, sig, pick


def references(data, x, sigma, ref_labels=None, labels=None):
    """the three forms of the restatement on one case -> (truth, tol): tol[k] for k in D, lse, entropy by the rule
    8 * max(err_b, err_c) + floor, floor = 2^-20 for D and 2^-20 max(1, |value|) for the statistics"""
    a = IR.ideal(x, sigma, data, form="f64", ref_labels=ref_labels, labels=labels)
    b = IR.ideal(x, sigma, data, form="f32", ref_labels=ref_labels, labels=labels)
    c = IR.ideal(x, sigma, data, form="f32x", ref_labels=ref_labels, labels=labels)
    tol, errs = {}, {}
    for k in ("D", "lse", "entropy"):
        eb, ec = np.abs(b[k] - a[k]).max(), np.abs(c[k] - a[k]).max()
        floor = 2.0 ** -20 * (1.0 if k == "D" else max(1.0, float(np.abs(a[k]).max())))
        errs[k] = max(eb, ec)
        tol[k] = 8.0 * errs[k] + floor
    return a, tol, errs


def cached(kind, name):
    """(inputs, truth, tol, errs) of soft_case / hard_case `name`, computed once"""
    key = (kind, name)
    if key not in _cache:
        inp = soft_case(name) if kind == "soft" else hard_case(name)
        _cache[key] = (inp,) + references(inp[0], inp[1], inp[2])
    return _cache[key]
