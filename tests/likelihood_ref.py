"""CPU restatements for the likelihood tests (tests/test_likelihood_cpu.py, tests/test_likelihood_gpu.py): the Rademacher
stream of the probe kernels, the augmented Heun recursion in fp64, and the exact eps . J eps of the oracle network."""
import math

import numpy as np
import torch

NLL_TAG = 0x4E4C0000        # ^ step; + (ev << 16) for the correction evaluation of a step
M32 = np.uint64(0xFFFFFFFF)


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


def philox_words(shape, seed, solve_index, tag):
    """word j % 4 of philox((j / 4, b, tag, solve_index), (seed_lo, seed_hi)) for element j of sample b: uint64 [B, CHW]"""
    B, CHW = shape[0], int(np.prod(shape[1:]))
    j = np.arange(CHW, dtype=np.uint64)
    b = np.arange(B, dtype=np.uint64)[:, None]
    r = philox4x32_10(j[None, :] // np.uint64(4) + 0 * b, b + 0 * j[None, :], tag, solve_index,
                      seed & 0xFFFFFFFF, seed >> 32)
    k = (j % np.uint64(4)).astype(np.int64)
    return np.take_along_axis(np.stack(r).transpose(1, 2, 0), k[None, :, None], axis=2)[..., 0]


def probe_signs(shape, seed, solve_index, step, ev=0, num_probes=1):
    """eps of the probes of evaluation ev (0 Euler, 1 correction) of step `step`: float32 [K, *shape] of +-1; bit p of
    the element's word clear = +1, set = -1"""
    w = philox_words(shape, seed, solve_index, (NLL_TAG + (ev << 16)) ^ step)
    eps = [1.0 - 2.0 * ((w >> np.uint64(p)) & np.uint64(1)).astype(np.float32) for p in range(num_probes)]
    return torch.from_numpy(np.stack(eps).reshape((num_probes,) + tuple(shape)).astype(np.float32))


def log_normal(x, var):
    """log N(x_b; 0, var I) per sample, fp64"""
    x = x.double().flatten(1)
    return -0.5 * x.shape[1] * math.log(2.0 * math.pi * var) - (x * x).sum(1) / (2.0 * var)


def nll_recursion(D, q, image, t, end=0):
    """The augmented Heun recursion of DeterministicSolver.log_likelihood in the dtype of `image` (fp64 for a reference).
    D(x, i): the denoiser at table entry i; q(x, i, step, ev): tr dD/dx (or its estimate) at x and table entry i, asked
    for evaluation ev of step `step`; t: the fp64 sigma table.  Returns (logp fp64 [B], unit-scale latent)."""
    x = image
    d = image[0].numel()
    L = torch.zeros(image.shape[0], dtype=torch.float64)
    for i in range(len(t) - 2, end, -1):
        t0, t1 = float(t[i]), float(t[i - 1])
        g0 = (d - q(x, i, i, 0).double()) / t0
        dx = (x - D(x, i)) / t0
        x1 = x + (t1 - t0) * dx
        g1 = (d - q(x1, i - 1, i, 1).double()) / t1
        x = x + (t1 - t0) * (0.5 * dx + 0.5 * (x1 - D(x1, i - 1)) / t1)
        L = L + (t1 - t0) * 0.5 * (g0 + g1)
    tk = float(t[end])
    return log_normal(x, tk * tk) + L, x / tk


def oracle_q(O, P, em, dm, x, sigma, labels, eps):
    """mean over the K probes eps [K, B, ...] of the exact eps . J eps of the oracle network at noise level sigma, fp64
    [B].  The jvp is the oracle's own arithmetic, fp32 (oracle.edm_oracle casts to fp32 inside its gates and its
    embedding, so it cannot be run in fp64): an analytic derivative at fp32 rounding, ~1e-6 relative, where a difference
    quotient at fp32 carries 1e-7 / delta; the products with eps and their sum are fp64."""
    sig = torch.full((x.shape[0],), float(sigma), dtype=torch.float32)

    def f(z):
        return O.edm_forward(P, em, dm, z, sig, labels).float()
    out = []
    for e in eps:
        _, jv = torch.autograd.functional.jvp(f, x.float(), e.float())
        out.append((e.double() * jv.double()).flatten(1).sum(1))
    return torch.stack(out).mean(0)
