"""CPU reference of zero-shot restoration (DDNM), in whatever floating-point dtype its inputs have (fp64 for the
tests' ground truth, fp32 for the rounding budget): the measurement operator A (block mean, optionally the mean over the
channels), its pseudo-inverse A+ (replication), the projection D + A+ (y - A D), and the projected Heun / stochastic /
multistep solves, composed from the solvers' own update formulas.  No GPU, no tinyedm_amd kernel."""
import torch

OPERATORS = [(2, False), (4, False), (1, True), (4, True), (8, True)]       # (scale, gray)


def block_terms(scale, gray, channels):
    """n: the number of terms of one block mean"""
    return scale * scale * (channels if gray else 1)


def degrade(x, scale, gray):
    """A x: [B, C, H, W] -> [B, 1 if gray else C, H/scale, W/scale]"""
    B, C, H, W = x.shape
    y = x.reshape(B, C, H // scale, scale, W // scale, scale).mean(dim=(3, 5))
    return y.mean(dim=1, keepdim=True) if gray else y


def pinv(y, scale, gray, channels):
    """A+ y: every value replicated to its block (and to all channels when gray)"""
    x = y.repeat_interleave(scale, dim=2).repeat_interleave(scale, dim=3)
    return x.expand(-1, channels, -1, -1).clone() if gray else x


def project(D, y, scale, gray):
    """D + A+ (y - A D)"""
    return D + pinv(y - degrade(D, scale, gray), scale, gray, D.shape[1])


def projector(y, scale, gray):
    """proj(D) of one measurement, or the identity for y = None (the plain solve)"""
    if y is None:
        return lambda D: D
    return lambda D: project(D, y, scale, gray)


def solve_heun(D, t, x0, proj=lambda d: d, start=0, image=None, lift=None):
    """Algorithm 1 of Karras et al. 2022 on the table t (t[N] = 0) with every evaluation D(x, sigma) passed through
    proj; entered at t[start] from image + t[start] * x0.  lift(x, i) -> (x_hat, t_hat) is the churn of Algorithm 2."""
    N = len(t) - 1
    x1 = t[start] * x0 if image is None else image + t[start] * x0
    for i in range(start, N):
        x, t0, t1 = x1, t[i], t[i + 1]
        if lift is not None:
            x, t0 = lift(x, i)
        dx = (x - proj(D(x, t0))) / t0
        x1 = x + (t1 - t0) * dx
        if i < N - 1:
            dxp = (x1 - proj(D(x1, t1))) / t1
            x1 = x + (t1 - t0) * (0.5 * dx + 0.5 * dxp)
    return x1


def solve_multistep(D, t, coeffs, x0, proj=lambda d: d, start=0, image=None):
    """DPM-Solver++ multistep with the rows (a, c0, c1, c2) of MultistepSolver.multistep_coefficients(start); the history
    holds the projected evaluations"""
    x = t[start] * x0 if image is None else image + t[start] * x0
    hist = []
    for i, (a, c0, c1, c2) in enumerate(coeffs):
        if i < start:
            continue
        m = proj(D(x, t[i]))
        x = a * x + c0 * m
        if c1 != 0.0:
            x = x + c1 * hist[-1]
        if c2 != 0.0:
            x = x + c2 * hist[-2]
        hist.append(m)
    return x


MU, SD = 0.3, 0.5


def gaussian(x, s):
    """the exact denoiser of N(MU, SD^2 I): an isotropic affine map, so it commutes with every projector A+ A"""
    return MU + SD ** 2 / (SD ** 2 + s * s) * (x - MU)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()
