"""CPU restatements for the input gradient of the denoiser and diffusion posterior sampling (DPS, Chung et al. 2023), in
whatever floating-point dtype their inputs have (fp64 for ground truth, fp32 for a rounding budget): conv_in's dgrad with
the preconditioning folded in, the zero-padded Gaussian blur, the adjoint of the averaging operator, the residual / norm /
update of a DPS step and the DPS Heun loop.  No GPU, no tinyedm_amd kernel."""
import math

import torch
import torch.nn.functional as F

import restoration_ref as R


# ------------------------------------------------------------------ conv_in's input gradient
def precond(sigma, sd):
    """(c_in, c_skip) as [B, 1, 1, 1] in sigma's dtype"""
    s = sigma.reshape(-1, 1, 1, 1)
    return 1.0 / (sd * sd + s * s).sqrt(), sd * sd / (s * s + sd * sd)


def conv_in_dgrad(gy, w, gD, sigma, sd):
    """gy [B, H, W, C0] (NHWC), w [C0, Cimg, 3, 3], gD [B, Cimg, H, W] or None ->
    (gx, mag): gx = c_in * dgrad3x3(gy; w) + c_skip * gD and mag = c_in * sum |gy * w| + c_skip * |gD|, the magnitude the
    rounding bound of an fp32 accumulation scales with"""
    c_in, c_skip = precond(sigma, sd)
    g = gy.permute(0, 3, 1, 2)
    gx = c_in * F.conv_transpose2d(g, w, padding=1)
    mag = c_in * F.conv_transpose2d(g.abs(), w.abs(), padding=1)
    if gD is not None:
        gx = gx + c_skip * gD
        mag = mag + c_skip * gD.abs()
    return gx, mag


# ------------------------------------------------------------------ operators
def gaussian_taps(std, radius):
    raw = [math.exp(-(k * k) / (2.0 * std * std)) for k in range(-radius, radius + 1)]
    tot = sum(raw)
    return [v / tot for v in raw]


def blur(x, taps):
    """separable zero-padded blur of every [H, W] plane of x [B, C, H, W]; symmetric taps: its own adjoint"""
    k = torch.tensor(list(taps), dtype=x.dtype)
    r = len(taps) // 2
    B, C, H, W = x.shape
    p = x.reshape(B * C, 1, H, W)
    p = F.conv2d(p, k.view(1, 1, 1, -1), padding=(0, r))
    p = F.conv2d(p, k.view(1, 1, -1, 1), padding=(r, 0))
    return p.reshape(B, C, H, W)


def degrade_adjoint(r, scale, gray, channels):
    """A^T r for the averaging A of restoration_ref.degrade: replicate and divide by the block size"""
    return R.pinv(r, scale, gray, channels) / R.block_terms(scale, gray, channels)


class Box:
    """(scale, gray) averaging operator"""

    def __init__(self, scale, gray):
        self.scale, self.gray = scale, gray

    def measure(self, x):
        return R.degrade(x, self.scale, self.gray)

    def adjoint(self, r, channels):
        return degrade_adjoint(r, self.scale, self.gray, channels)


class Blur:
    def __init__(self, std, radius, taps=None):
        self.taps = gaussian_taps(std, radius) if taps is None else list(taps)

    def measure(self, x):
        return blur(x, self.taps)

    def adjoint(self, r, channels=None):
        return blur(r, self.taps)


# ------------------------------------------------------------------ one DPS step's measurement side
def residual(y, AD):
    r = y - AD
    return r, r.flatten(1).norm(dim=1)


def update(x, g, nrm, scale):
    fac = torch.where(nrm > 0, scale / nrm.clamp_min(1e-300 if nrm.dtype == torch.float64 else 1e-38), torch.zeros_like(nrm))
    return x + fac.view(-1, 1, 1, 1) * g


# ------------------------------------------------------------------ the loop
def solve_dps(D_vjp, D, t, x0, op, y, scale, lift=None):
    """Algorithm 1 of Karras et al. 2022 with the DPS correction after every step:
    D_vjp(x, sigma) -> (D, pullback) for the Euler evaluation, D(x, sigma) for the Heun correction's;
    x_{i+1} = x' + (scale / ||r||) J^T A^T r, r = y - A D(x_i), x' the ordinary Heun step.  lift: the churn of Algorithm 2."""
    N = len(t) - 1
    x1 = t[0] * x0
    for i in range(N):
        x, t0, t1 = x1, t[i], t[i + 1]
        if lift is not None:
            x, t0 = lift(x, i)
        D0, pull = D_vjp(x, t0)
        r, nrm = residual(y, op.measure(D0))
        g = pull(op.adjoint(r, D0.shape[1]))
        dx = (x - D0) / t0
        x1 = x + (t1 - t0) * dx
        if i < N - 1:
            dxp = (x1 - D(x1, t1)) / t1
            x1 = x + (t1 - t0) * (0.5 * dx + 0.5 * dxp)
        x1 = update(x1, g, nrm, scale)
    return x1


def gaussian_vjp(x, s):
    """the exact denoiser of N(MU, SD^2 I) and its VJP: J = c I, c = SD^2 / (SD^2 + s^2)"""
    c = R.SD ** 2 / (R.SD ** 2 + s * s)
    return R.MU + c * (x - R.MU), (lambda v: c * v)


def autograd_vjp(fn):
    """D_vjp from a differentiable fn(x, sigma)"""
    def D_vjp(x, s):
        with torch.enable_grad():
            xr = x.detach().requires_grad_()
            out = fn(xr, s)
        return out.detach(), (lambda v: torch.autograd.grad(out, xr, v.to(out.dtype))[0])
    return D_vjp


# ------------------------------------------------------------------ the analytic cases shared by the CPU and GPU tests
ANALYTIC_STEPS = 18
ANALYTIC_SHAPE = (4, 3, 16, 16)
ANALYTIC_NOISE = 0.05           # std of the noise added to y
ANALYTIC_SEED = 5
# name -> (operator, dps_scale)
ANALYTIC_CASES = {"box": (("box", 2, False), 2.0), "gray": (("box", 1, True), 2.0), "blur": (("blur", 1.0, 2), 2.0)}


def analytic_operator(spec):
    return Box(spec[1], spec[2]) if spec[0] == "box" else Blur(spec[1], spec[2])


def analytic_inputs(spec, dtype=torch.float64):
    """(x0, y): unit noise and the noisy measurement of a draw from N(MU, SD^2 I)"""
    g = torch.Generator().manual_seed(ANALYTIC_SEED)
    x0 = torch.randn(ANALYTIC_SHAPE, generator=g, dtype=torch.float64)
    img = R.MU + R.SD * torch.randn(ANALYTIC_SHAPE, generator=g, dtype=torch.float64)
    y = analytic_operator(spec).measure(img)
    y = y + ANALYTIC_NOISE * torch.randn(y.shape, generator=g, dtype=torch.float64)
    return x0.to(dtype), y.to(dtype)
