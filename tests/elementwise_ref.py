"""Plain torch, CPU, fp64 references of the bf16 elementwise / norm / boundary kernels (tinyedm_amd/csrc/elementwise.hip).

Written from the formulas in that file's comments and from oracle/edm_oracle.py (rms_div, mp_silu, mp_add, precond_scalars,
scale_long_gate); tests/test_elementwise_ref_cpu.py checks each of them against an independent formulation.  Activations are
(B, H, W, C) -- the kernels' layout -- and every argument is converted to fp64 on entry.  Results are NOT rounded: the caller
compares a kernel's bf16 output with the exact value.  bf16 rounding (`bf`) appears only where the kernels' contract stores or
documents a bf16 intermediate:
  * xn before mp_silu (pixelnorm_silu: pass the stored xn to `mp_silu`),
  * the pooled row before the norm (pool_pixelnorm_silu_fwd),
  * skip * gate before mp_silu (concat_gate_fwd: pass the stored cat to `mp_silu`),
  * the pooled-resolution gradient before the 0.25 * upsample (pool_pixelnorm_silu_bwd).
"""
import math

import numpy as np
import torch

SILU_DIV = 0.596
NORM_EPS = float(np.float32(1e-4))      # the kernels' constant is the fp32 value of 1e-4
F64 = torch.float64


def f64(t):
    return None if t is None else t.detach().to("cpu").to(F64)


def bf(t):
    """round to bf16 (nearest even), back in fp64"""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


# ------------------------------------------------------------------ mp_silu
def mp_silu(x):
    x = f64(x)
    return x * torch.sigmoid(x) / SILU_DIV


def mp_silu_grad(x):
    x = f64(x)
    s = torch.sigmoid(x)
    return s * (1.0 + x * (1.0 - s)) / SILU_DIV


def silu_bwd(x, ga, gextra=None, extra_scale=1.0):
    """gx = mp_silu'(x) * ga + extra_scale * gextra"""
    gx = mp_silu_grad(x) * f64(ga)
    if gextra is not None:
        gx = gx + float(extra_scale) * f64(gextra)
    return gx


def axpby(a, alpha, b=None, beta=0.0):
    out = float(alpha) * f64(a)
    if b is not None:
        out = out + float(beta) * f64(b)
    return out


# ------------------------------------------------------------------ pixel norm (+ mp_silu)
def pixelnorm_fwd(x):
    """(xn, d): d = eps + ||x|| / sqrt(C) per pixel (B*H*W,), xn = x / d (exact; the kernel stores bf(xn) and
    a = mp_silu(of the stored xn))"""
    x = f64(x)
    C = x.shape[-1]
    d = NORM_EPS + x.square().sum(-1).sqrt() / math.sqrt(C)
    return x / d[..., None], d.reshape(-1)


def pixelnorm_bwd(xn, d, gxn, gxn_scale, ga, gadd=None):
    """closed form: g = gs * gxn + mp_silu'(xn) * ga ; s = d - eps ; coef = <g, xn> d / (C s) (0 where s == 0: the zero
    row, gx = g / eps there) ; gx = (g - xn coef) / d (+ gadd).  xn and d are the saved forward results."""
    xn = f64(xn)
    C = xn.shape[-1]
    d = f64(d).reshape(xn.shape[:-1])[..., None]
    g = torch.zeros_like(xn)
    if gxn is not None:
        g = g + float(gxn_scale) * f64(gxn)
    if ga is not None:
        g = g + mp_silu_grad(xn) * f64(ga)
    s = d - NORM_EPS
    dot = (g * xn).sum(-1, keepdim=True)
    coef = torch.where(s > 0, dot * d / (C * torch.where(s > 0, s, torch.ones_like(s))), torch.zeros_like(s))
    gx = (g - xn * coef) / d
    if gadd is not None:
        gx = gx + f64(gadd)
    return gx


# ------------------------------------------------------------------ 2x resampling
def pool2(x, scale=0.25):
    """y[b,h,w,c] = scale * sum_{i,j<2} x[b,2h+i,2w+j,c]"""
    x = f64(x)
    return float(scale) * (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2])


def up2(x, scale=1.0, add=None):
    """y[b,h,w,c] = scale * x[b,h//2,w//2,c] (+ add)"""
    x = f64(x)
    B, H, W, C = x.shape
    y = float(scale) * x[:, :, None, :, None, :].expand(B, H, 2, W, 2, C).reshape(B, 2 * H, 2 * W, C)
    if add is not None:
        y = y + f64(add)
    return y


def pool_pixelnorm_fwd(x):
    """pixelnorm_fwd of the bf16-rounded 2x2 mean of x"""
    return pixelnorm_fwd(bf(pool2(x, 0.25)))


def pool_pixelnorm_bwd(xn, d, gxn, gxn_scale, ga, gadd=None):
    """0.25 * upsample of the bf16-rounded pooled-resolution gradient (+ gadd at the resolution before the pool)"""
    return up2(bf(pixelnorm_bwd(xn, d, gxn, gxn_scale, ga)), 0.25, gadd)


# ------------------------------------------------------------------ modulation + mp_silu + dropout
def dropout_scale(pdrop):
    """the kernels compare 16 random bits with round(p * 65536) and rescale by the same quantised p"""
    if pdrop <= 0:
        return 1.0
    thr = int(np.float32(pdrop) * np.float32(65536.0) + np.float32(0.5))
    return 65536.0 / (65536 - thr)


def mod_silu_drop_fwd(r, lin, gain, keep, pdrop):
    """a = keep * scale * mp_silu(r * (lin * gain + 1));  r, keep (B,H,W,C), lin (B,C), gain scalar"""
    r = f64(r)
    m = (f64(lin) * float(gain) + 1.0)[:, None, None, :]
    return mp_silu(r * m) * f64(keep) * dropout_scale(pdrop)


def mod_silu_drop_bwd(r, lin, gain, ga, keep, pdrop):
    """(gr, gm, glin, ggain): gu = ga keep scale mp_silu'(r m) ; gr = gu m ; gm[b,c] = sum_hw gu r ; glin = gm gain ;
    ggain = sum gm lin"""
    r, lin = f64(r), f64(lin)
    m = (lin * float(gain) + 1.0)[:, None, None, :]
    gu = f64(ga) * f64(keep) * dropout_scale(pdrop) * mp_silu_grad(r * m)
    gm = (gu * r).sum(dim=(1, 2))
    return gu * m, gm, gm * float(gain), (gm * lin).sum()


# ------------------------------------------------------------------ reduce_hw, concat / gate
def reduce_hw(x, C=None, c_off=0, y=None, scale=1.0):
    """out[b,c] = scale * sum_hw x[b,hw,c_off+c] (* y[b,hw,c])"""
    x = f64(x)
    C = x.shape[-1] - c_off if C is None else C
    t = x[..., c_off:c_off + C]
    if y is not None:
        t = t * f64(y)[..., :C]
    return float(scale) * t.sum(dim=(1, 2))


def concat_gate_fwd(inp, skip, gate):
    """cat = [inp | skip * gate[b,:]] (exact; the kernel stores bf(skip * gate) and sil = mp_silu(of the stored cat))"""
    return torch.cat((f64(inp), f64(skip) * f64(gate)[:, None, None, :]), dim=-1)


def concat_gate_bwd(gcat, gate, gmean, Ci):
    """ginp = gcat[..., :Ci] ; gskip = gcat[..., Ci:] * gate + gmean / HW"""
    gcat = f64(gcat)
    HW = gcat.shape[1] * gcat.shape[2]
    return gcat[..., :Ci], gcat[..., Ci:] * f64(gate)[:, None, None, :] + f64(gmean)[:, None, None, :] / HW


# ------------------------------------------------------------------ preconditioning, conv_out
def precond_scalars(sigma, sd, B):
    """(c_skip, c_out, c_in), each (B,); sigma has B elements or one"""
    s = f64(sigma).reshape(-1).expand(B) if f64(sigma).numel() == 1 else f64(sigma).reshape(B)
    den = s * s + sd * sd
    return sd * sd / den, s * sd / den.sqrt(), 1.0 / den.sqrt()


def precond_in(noisy, sigma, sd, CP):
    """noisy (B,Cimg,H,W) -> (B,H,W,CP): [c_in * noisy, 1, 0 ...]"""
    noisy = f64(noisy)
    B, Cimg, H, W = noisy.shape
    c_in = precond_scalars(sigma, sd, B)[2]
    out = torch.zeros(B, H, W, CP, dtype=F64)
    out[..., :Cimg] = (noisy * c_in[:, None, None, None]).permute(0, 2, 3, 1)
    out[..., Cimg] = 1.0
    return out


def conv_out_fwd(x, w_hat, gain, noisy, sigma, sd):
    """(D, Fraw), both (B,Co,H,W): F[b,o,h,w] = sum_c x[b,h,w,c] wh[o,c] ; D = F gain c_out + noisy c_skip"""
    x = f64(x)
    B = x.shape[0]
    c_skip, c_out, _ = precond_scalars(sigma, sd, B)
    Fr = torch.einsum("bhwc,oc->bohw", x, f64(w_hat))
    return Fr * float(gain) * c_out[:, None, None, None] + f64(noisy) * c_skip[:, None, None, None], Fr


def conv_out_bwd(x, w_hat, gain, Fraw, dD, sigma, sd):
    """(gx, gw_hat, ggain): dF = dD c_out gain ; gx = dF . wh ; gw_hat[o,c] = sum dF x ; ggain = sum dD c_out F"""
    x, dD = f64(x), f64(dD)
    c_out = precond_scalars(sigma, sd, x.shape[0])[1][:, None, None, None]
    dF = dD * c_out * float(gain)
    return (torch.einsum("bohw,oc->bhwc", dF, f64(w_hat)), torch.einsum("bohw,bhwc->oc", dF, x),
            (dD * c_out * f64(Fraw)).sum())


# ------------------------------------------------------------------ layout
def nchw_to_nhwc(x):
    return f64(x).permute(0, 2, 3, 1).contiguous()


def nhwc_to_nchw(x):
    return f64(x).permute(0, 3, 1, 2).contiguous()
