"""Plain torch, CPU, fp64 references of the fp32 evaluation path's elementwise kernels (tinyedm_amd/csrc/eval_f32.hip) and
exact restatements of the split-bf16 pair format that the "f32x3" path carries its operands in.

Written from the header comments of that file and from oracle/edm_oracle.py (rms_div, mp_silu, scale_long_gate,
precond_scalars), not from the kernels' code; tests/test_evalf32_ref_cpu.py checks each of them against an independent
formulation.  Activations are (B, H, W, C) -- the kernels' layout -- except where a kernel's own interface is NCHW
(precond_in's input, conv_out's output, the layout changes).  Every argument is converted to fp64 on entry and no result is
rounded: the caller compares a kernel's fp32 output with the exact value.

The pair format is the one place where rounding IS the contract: an fp32 value x travels as two bf16 numbers,
hi = bf16(x) (round to nearest even) and lo = bf16(x - hi); x - hi is exact in fp32 and |hi + lo - x| <= 2^-17 |x| for
normal x.  `pairs_of` and `split_pack_ref` do that rounding with torch's CPU conversion, so a kernel can be held to them
bit for bit."""
import math

import numpy as np
import torch

SILU_DIV = 0.596
NORM_EPS = float(np.float32(1e-4))      # the kernels' constant is the fp32 value of 1e-4
F64 = torch.float64
PAIR_REL = 2.0 ** -17                   # |hi + lo - x| <= PAIR_REL |x|


def f64(t):
    return None if t is None else t.detach().to("cpu").to(F64)


# ------------------------------------------------------------------ mp_silu, pixel norm
def mp_silu(x):
    """x * sigmoid(x) / 0.596"""
    x = f64(x)
    return x * torch.sigmoid(x) / SILU_DIV


def pixelnorm(x):
    """xn = x / (eps + |x| / sqrt(C)), the norm over the channels of one pixel"""
    x = f64(x)
    C = x.shape[-1]
    return x / (NORM_EPS + x.square().sum(-1, keepdim=True).sqrt() / math.sqrt(C))


def pixelnorm_silu(x):
    """(xn, mp_silu(xn))"""
    xn = pixelnorm(x)
    return xn, mp_silu(xn)


# ------------------------------------------------------------------ 2x resampling and the fused forms
def pool2(x):
    """y[b,h,w,c] = mean of x[b, 2h:2h+2, 2w:2w+2, c]"""
    x = f64(x)
    return 0.25 * (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2])


def up2(x):
    """nearest-exact x2: y[b,h,w,c] = x[b,h//2,w//2,c]"""
    x = f64(x)
    B, H, W, C = x.shape
    return x[:, :, None, :, None, :].expand(B, H, 2, W, 2, C).reshape(B, 2 * H, 2 * W, C)


def pool_pixelnorm_silu(x):
    """(xn, s) of the 2x2 mean of x"""
    return pixelnorm_silu(pool2(x))


def up2_silu(x):
    """(y, mp_silu(y)), y = up2(x)"""
    y = up2(x)
    return y, mp_silu(y)


# ------------------------------------------------------------------ ScaleLong gate, concat
def skip_gate(skip, w1h, w2h):
    """gate (B, C) = sigmoid(W2 . mp_silu(W1 . [mean_hw(skip), 1])); w1h (R, C+1), w2h (C, R) are the effective weights"""
    skip = f64(skip)
    m = skip.mean(dim=(1, 2))
    m1 = torch.cat((m, torch.ones_like(m[:, :1])), dim=1)
    h = mp_silu(m1 @ f64(w1h).t())
    return torch.sigmoid(h @ f64(w2h).t())


def skip_half(skip, gate):
    """skip * gate[b, :]: the skip half of the concatenated operand"""
    return f64(skip) * f64(gate)[:, None, None, :]


def concat_gate(inp, skip, gate):
    """(cat, mp_silu(cat)), cat = [inp | skip * gate[b, :]]"""
    cat = torch.cat((f64(inp), skip_half(skip, gate)), dim=-1)
    return cat, mp_silu(cat)


# ------------------------------------------------------------------ preconditioning, conv_out
def precond_scalars(sigma, sd, B):
    """(c_skip, c_out, c_in), each (B,); sigma has B elements or one"""
    s = f64(sigma).reshape(-1)
    s = s.expand(B) if s.numel() == 1 else s.reshape(B)
    den = s * s + sd * sd
    return sd * sd / den, s * sd / den.sqrt(), 1.0 / den.sqrt()


def precond_in(noisy, sigma, sd, CP):
    """noisy (B,Cimg,H,W) -> (B,H,W,CP): channels [c_in * noisy, 1, 0 ...]"""
    noisy = f64(noisy)
    B, Cimg, H, W = noisy.shape
    c_in = precond_scalars(sigma, sd, B)[2]
    out = torch.zeros(B, H, W, CP, dtype=F64)
    out[..., :Cimg] = (noisy * c_in[:, None, None, None]).permute(0, 2, 3, 1)
    out[..., Cimg] = 1.0
    return out


def conv_out(x, w_hat, gain, noisy, sigma, sd):
    """D (B,Co,H,W) = (sum_c x[b,h,w,c] wh[o,c]) * gain * c_out(b) + noisy * c_skip(b)"""
    x = f64(x)
    c_skip, c_out, _ = precond_scalars(sigma, sd, x.shape[0])
    Fr = torch.einsum("bhwc,oc->bohw", x, f64(w_hat))
    return Fr * float(gain) * c_out[:, None, None, None] + f64(noisy) * c_skip[:, None, None, None]


# ------------------------------------------------------------------ layout
def nchw_to_nhwc(x):
    return f64(x).permute(0, 2, 3, 1).contiguous()


def nhwc_to_nchw(x):
    return f64(x).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------ the pair format
def pairs_of(x):
    """fp32 (..., C) -> bf16 (..., 2C) = [hi | lo]: hi = bf16(x), lo = bf16(x - hi), torch's CPU rounding (nearest even)"""
    x = x.detach().to("cpu")
    assert x.dtype == torch.float32
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.cat((hi, lo), dim=-1)


def split_pack_ref(w_hat, taps):
    """w_hat fp32 (Cout, I*taps), master order (element (o, i*taps + t)) -> bf16 (taps, Cout, 3*Ip) = [hi | lo | hi],
    Ip = I rounded up to 32, channels I..Ip-1 zero"""
    w_hat = w_hat.detach().to("cpu")
    assert w_hat.dtype == torch.float32 and w_hat.dim() == 2 and w_hat.shape[1] % taps == 0
    Cout, I = w_hat.shape[0], w_hat.shape[1] // taps
    Ip = (I + 31) // 32 * 32
    w = w_hat.view(Cout, I, taps).permute(2, 0, 1)                      # (taps, Cout, I)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    pk = torch.zeros(taps, Cout, 3 * Ip, dtype=torch.bfloat16)
    pk[..., :I] = hi
    pk[..., Ip:Ip + I] = lo
    pk[..., 2 * Ip:2 * Ip + I] = hi
    return pk


def halves(pairs):
    """(hi, lo) of a [hi | lo] row, both fp64"""
    C = pairs.shape[-1] // 2
    p = f64(pairs.float())
    return p[..., :C], p[..., C:]


def value_of(pairs):
    """the value a pair stands for: hi + lo in fp64"""
    hi, lo = halves(pairs)
    return hi + lo


def half_ulp_bf16(hi):
    """half a bf16 ulp (8 significant bits) of each fp64 element of `hi`; 0 where hi == 0"""
    _, e = torch.frexp(hi)                                              # |hi| = m 2^e, m in [0.5, 1): ulp = 2^(e - 8)
    return torch.where(hi == 0, torch.zeros_like(hi), torch.ldexp(torch.ones_like(hi), e - 9))


# ------------------------------------------------------------------ the kernels' expressions restated in numpy float32
# Used only to MEASURE how far an fp32 evaluation of the documented expression lies from the fp64 reference where the
# expression passes through the native exponential (tests/test_evalf32_edges_gpu.py: "measured allowances").
def _f32(x):
    return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float32)


def expf_native32(x):
    """__expf(x) = exp2(x * log2 e), the scaled argument rounded to fp32"""
    return np.exp2(_f32(x) * np.float32(1.4426950408889634))


def sigmoid32(x):
    x = _f32(x)
    return np.float32(1) / (np.float32(1) + expf_native32(-x))


def mp_silu32(x):
    """x * (1 / (1 + __expf(-x))) * (1 / 0.596f), every step rounded to fp32"""
    x = _f32(x)
    return x * sigmoid32(x) * (np.float32(1) / np.float32(SILU_DIV))


def skip_gate32(skip, w1h, w2h):
    """the gate with every sum, product and function in fp32 (numpy's summation order)"""
    skip, w1h, w2h = _f32(skip), _f32(w1h), _f32(w2h)
    B, H, W, C = skip.shape
    m = skip.reshape(B, H * W, C).sum(axis=1, dtype=np.float32) / np.float32(H * W)
    m1 = np.concatenate((m, np.ones((B, 1), np.float32)), axis=1)
    h = mp_silu32(m1 @ w1h.T)
    return sigmoid32(h @ w2h.T)


def mp_silu_grad(x):
    """d/dx mp_silu"""
    x = f64(x)
    s = torch.sigmoid(x)
    return s * (1.0 + x * (1.0 - s)) / SILU_DIV
