"""tests/evalf32_ref.py against independent formulations (torch.nn.functional and torch.linalg in fp64, the oracle) on small
random inputs, and the pair-format restatement against the definition of round-to-nearest-even on chosen bit patterns: the
references that tests/test_evalf32_edges_gpu.py holds the HIP kernels to do not rest on the code under test.

Where the oracle forms an intermediate in fp32 (rms_div's norm, the gate MLP, precond_scalars) the fp64 formulation with
torch.nn.functional is the 1e-12 check and the oracle is compared at its own precision, 1e-6."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import evalf32_ref as R
from oracle import edm_oracle as O

D = torch.float64
bf16 = torch.bfloat16


def gen(seed):
    return torch.Generator().manual_seed(seed)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * (1.0 + b.abs().max().item()), (a - b).abs().max().item()


def bits(words):
    """fp32 tensor from 32-bit patterns"""
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


def hi_bits(t):
    """upper 16 bits of the fp32 form of a bf16 tensor"""
    return (t.float().numpy().view(np.uint32) >> 16).tolist()


# ---------------------------------------------------------------------------------------------- fp64 restatements
def test_mp_silu():
    x = torch.randn(4, 3, 5, 16, generator=gen(1), dtype=D) * 3
    close(R.mp_silu(x), O.mp_silu(x))
    close(R.mp_silu(x), F.silu(x) / 0.596)
    xr = x.clone().requires_grad_(True)
    (F.silu(xr) / 0.596).sum().backward()
    close(R.mp_silu_grad(x), xr.grad)


@pytest.mark.parametrize("C", [4, 260, 1028])
def test_pixelnorm_silu(C):
    x = torch.randn(2, 3, 5, C, generator=gen(C), dtype=D) * 2
    xn, s = R.pixelnorm_silu(x)
    want = x / (R.NORM_EPS + torch.linalg.vector_norm(x, dim=-1, keepdim=True) / math.sqrt(C))
    close(xn, want)
    close(s, F.silu(want) / 0.596)
    close(nchw(xn), O.rms_div(nchw(x), [1]), 1e-6)                 # the oracle forms the norm in fp32
    z = torch.zeros(1, 1, 1, C, dtype=D)                           # the zero row: 0 / eps
    assert torch.equal(R.pixelnorm(z), z)


@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 4), (3, 6, 10, 8), (2, 14, 4, 12)])
def test_resampling_and_fused_forms(B, H, W, C):
    g = gen(H * W + C)
    x = torch.randn(B, H, W, C, generator=g, dtype=D)
    pooled = nhwc(F.avg_pool2d(nchw(x), 2, 2))
    close(R.pool2(x), pooled)
    up = nhwc(F.interpolate(nchw(x), scale_factor=2, mode="nearest-exact"))
    assert torch.equal(R.up2(x), up)
    xn, s = R.pool_pixelnorm_silu(x)
    want = pooled / (R.NORM_EPS + torch.linalg.vector_norm(pooled, dim=-1, keepdim=True) / math.sqrt(C))
    close(xn, want)
    close(s, F.silu(want) / 0.596)
    y, sy = R.up2_silu(x)
    assert torch.equal(y, up)
    close(sy, F.silu(up) / 0.596)


@pytest.mark.parametrize("C,R_,HW", [(4, 1, (1, 1)), (40, 2, (3, 1)), (128, 8, (7, 7))])
def test_skip_gate_and_concat(C, R_, HW):
    g = gen(C + R_)
    B, (H, W), Ci = 3, HW, 8
    P = {"l.layer1.weight": torch.randn(R_, C + 1, 1, 1, generator=g), "l.layer2.weight": torch.randn(C, R_, 1, 1, generator=g)}
    w1 = O.effective_weight(P["l.layer1.weight"]).to(D)
    w2 = O.effective_weight(P["l.layer2.weight"]).to(D)
    skip = torch.randn(B, H, W, C, generator=g, dtype=D)
    gate = R.skip_gate(skip, w1.view(R_, C + 1), w2.view(C, R_))
    # networks.py:112-118 with torch.nn.functional in fp64
    m = nchw(skip).mean(dim=(2, 3), keepdim=True)
    m = torch.cat((m, torch.ones_like(m[:, :1])), dim=1)
    want = torch.sigmoid(F.conv2d(F.silu(F.conv2d(m, w1)) / 0.596, w2)).view(B, C)
    close(gate, want)
    close(gate, O.scale_long_gate(P, "l.", nchw(skip)).view(B, C).to(D), 1e-6)      # (the oracle keeps this MLP in fp32)
    inp = torch.randn(B, H, W, Ci, generator=g, dtype=D)
    cat, sil = R.concat_gate(inp, skip, gate)
    want_cat = nhwc(torch.cat((nchw(inp), nchw(skip) * want.view(B, C, 1, 1)), dim=1))
    close(cat, want_cat)
    close(sil, F.silu(want_cat) / 0.596)
    assert torch.equal(cat[..., :Ci], inp) and torch.equal(cat[..., Ci:], R.skip_half(skip, gate))


@pytest.mark.parametrize("Cimg,nsig", [(1, 3), (3, 1), (4, 3)])
def test_precond_and_conv_out(Cimg, nsig):
    g = gen(13 + Cimg)
    B, H, W, C, CP, sd = 3, 5, 7, 16, 8, 0.5
    noisy = torch.randn(B, Cimg, H, W, generator=g, dtype=D)
    sigma = torch.randn(nsig, generator=g, dtype=D).exp()
    s = (sigma.expand(B) if nsig == 1 else sigma).view(B, 1, 1, 1)
    c_skip, c_out, c_in = sd ** 2 / (s ** 2 + sd ** 2), s * sd / (s ** 2 + sd ** 2).sqrt(), 1 / (sd ** 2 + s ** 2).sqrt()
    for got, want in zip(R.precond_scalars(sigma, sd, B), (c_skip, c_out, c_in)):
        close(got, want.view(B))
    for got, want in zip(R.precond_scalars(sigma, sd, B), O.precond_scalars(s.view(B), sd)):
        close(got, want.view(B).to(D), 1e-6)                       # the oracle's scalars are fp32
    out = R.precond_in(noisy, sigma, sd, CP)
    close(nchw(out)[:, :Cimg], c_in * noisy)
    assert (out[..., Cimg] == 1).all() and (out[..., Cimg + 1:] == 0).all() and out.shape == (B, H, W, CP)
    x = torch.randn(B, H, W, C, generator=g, dtype=D)
    wh = torch.randn(Cimg, C, generator=g, dtype=D)
    want = F.conv2d(nchw(x), wh[:, :, None, None]) * 0.7 * c_out + noisy * c_skip
    close(R.conv_out(x, wh, 0.7, noisy, sigma, sd), want)


def test_layout():
    x = torch.randn(2, 3, 5, 9, generator=gen(14), dtype=D)
    y = R.nchw_to_nhwc(x)
    assert y.shape == (2, 5, 9, 3) and y.is_contiguous() and y[1, 2, 3, 1] == x[1, 1, 2, 3]
    assert torch.equal(R.nhwc_to_nchw(y), x)


# ---------------------------------------------------------------------------------------------- the pair format
def test_bf16_conversion_rounds_ties_to_even():
    """low half 0x8000 under an even / an odd upper mantissa bit, both signs; one fp32 ulp either side of the tie"""
    x = bits([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF])
    assert hi_bits(x.to(bf16)) == [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x3F82, 0x3F81]
    p = R.pairs_of(x.view(1, -1))
    assert hi_bits(p[0, :8]) == [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x3F82, 0x3F81]
    # lo of a tie is +-2^-8 exactly, taken from the hi that was stored (a lo from a truncated hi would be +2^-8 everywhere)
    assert p[0, 8:12].float().tolist() == [2.0 ** -8, -(2.0 ** -8), -(2.0 ** -8), 2.0 ** -8]
    z = R.pairs_of(bits([0x00000000, 0x80000000]).view(1, -1))
    assert hi_bits(z[0]) == [0x0000, 0x8000, 0x0000, 0x0000]       # -0 keeps its sign in hi; lo = (-0) - (-0) = +0


def _many_binades(n_per=8192):
    g = gen(21)
    e = torch.arange(-60, 60, dtype=torch.float32)                  # 120 binades
    m = 1.0 + torch.rand(120, n_per, generator=g)
    sgn = torch.where(torch.rand(120, n_per, generator=g) < 0.5, -1.0, 1.0)
    return (sgn * m * torch.exp2(e)[:, None]).reshape(-1)           # ~2^20 normal values


def test_pairs_residual_is_exact_and_pair_is_within_2_pow_minus_17():
    x = _many_binades()
    hi = x.to(bf16).float()
    assert torch.equal((x - hi).double(), x.double() - hi.double())                 # x - hi is exact in fp32
    p = R.pairs_of(x.view(-1, 8))
    v = R.value_of(p).reshape(-1)
    err = ((v - x.double()).abs() / x.double().abs()).max().item()
    print(f"worst |hi + lo - x| / |x| over {x.numel()} values: {err:.3e} (2^-17 = {2.0 ** -17:.3e})")
    assert err <= R.PAIR_REL
    h, lo = R.halves(p)
    # hi is a bf16 nearest to hi + lo (lo rounds up to exactly half an ulp next to a tie, so "<=", not a re-rounding)
    assert (lo.abs() <= R.half_ulp_bf16(h)).all()


def test_half_ulp_bf16():
    h = torch.tensor([1.0, 1.9921875, 2.0, -0.75, 0.0, 2.0 ** -100], dtype=D)
    assert R.half_ulp_bf16(h).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 0.0, 2.0 ** -108]


@pytest.mark.parametrize("I,taps,Cout", [(4, 1, 3), (40, 9, 3), (32, 9, 2)])
def test_split_pack_ref_layout(I, taps, Cout):
    w = torch.randn(Cout, I * taps, generator=gen(I + taps))
    pk = R.split_pack_ref(w, taps)
    Ip = (I + 31) // 32 * 32
    assert pk.shape == (taps, Cout, 3 * Ip) and pk.dtype == bf16
    for t in range(taps):
        for o in range(Cout):
            for i in range(Ip):
                v = w[o, i * taps + t] if i < I else torch.tensor(0.0)
                h = v.to(bf16)
                l = (v - h.float()).to(bf16)
                assert pk[t, o, i] == h and pk[t, o, Ip + i] == l and pk[t, o, 2 * Ip + i] == h


def test_fp32_restatements_are_fp32_evaluations_of_the_references():
    """the numpy float32 restatements used to measure allowances: a few ulps from the fp64 references"""
    g = gen(33)
    x = (torch.rand(4096, generator=g) * 16 - 8)
    e = np.abs(R.mp_silu32(x).astype(np.float64) - R.mp_silu(x).numpy())
    assert (e <= 32 * 2.0 ** -24 * np.abs(R.mp_silu(x).numpy())).all()
    skip = torch.randn(2, 3, 5, 40, generator=g)
    w1, w2 = torch.randn(2, 41, generator=g) / 6, torch.randn(40, 2, generator=g)
    ref = R.skip_gate(skip, w1, w2).numpy()
    assert np.abs(R.skip_gate32(skip, w1, w2) - ref).max() <= 1e-6
