"""tests/elementwise_ref.py against independent formulations (the oracle, torch.nn.functional, fp64 autograd) on small
random inputs: the reference that tests/test_elementwise_edges_gpu.py holds the HIP kernels to does not rest on the code
under test."""
import math

import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as R
from oracle import edm_oracle as O

D = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * (1.0 + b.abs().max().item()), (a - b).abs().max().item()


def test_bf_rounds_to_nearest_even():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.0, 1e-30, 0.0], dtype=D)
    assert torch.equal(R.bf(x), torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, -3.0, float(torch.tensor(1e-30).bfloat16()), 0.0], dtype=D))


def test_mp_silu_and_grad():
    x = torch.randn(4, 3, 5, 16, generator=gen(1), dtype=D) * 3
    close(R.mp_silu(x), O.mp_silu(x))
    xr = x.clone().requires_grad_(True)
    ga = torch.randn(x.shape, generator=gen(2), dtype=D)
    O.mp_silu(xr).backward(ga)
    close(R.mp_silu_grad(x) * ga, xr.grad)
    ge = torch.randn(x.shape, generator=gen(3), dtype=D)
    close(R.silu_bwd(x, ga, ge, 0.7), xr.grad + 0.7 * ge)
    close(R.silu_bwd(x, ga), xr.grad)


def test_axpby_is_mp_add():
    a, b = torch.randn(2, 40, generator=gen(4), dtype=D), torch.randn(2, 40, generator=gen(5), dtype=D)
    t = 0.3
    c = math.sqrt((1 - t) ** 2 + t ** 2)
    close(R.axpby(a, (1 - t) / c, b, t / c), O.mp_add(a, b, t))
    close(R.axpby(a, 1.7), 1.7 * a)


@pytest.mark.parametrize("C", [8, 24, 136])
def test_pixelnorm_forward_and_closed_form_backward(C):
    g = gen(C)
    x = torch.randn(2, 3, 5, C, generator=g, dtype=D) * 2
    xn, d = R.pixelnorm_fwd(x)
    # the oracle forms the norm in fp32: 1e-6
    close(nchw(xn), O.rms_div(nchw(x), [1]), 1e-6)
    nrm = torch.linalg.vector_norm(x, dim=-1)
    close(d, (R.NORM_EPS + nrm / math.sqrt(C)).reshape(-1))
    # closed-form backward == fp64 autograd through x / (eps + ||x|| / sqrt(C)) and mp_silu, every None combination
    gxn, ga, gadd = (torch.randn(x.shape, generator=g, dtype=D) for _ in range(3))
    for use_gxn, use_ga, use_add in [(1, 1, 1), (1, 1, 0), (1, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0)]:
        xr = x.clone().requires_grad_(True)
        y = xr / (R.NORM_EPS + torch.linalg.vector_norm(xr, dim=-1, keepdim=True) / math.sqrt(C))
        loss = 0.0
        if use_gxn:
            loss = loss + 0.8 * (y * gxn).sum()
        if use_ga:
            loss = loss + (F.silu(y) / 0.596 * ga).sum()
        loss.backward()
        want = xr.grad + (gadd if use_add else 0)
        got = R.pixelnorm_bwd(xn, d, gxn if use_gxn else None, 0.8, ga if use_ga else None, gadd if use_add else None)
        close(got, want, 1e-10)


def test_pixelnorm_backward_degenerate_rows():
    g = gen(7)
    x = torch.randn(1, 1, 4, 16, generator=g, dtype=D)
    x[0, 0, 1] = 0
    x[0, 0, 2] *= 2.0 ** -60
    x[0, 0, 3] *= 2.0 ** 30
    xn, d = R.pixelnorm_fwd(x)
    assert d[1].item() == R.NORM_EPS and torch.isfinite(xn).all()
    gxn, ga = torch.randn(x.shape, generator=g, dtype=D), torch.randn(x.shape, generator=g, dtype=D)
    gx = R.pixelnorm_bwd(xn, d, gxn, 0.8, ga)
    assert torch.isfinite(gx).all()
    close(gx[0, 0, 1], (0.8 * gxn[0, 0, 1] + ga[0, 0, 1] * 0.5 / 0.596) / R.NORM_EPS)      # zero row: g / eps, mp_silu'(0) = 0.5 / 0.596
    xr = x.clone().requires_grad_(True)
    y = xr / (R.NORM_EPS + torch.linalg.vector_norm(xr, dim=-1, keepdim=True) / 4.0)
    (0.8 * (y * gxn).sum() + (F.silu(y) / 0.596 * ga).sum()).backward()
    for row in (0, 2, 3):                                          # autograd is defined (and agrees) off the zero row
        close(gx[0, 0, row], xr.grad[0, 0, row], 1e-9)


@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 8), (3, 6, 10, 24), (2, 14, 4, 8), (2, 4, 14, 16)])
def test_resampling(B, H, W, C):
    g = gen(H * W + C)
    x = torch.randn(B, H, W, C, generator=g, dtype=D)
    close(R.pool2(x), nhwc(F.avg_pool2d(nchw(x), 2, 2)))
    close(R.pool2(x, 0.7), 2.8 * nhwc(F.avg_pool2d(nchw(x), 2, 2)))
    up = nhwc(F.interpolate(nchw(x), scale_factor=2, mode="nearest-exact"))
    assert torch.equal(R.up2(x), up)
    add = torch.randn(B, 2 * H, 2 * W, C, generator=g, dtype=D)
    close(R.up2(x, 0.25, add), 0.25 * up + add)
    # pooled pixel norm: the norm of the bf16-rounded pooled tensor; its backward: the pooled-resolution gradient, rounded,
    # spread over the four source pixels with weight 0.25
    xn, d = R.pool_pixelnorm_fwd(x)
    xn2, d2 = R.pixelnorm_fwd(R.bf(nhwc(F.avg_pool2d(nchw(x), 2, 2))))
    close(xn, xn2)
    close(d, d2)
    gxn, ga = (torch.randn(xn.shape, generator=g, dtype=D) for _ in range(2))
    gx = R.pool_pixelnorm_bwd(xn, d, gxn, 0.8, ga, x)
    gp = R.bf(R.pixelnorm_bwd(xn, d, gxn, 0.8, ga))
    close(gx, 0.25 * nhwc(F.interpolate(nchw(gp), scale_factor=2, mode="nearest-exact")) + x)
    # 0.25 * upsample is the adjoint of the 2x2 mean
    t = torch.randn(B, H, W, C, generator=g, dtype=D)
    u = torch.randn(B, H // 2, W // 2, C, generator=g, dtype=D)
    close((R.pool2(t) * u).sum(), (t * R.up2(u, 0.25)).sum())


@pytest.mark.parametrize("pdrop", [0.0, 0.13])
def test_modulation(pdrop):
    g = gen(11)
    B, H, W, C = 3, 4, 5, 16
    r = torch.randn(B, H, W, C, generator=g, dtype=D)
    lin = torch.randn(B, C, generator=g, dtype=D) * 0.3
    gain = 0.9
    keep = (torch.rand(B, H, W, C, generator=g) >= pdrop).to(D)
    ga = torch.randn(B, H, W, C, generator=g, dtype=D)
    scale = R.dropout_scale(pdrop)
    assert abs(scale - 1 / (1 - pdrop)) < 1e-4 and (pdrop > 0 or scale == 1.0)
    rr, ll, gg = r.clone().requires_grad_(True), lin.clone().requires_grad_(True), torch.tensor(gain, dtype=D, requires_grad=True)
    ref = O.mp_silu(rr * (ll * gg + 1)[:, None, None, :]) * keep * scale
    ref.backward(ga)
    close(R.mod_silu_drop_fwd(r, lin, gain, keep, pdrop), ref.detach())
    gr, gm, glin, ggain = R.mod_silu_drop_bwd(r, lin, gain, ga, keep, pdrop)
    close(gr, rr.grad)
    close(glin, ll.grad)
    close(ggain, gg.grad)
    close(gm * gain, ll.grad)


def test_reduce_and_concat_gate():
    g = gen(12)
    B, H, W, Ci, Cs = 2, 3, 5, 16, 24
    x = torch.randn(B, H, W, Ci + Cs, generator=g, dtype=D)
    y = torch.randn(B, H, W, Cs + 8, generator=g, dtype=D)
    close(R.reduce_hw(x, scale=1 / 15), nhwc(nchw(x).mean(dim=(2, 3), keepdim=True)).reshape(B, -1))
    close(R.reduce_hw(x, C=16, c_off=8, y=y, scale=0.5),
          0.5 * torch.einsum("bhwc,bhwc->bc", x[..., 8:24], y[..., :16]))
    # gate from the oracle's ScaleLong MLP; concat and its backward against autograd
    P = {"l.layer1.weight": torch.randn(2, Cs + 1, 1, 1, generator=g),        # (the oracle keeps this MLP in fp32)
         "l.layer2.weight": torch.randn(Cs, 2, 1, 1, generator=g)}
    inp = torch.randn(B, H, W, Ci, generator=g, dtype=D).requires_grad_(True)
    skip = torch.randn(B, H, W, Cs, generator=g, dtype=D).requires_grad_(True)
    gate = O.scale_long_gate(P, "l.", nchw(skip)).detach().reshape(B, Cs).to(D)
    cat = torch.cat((inp, skip * gate[:, None, None, :]), dim=-1)
    close(R.concat_gate_fwd(inp, skip, gate), cat.detach())
    gcat = torch.randn(cat.shape, generator=g, dtype=D)
    gmean = torch.randn(B, Cs, generator=g, dtype=D)
    # gmean is the gradient of the per-sample mean of the skip (the gate MLP's input)
    ((cat * gcat).sum() + (skip.mean(dim=(1, 2)) * gmean).sum()).backward()
    ginp, gskip = R.concat_gate_bwd(gcat, gate, gmean, Ci)
    assert torch.equal(ginp, inp.grad)
    close(gskip, skip.grad)


@pytest.mark.parametrize("Cimg,CP,nsig", [(1, 8, 3), (3, 32, 1), (4, 8, 3)])
def test_precond_and_conv_out(Cimg, CP, nsig):
    g = gen(13 + Cimg)
    B, H, W, C, Co = 3, 5, 7, 16, Cimg
    sd = 0.5
    noisy = torch.randn(B, Cimg, H, W, generator=g, dtype=D)
    sigma = torch.randn(nsig, generator=g, dtype=D).exp()
    c_skip, c_out, c_in = (t.to(D) for t in O.precond_scalars(sigma.expand(B) if nsig == 1 else sigma, sd))
    out = R.precond_in(noisy, sigma, sd, CP)
    # the oracle's scalars are fp32
    close(nchw(out)[:, :Cimg], c_in * noisy, 1e-6)
    assert (out[..., Cimg] == 1).all() and (out[..., Cimg + 1:] == 0).all()
    x = torch.randn(B, H, W, C, generator=g, dtype=D).requires_grad_(True)
    wh = torch.randn(Co, C, generator=g, dtype=D).requires_grad_(True)
    gain = torch.tensor(0.7, dtype=D, requires_grad=True)
    s = sigma.expand(B) if nsig == 1 else sigma
    den = s * s + sd * sd
    Fr = F.conv2d(nchw(x), wh[:, :, None, None])
    Dref = Fr * gain * (s * sd / den.sqrt())[:, None, None, None] + noisy * (sd * sd / den)[:, None, None, None]
    Dm, Fm = R.conv_out_fwd(x, wh, 0.7, noisy, sigma, sd)
    close(Dm, Dref.detach())
    close(Fm, Fr.detach())
    close(Dm, (Fr.detach() * 0.7 * c_out + noisy * c_skip), 1e-6)
    dD = torch.randn(B, Co, H, W, generator=g, dtype=D)
    Dref.backward(dD)
    gx, gw, gg = R.conv_out_bwd(x, wh, 0.7, Fm, dD, sigma, sd)
    close(gx, x.grad)
    close(gw, wh.grad)
    close(gg, gain.grad)


def test_layout():
    x = torch.randn(2, 24, 5, 9, generator=gen(14), dtype=D)
    y = R.nchw_to_nhwc(x)
    assert y.shape == (2, 5, 9, 24) and y.is_contiguous() and y[1, 2, 3, 4] == x[1, 4, 2, 3]
    assert torch.equal(R.nhwc_to_nchw(y), x)
