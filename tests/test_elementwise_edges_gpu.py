"""Edge-shape parity of the bf16 elementwise / norm / boundary kernels (tinyedm_amd/csrc/elementwise.hip) against the fp64
references of tests/elementwise_ref.py (themselves checked by tests/test_elementwise_ref_cpu.py).

The shapes are the smallest that reach a path of the launch arithmetic no other per-kernel test executes:
  * pixel norm: P = 1 / 21 / 105 pixels leave the last lane group of a wave partly filled (pv == false) for every
    lanes-per-pixel choice; C = 128/136 and 256/264 straddle pick_lpp's switches, C = 8 and 1024 are its ends;
  * every flat 16-byte kernel caps its grid at 4096 workgroups of 256 lanes (grid_for): the "over-cap" cases are the smallest
    tensors that send the grid-stride loop round a second, partly filled trip;
  * conv_out backward: several workgroups (atomics), HW < PS (the hw >= HW carry over several samples), PS shrunk by the
    48-KiB LDS limit; reduce_hw: the 512-row trip boundary, the p < HW tail, a partial 64-channel slice.

Comparison rule (the helpers below):
  * pure data movement is bit-equal;
  * a bf16 output with one final rounding is held PER ELEMENT to |y - ref| <= 2^-8 |ref| + a: 2^-8 |ref| covers the
    half-ulp rounding for any position in the binade, `a` is the worst-case fp32 evaluation error of the value that is
    rounded, derived next to each case (U = 2^-24 is the fp32 unit roundoff);
  * pixel-norm backward and concat_gate_bwd's gskip (a reduction and a cancellation) keep close_bf16(l2=8e-3, mx=3e-2);
  * fp32 outputs keep the bounds of tests/test_kernels_gpu.py.
No case excludes elements.  Every case seeds its own generator from its parameters."""
import math
import os
import zlib

import numpy as np
import pytest
import torch

import elementwise_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
bf16 = torch.bfloat16
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def gen(*params):
    return torch.Generator().manual_seed(zlib.crc32(repr(params).encode()))


def rbf(g, *shape, scale=1.0):
    """random bf16 CPU tensor"""
    return (torch.randn(*shape, generator=g) * scale).to(bf16)


def rbf_pool(g, *shape):
    """bf16 input of a 2x2 mean whose bf16 rounding is part of the contract: magnitudes in [2^-8, ~2^4) or exactly 0, so the
    four-term fp32 sum is exact (19 bits at most) and the rounded mean does not depend on the summation order"""
    x = (torch.randn(*shape, generator=g) * 2).to(bf16)
    return torch.where(x.abs().float() < 2.0 ** -8, torch.zeros_like(x), x)


def dv(t):
    return None if t is None else t.to(DEV)


def _name(what):
    from_env = os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" ")[0]
    return f"elementwise/{from_env}/{what}"


def rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def bit_equal(y, ref, what):
    from parity_log import record
    same = torch.equal(y.cpu(), ref.cpu())
    record(_name(what), 0.0 if same else 1.0, 0.0)
    assert same, f"{what}: not bit-equal"


def within(y, ref, a, what):
    """bf16 output with one final rounding: |y - ref| <= 2^-8 |ref| + a, every element"""
    from parity_log import record
    y = R.f64(y.float())
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    assert torch.isfinite(y).all(), f"{what}: non-finite output"
    err = (y - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + a
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, 2.0), torch.zeros_like(err)))
    worst = ratio.max().item()
    record(_name(what), worst, 1.0)
    print(f"{_name(what)}: worst err/bound {worst:.3f}")
    if worst > 1.0:
        i = ratio.argmax().item()
        raise AssertionError(f"{what}: {(ratio > 1).sum().item()} of {ratio.numel()} elements over the bound; worst at flat index {i}: "
                             f"y={y.reshape(-1)[i].item():.9g} ref={ref.reshape(-1)[i].item():.9g} bound={bound.reshape(-1)[i].item():.3g}")


def close_bf16(y, ref, what, l2=4e-3, mx=1.5e-2):
    """tests/test_kernels_gpu.py's rule"""
    from parity_log import record
    y = R.f64(y.float())
    assert y.shape == ref.shape and torch.isfinite(y).all(), what
    e = rel(y, ref)
    record(_name(what), e, l2)
    print(f"{_name(what)}: rel L2 {e:.3e} (limit {l2:.0e}), max err {(y - ref).abs().max().item():.3e}")
    assert e <= l2, f"{what}: rel L2 {e:.3e}"
    assert (y - ref).abs().max().item() <= mx * ref.abs().max().item() + 1e-6, \
        f"{what}: max err {(y - ref).abs().max().item():.3e} vs scale {ref.abs().max().item():.3e}"


def close_f32(y, ref, tol, what):
    from parity_log import record
    y = R.f64(y)
    assert y.shape == ref.shape and torch.isfinite(y).all(), what
    e = rel(y, ref)
    record(_name(what), e, tol)
    print(f"{_name(what)}: rel L2 {e:.3e} (limit {tol:.0e})")
    assert e <= tol, f"{what}: rel L2 {e:.3e}"


# ---- worst-case fp32 evaluation errors (absolute) of the functions the kernels round to bf16
def err_silu(x):
    """mp_silu_b(x) = x * rcp(1 + __expf(-x)) * (1 / 0.596f): the argument scaling inside __expf (x * log2 e, relative error
    2 |x| U in the exponential), v_exp_f32 and v_rcp_f32 (1 ulp = 2 U each), one add, two multiplies, the constant
    (2 U): (10 + 2 |x|) U relative"""
    x = R.f64(x)
    return (10 + 2 * x.abs()) * U * R.mp_silu(x).abs()


def err_silu_grad(x):
    """mp_silu_grad_b(x) = s (1 + x (1 - s)) / 0.596: s as above to es = (5 + 2 |x|) U relative; the inner sum cancels
    (x (1 - s) -> -1), so its error is absolute: |x| es + U (1 + 3 |x|); the outer products add es + 3 U relative"""
    x = R.f64(x)
    s = torch.sigmoid(x)
    es = (5 + 2 * x.abs()) * U
    return s / R.SILU_DIV * (x.abs() * es + U * (1 + 3 * x.abs())) + R.mp_silu_grad(x).abs() * (es + 3 * U)


def err_norm(C):
    """relative error of 1 / (eps + sqrt(sum_C v^2) / sqrt(C)) in fp32: any summation order of C non-negative terms is within
    (C - 1) U of the sum, the square root halves it; sqrt, rsqrt, multiply, add, divide: 10 U more"""
    return (C / 2 + 10) * U


# ================================================================== pixel norm + mp_silu
PN_C = [8, 128, 136, 256, 264, 768, 1024]
PN_PIX = [(1, 1, 1), (1, 3, 7), (3, 5, 7)]
PN_OVERCAP = [(65, 31, 33, 64), (33, 31, 33, 136), (17, 31, 33, 264)]      # P > 4096 workgroups * 4 waves * (64 / LPP)


def _check_pnorm_fwd(ops, x, xn, a, d, exact_row=None):
    """xn, a, d of pixelnorm_silu_fwd (or the pooled form: `exact_row` = the rounded pooled tensor) against fp64"""
    row = R.f64(x.float()) if exact_row is None else exact_row
    C = row.shape[-1]
    xn_ref, d_ref = R.pixelnorm_fwd(row)
    within(xn, xn_ref, err_norm(C) * xn_ref.abs(), "xn")                   # a: one multiply by the fp32 reciprocal norm
    within(a, R.mp_silu(xn.float()), err_silu(xn.float()), "a")            # mp_silu of the STORED xn
    close_f32(d.cpu(), d_ref, 1e-5, "dsave")
    dd = R.f64(d)
    assert ((dd - d_ref).abs() <= err_norm(C) * d_ref).all(), "dsave: an element off by more than the fp32 evaluation error"


@pytest.mark.parametrize("pix", PN_PIX, ids=lambda p: "x".join(map(str, p)))
@pytest.mark.parametrize("C", PN_C)
def test_pixelnorm_silu_fwd_edges(ops, C, pix):
    x = rbf(gen("pnf", C, pix), *pix, C, scale=2.0)
    xn, a, d = ops.pixelnorm_silu_fwd(dv(x))
    _check_pnorm_fwd(ops, x, xn, a, d)


@pytest.mark.parametrize("shape", PN_OVERCAP, ids=lambda s: "x".join(map(str, s)))
def test_pixelnorm_silu_fwd_over_cap(ops, shape):
    x = rbf(gen("pnfo", shape), *shape, scale=2.0)
    xn, a, d = ops.pixelnorm_silu_fwd(dv(x))
    _check_pnorm_fwd(ops, x, xn, a, d)


BWD_COMBOS = [(1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0)]     # gxn, ga, gadd present


def _pnorm_bwd_case(ops, g, x, combos):
    xd = dv(x)
    xn, a, d = ops.pixelnorm_silu_fwd(xd)
    gxn, ga, gadd = (rbf(g, *x.shape) for _ in range(3))
    for use_gxn, use_ga, use_add in combos:
        args = (gxn if use_gxn else None, 0.8, ga if use_ga else None, gadd if use_add else None)
        gx = ops.pixelnorm_silu_bwd(xn, d, dv(args[0]), args[1], dv(args[2]), gadd=dv(args[3]))
        ref = R.pixelnorm_bwd(xn.float(), d, *args)
        close_bf16(gx, ref, f"gx[gxn={use_gxn},ga={use_ga},gadd={use_add}]", l2=8e-3, mx=3e-2)


@pytest.mark.parametrize("pix", PN_PIX, ids=lambda p: "x".join(map(str, p)))
@pytest.mark.parametrize("C", PN_C)
def test_pixelnorm_silu_bwd_edges(ops, C, pix):
    g = gen("pnb", C, pix)
    _pnorm_bwd_case(ops, g, rbf(g, *pix, C, scale=2.0), BWD_COMBOS)


@pytest.mark.parametrize("shape", PN_OVERCAP, ids=lambda s: "x".join(map(str, s)))
def test_pixelnorm_silu_bwd_over_cap(ops, shape):
    g = gen("pnbo", shape)
    _pnorm_bwd_case(ops, g, rbf(g, *shape, scale=2.0), [(1, 1, 1), (0, 1, 0)])


@pytest.mark.parametrize("C", [8, 136, 264, 1024])
def test_pixelnorm_silu_degenerate_rows(ops, C):
    """an all-zero row (d == NORM_EPS exactly; backward: s == 0 -> coef = 0, gx = g / eps), a row of magnitude 2^-60 (far below
    NORM_EPS: its norm vanishes in eps + n) and one of magnitude 2^30, inside an otherwise random tensor"""
    g = gen("pndeg", C)
    x = torch.randn(1, 3, 7, C, generator=g) * 2
    ZERO, TINY, HUGE = (0, 0, 2), (0, 1, 2), (0, 2, 1)
    x[ZERO] = 0
    x[TINY] *= 2.0 ** -60
    x[HUGE] *= 2.0 ** 30
    x = x.to(bf16)
    xn, a, d = ops.pixelnorm_silu_fwd(dv(x))
    _check_pnorm_fwd(ops, x, xn, a, d)
    dm = d.cpu().view(1, 3, 7)
    eps32 = torch.tensor(1e-4, dtype=torch.float32)
    assert dm[ZERO] == eps32 and dm[TINY] == eps32, (dm[ZERO].item(), dm[TINY].item())
    assert (xn[ZERO] == 0).all() and (a[ZERO] == 0).all()
    gxn, ga, gadd = (rbf(g, *x.shape) for _ in range(3))
    normal = torch.ones(1, 3, 7, dtype=torch.bool)
    for r in (ZERO, TINY, HUGE):
        normal[r] = False
    for use_add in (0, 1):
        add = gadd if use_add else None
        gx = ops.pixelnorm_silu_bwd(xn, d, dv(gxn), 0.8, dv(ga), gadd=dv(add))
        ref = R.pixelnorm_bwd(xn.float(), d, gxn, 0.8, ga, add)
        close_bf16(gx, ref, f"gx all rows[gadd={use_add}]", l2=8e-3, mx=3e-2)
        # the g / eps rows dominate both norms: every group of rows on its own scale as well
        close_bf16(gx.cpu()[normal], ref[normal], f"gx random rows[gadd={use_add}]", l2=8e-3, mx=3e-2)
        for nm, r in (("zero", ZERO), ("tiny", TINY), ("huge", HUGE)):
            close_bf16(gx.cpu()[r], ref[r], f"gx {nm} row[gadd={use_add}]", l2=8e-3, mx=3e-2)
    # zero row, per element: g / eps.  a: g = 0.8 gxn + mp_silu'(0) ga (the error of mp_silu', two products, a sum), then the
    # reciprocal of d and the product with it: 4 U
    g0 = 0.8 * R.f64(gxn[ZERO].float()) + R.mp_silu_grad(torch.zeros(C)) * R.f64(ga[ZERO].float())
    gx = ops.pixelnorm_silu_bwd(xn, d, dv(gxn), 0.8, dv(ga))
    within(gx[ZERO], g0 / R.NORM_EPS, (err_silu_grad(torch.zeros(C)) * R.f64(ga[ZERO].float()).abs() + 4 * U * g0.abs()
                                        + 2 * U * (0.8 * R.f64(gxn[ZERO].float())).abs()) / R.NORM_EPS, "gx zero row = g/eps")


POOL_MAPS = [(1, 2, 2), (3, 6, 10), (2, 14, 4)]


@pytest.mark.parametrize("bhw", POOL_MAPS, ids=lambda p: "x".join(map(str, p)))
@pytest.mark.parametrize("C", [8, 136, 264])
def test_pool_pixelnorm_silu_against_fp64(ops, C, bhw):
    g = gen("ppn", C, bhw)
    B, H, W = bhw
    x = rbf_pool(g, B, H, W, C)
    xn, a, d = ops.pool_pixelnorm_silu_fwd(dv(x))
    assert xn.shape == (B, H // 2, W // 2, C)
    _check_pnorm_fwd(ops, x, xn, a, d, exact_row=R.bf(R.pool2(x.float(), 0.25)))
    gxn, ga = rbf(g, *xn.shape), rbf(g, *xn.shape)
    gadd = rbf(g, *x.shape)
    for add in (None, gadd):
        gx = ops.pool_pixelnorm_silu_bwd(xn, d, dv(gxn), 0.8, dv(ga), gadd=dv(add))
        ref = R.pool_pixelnorm_bwd(xn.float(), d, gxn, 0.8, ga, add)
        close_bf16(gx, ref, f"gx[gadd={add is not None}]", l2=8e-3, mx=3e-2)
        # the four source pixels of a pooled pixel receive the same rounded value: without gadd, bit-equal 2x2 blocks
        if add is None:
            t = gx.view(B, H // 2, 2, W // 2, 2, C)
            assert torch.equal(t[:, :, 0, :, 0], t[:, :, 1, :, 1]) and torch.equal(t[:, :, 0, :, 1], t[:, :, 1, :, 0]) \
                and torch.equal(t[:, :, 0, :, 0], t[:, :, 0, :, 1])


# ================================================================== flat kernels
FLAT_N = [8, 8 * 257, 33 * 32 * 32 * 256 + 24]       # the last: 8,650,776 > 4096 * 256 * 8 = 8,388,608, last trip partly filled


@pytest.mark.parametrize("n", FLAT_N)
def test_silu_fwd_flat(ops, n):
    x = rbf(gen("sf", n), n, scale=2.0)
    within(ops.silu_fwd(dv(x)), R.mp_silu(x.float()), err_silu(x.float()), "a")


@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("n", FLAT_N)
def test_silu_bwd_flat(ops, n, with_extra):
    g = gen("sb", n, with_extra)
    x, ga = rbf(g, n, scale=2.0), rbf(g, n)
    ge = rbf(g, n) if with_extra else None
    gx = ops.silu_bwd(dv(x), dv(ga), dv(ge), 0.7)
    gaf = R.f64(ga.float())
    # a: the error of mp_silu' times |ga|, the two products and the sum 2 U of each summand
    a = err_silu_grad(x.float()) * gaf.abs() + 2 * U * (R.mp_silu_grad(x.float()) * gaf).abs()
    if with_extra:
        a = a + 2 * U * (0.7 * R.f64(ge.float())).abs()
    within(gx, R.silu_bwd(x.float(), ga.float(), None if ge is None else ge.float(), np.float32(0.7)), a, "gx")


@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("n", FLAT_N)
def test_axpby_flat(ops, n, with_b):
    g = gen("ax", n, with_b)
    a_, b_ = rbf(g, n), (rbf(g, n) if with_b else None)
    al, be = np.float32(0.8574929), np.float32(-0.5144957)
    out = ops.axpby(dv(a_), float(al), dv(b_), float(be))
    # a = 2^-22 (|alpha a| + |beta b|): two products and a sum in fp32
    bound = 2.0 ** -22 * ((float(al) * R.f64(a_.float())).abs() + (0 if b_ is None else (float(be) * R.f64(b_.float())).abs()))
    within(out, R.axpby(a_.float(), al, None if b_ is None else b_.float(), be), bound, "out")


# ================================================================== modulation + dropout
MOD_SHAPES = [(1, 1, 1, 8), (2, 7, 7, 192), (3, 28, 28, 192), (2, 16, 16, 1024)]
SEED, SUB, STEP = 0x1234567812345678, 17, 5


def _mod_inputs(g, B, H, W, C):
    r, ga = rbf(g, B, H, W, C), rbf(g, B, H, W, C)
    wide = torch.randn(B, C + 40, generator=g) * 0.3            # lin: a column slice of a wider buffer (row stride C + 40)
    gain = torch.tensor(0.9)
    return r, ga, wide, gain


def _mod_errs(r, lin, gain, keep, pdrop):
    """m = lin * gain + 1 to em = 2 U (|lin gain| + 1) absolute; the argument r * m to |r| em + U |r m|"""
    rf = R.f64(r.float())
    m = (R.f64(lin) * float(gain) + 1.0)[:, None, None, :]
    em = 2 * U * ((R.f64(lin) * float(gain)).abs() + 1.0)[:, None, None, :]
    earg = rf.abs() * em + U * (rf * m).abs()
    return rf, m, em, earg, R.f64(keep) * R.dropout_scale(pdrop)


@pytest.mark.parametrize("pdrop", [0.0, 0.13])
@pytest.mark.parametrize("B,H,W,C", MOD_SHAPES)
def test_mod_silu_drop_edges(ops, B, H, W, C, pdrop):
    g = gen("mod", B, H, W, C, pdrop)
    r, ga, wide, gain = _mod_inputs(g, B, H, W, C)
    wd = dv(wide)
    lin_d, lin = wd[:, 16:16 + C], wide[:, 16:16 + C]
    rd, gad, gd = dv(r), dv(ga), dv(gain)
    a = ops.mod_silu_drop_fwd(rd, lin_d, gd, pdrop, SEED, SUB, STEP)
    keep = ops.dropout_mask(rd.numel(), pdrop, SEED, SUB, STEP, DEV).view(B, H, W, C).cpu()
    if pdrop > 0 and keep.numel() >= 1 << 16:
        assert abs(keep.float().mean().item() - (1 - pdrop)) < 0.01            # keep rate (RNG parity is distributional)
    if pdrop == 0:
        assert keep.all()
    rf, m, em, earg, ks = _mod_errs(r, lin, gain, keep, pdrop)
    # forward.  a: mp_silu is 1.85-Lipschitz (max |mp_silu'| = 1.0998 / 0.596), its own error, the rescale (U)
    ref = R.mod_silu_drop_fwd(r.float(), lin, gain, keep, pdrop)
    within(a, ref, ks * (1.85 * earg + err_silu(rf * m)) + 2 * U * ref.abs(), "a")
    # backward into a strided glin, an accumulating ggain
    gr_ref, gm_ref, glin_ref, gg_ref = R.mod_silu_drop_bwd(r.float(), lin, gain, ga.float(), keep, pdrop)
    glin_wide = torch.full((B, C + 24), 7.0, device=DEV)
    ggain = torch.full((), 3.0, device=DEV)
    gr, glin, gg = ops.mod_silu_drop_bwd(rd, lin_d, gd, gad, pdrop, SEED, SUB, STEP, glin_out=glin_wide[:, 8:8 + C],
                                         ggain_out=ggain)
    # gr = gu * m, gu = ga * scale * mp_silu'(r m).  a: mp_silu' is 0.84-Lipschitz (max |mp_silu''| = 0.5 / 0.596) in the
    # argument, its own error; m's error on gu; three products
    gaf = R.f64(ga.float()).abs()
    a_gr = gaf * ks * m.abs() * (0.84 * earg + err_silu_grad(rf * m)) + (gaf * ks * R.mp_silu_grad(rf * m).abs()) * em \
        + 4 * U * gr_ref.abs()
    within(gr, gr_ref, a_gr, "gr")
    assert glin.data_ptr() == glin_wide[:, 8:8 + C].data_ptr() and gg.data_ptr() == ggain.data_ptr()
    assert (glin_wide[:, :8] == 7).all() and (glin_wide[:, 8 + C:] == 7).all()          # neighbours untouched
    close_f32(glin_wide[:, 8:8 + C].cpu(), glin_ref, 2e-3, "glin")
    assert abs(ggain.item() - 3.0 - gg_ref.item()) <= 2e-3 * abs(gg_ref.item()) + 1e-3, (ggain.item(), gg_ref.item())
    # the raw form: gm into a column slice of a zero-filled wider buffer
    gm_all = torch.zeros(B, C + 96, device=DEV)
    gr2, n1, n2 = ops.mod_silu_drop_bwd(rd, lin_d, gd, gad, pdrop, SEED, SUB, STEP, gm_out=gm_all[:, 32:32 + C])
    assert n1 is None and n2 is None
    bit_equal(gr2, gr, "gr raw == gr")
    assert (gm_all[:, :32] == 0).all() and (gm_all[:, 32 + C:] == 0).all()
    close_f32(gm_all[:, 32:32 + C].cpu(), gm_ref, 2e-3, "gm")


@pytest.mark.parametrize("B,H,W,C", MOD_SHAPES[1:3])
def test_mod_silu_drop_dyn_record_overrides_seed_and_step(ops, B, H, W, C):
    """a non-null `dyn` (the edm_step_params record of a captured step) replaces the by-value seed and step"""
    g = gen("moddyn", B, H, W, C)
    r, ga, wide, gain = _mod_inputs(g, B, H, W, C)
    rd, gad, lin_d, gd = dv(r), dv(ga), dv(wide)[:, 16:16 + C], dv(gain)
    seed2, step2, pdrop = 0x0FEDCBA987654321, 41, 0.13
    rec = np.zeros(12, dtype=np.uint32)
    rec[0], rec[1], rec[2] = step2, seed2 & 0xFFFFFFFF, seed2 >> 32
    rec = torch.from_numpy(rec.view(np.int32)).to(DEV)
    a_dyn = ops.mod_silu_drop_fwd(rd, lin_d, gd, pdrop, SEED, SUB, STEP, dyn=rec)
    a_rec = ops.mod_silu_drop_fwd(rd, lin_d, gd, pdrop, seed2, SUB, step2)
    a_arg = ops.mod_silu_drop_fwd(rd, lin_d, gd, pdrop, SEED, SUB, STEP)
    bit_equal(a_dyn, a_rec, "fwd dyn == record's values as scalars")
    assert not torch.equal(a_dyn, a_arg)
    gr_dyn, glin_dyn, _ = ops.mod_silu_drop_bwd(rd, lin_d, gd, gad, pdrop, SEED, SUB, STEP, dyn=rec)
    gr_rec, glin_rec, _ = ops.mod_silu_drop_bwd(rd, lin_d, gd, gad, pdrop, seed2, SUB, step2)
    gr_arg, _, _ = ops.mod_silu_drop_bwd(rd, lin_d, gd, gad, pdrop, SEED, SUB, STEP)
    bit_equal(gr_dyn, gr_rec, "bwd dyn == record's values as scalars")
    assert not torch.equal(gr_dyn, gr_arg)
    close_f32(glin_dyn.cpu(), R.f64(glin_rec), 1e-5, "glin dyn (atomics: not bit-equal)")
    gm_a, gm_b = torch.zeros(B, C, device=DEV), torch.zeros(B, C, device=DEV)
    gr_raw_dyn, _, _ = ops.mod_silu_drop_bwd(rd, lin_d, gd, gad, pdrop, SEED, SUB, STEP, dyn=rec, gm_out=gm_a)
    ops.mod_silu_drop_bwd(rd, lin_d, gd, gad, pdrop, seed2, SUB, step2, gm_out=gm_b)
    bit_equal(gr_raw_dyn, gr_rec, "bwd_raw dyn == record's values as scalars")
    close_f32(gm_a.cpu(), R.f64(gm_b), 1e-5, "gm dyn (atomics: not bit-equal)")


# ================================================================== resampling
RS_MAPS = [(1, 2, 2, 8), (3, 6, 10, 24), (2, 14, 4, 72), (2, 4, 14, 72)]


def _sum4_abs(x):
    xa = R.f64(x.float()).abs()
    return xa[:, 0::2, 0::2] + xa[:, 0::2, 1::2] + xa[:, 1::2, 0::2] + xa[:, 1::2, 1::2]


@pytest.mark.parametrize("B,H,W,C", RS_MAPS)
def test_resample_against_fp64(ops, B, H, W, C):
    g = gen("rs", B, H, W, C)
    x = rbf(g, B, H, W, C)
    xd = dv(x)
    for s in (0.25, 0.7):
        s32 = float(np.float32(s))
        # a = 2^-22 * sum |s x_i|: three additions and the product
        within(ops.pool2(xd, s), R.pool2(x.float(), s32), 2.0 ** -22 * s32 * _sum4_abs(x), f"pool2[{s}]")
    up_ref = R.up2(x.float())
    bit_equal(ops.up2(xd), up_ref.to(bf16), "up2")
    add = rbf(g, B, 2 * H, 2 * W, C)
    s32 = float(np.float32(0.3))
    # a = 2^-22 (|s x| + |add|)
    within(ops.up2(xd, 0.3, add=dv(add)), R.up2(x.float(), s32, add.float()),
           2.0 ** -22 * (s32 * up_ref.abs() + R.f64(add.float()).abs()), "up2(scale, add)")
    within(ops.up2(xd, 0.25), R.up2(x.float(), 0.25), 0.0, "up2(0.25)")                    # a power of two: exact
    y, a = ops.up2_silu(xd)
    bit_equal(y, up_ref.to(bf16), "up2_silu y")
    within(a, R.mp_silu(up_ref), err_silu(up_ref), "up2_silu a")


def test_up2_over_cap(ops):
    """(9,32,32,264) in: 9,732,096 output elements > 4096 * 256 * 8"""
    g = gen("up2cap")
    x = rbf(g, 9, 32, 32, 264)
    up_ref = R.up2(x.float())
    bit_equal(ops.up2(dv(x)), up_ref.to(bf16), "up2")
    y, a = ops.up2_silu(dv(x))
    bit_equal(y, up_ref.to(bf16), "up2_silu y")
    within(a, R.mp_silu(up_ref), err_silu(up_ref), "up2_silu a")
    # and the pool back down: sixteen-fold smaller than the cap, but the 2x2 mean of an upsampled tensor is the tensor
    bit_equal(ops.pool2(y), x, "pool2(up2(x)) == x")


# ================================================================== reduce_hw
@pytest.mark.parametrize("HW", [1, 33, 513, 1025])
@pytest.mark.parametrize("C", [8, 72, 200])
def test_reduce_hw_edges(ops, C, HW):
    g = gen("red", C, HW)
    B = 2
    x = rbf(g, B, 1, HW, C)
    xd = dv(x)
    out = ops.reduce_hw(xd, scale=1.0 / HW)
    assert out.shape == (B, C)
    close_f32(out.cpu(), R.reduce_hw(x.float(), scale=np.float32(1.0 / HW)), 1e-4, "mean")
    bit_equal(ops.reduce_hw(xd, scale=1.0 / HW), out, "mean twice")
    # a channel slice of a wider x (c_off = 8, C < Cx - 8) times a wider y, scale != 1
    xw, yw = rbf(g, B, 1, HW, C + 24), rbf(g, B, 1, HW, C + 8)
    xwd, ywd = dv(xw), dv(yw)
    o2 = ops.reduce_hw(xwd, C=C, c_off=8, y=ywd, scale=0.37)
    assert o2.shape == (B, C)
    close_f32(o2.cpu(), R.reduce_hw(xw.float(), C=C, c_off=8, y=yw.float(), scale=np.float32(0.37)), 1e-4, "sum x*y slice")
    bit_equal(ops.reduce_hw(xwd, C=C, c_off=8, y=ywd, scale=0.37), o2, "sum x*y twice")


# ================================================================== concat / gate
@pytest.mark.parametrize("want_silu", [False, True])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (33, 31)])
@pytest.mark.parametrize("Ci,Cs", [(8, 8), (72, 200), (256, 64)])
def test_concat_gate_edges(ops, Ci, Cs, H, W, want_silu):
    g = gen("cg", Ci, Cs, H, W, want_silu)
    B = 2
    inp, skip = rbf(g, B, H, W, Ci), rbf(g, B, H, W, Cs)
    gate = torch.rand(B, Cs, generator=g)
    cat, sil = ops.concat_gate_fwd(dv(inp), dv(skip), dv(gate), want_silu)
    ref = R.concat_gate_fwd(inp.float(), skip.float(), gate)
    bit_equal(cat[..., :Ci], inp, "cat input half")
    within(cat[..., Ci:], ref[..., Ci:], U * ref[..., Ci:].abs(), "cat skip half")       # a: one fp32 product
    if want_silu:
        within(sil, R.mp_silu(cat.float()), err_silu(cat.float()), "sil")                # mp_silu of the STORED cat
    else:
        assert sil is None
    gcat = rbf(g, B, H, W, Ci + Cs)
    gmean = torch.randn(B, Cs, generator=g)
    ginp, gskip = ops.concat_gate_bwd(dv(gcat), dv(gate), dv(gmean), Ci)
    ginp_ref, gskip_ref = R.concat_gate_bwd(gcat.float(), gate, gmean, Ci)
    bit_equal(ginp, ginp_ref.to(bf16), "ginp")
    close_bf16(gskip, gskip_ref, "gskip", l2=8e-3, mx=3e-2)


# ================================================================== preconditioning
def _sigmas(g, B):
    return {"per-sample": torch.randn(B, generator=g).exp(), "one": torch.tensor([1.7])}


def _check_precond(ops, g, B, Cimg, H, W, CP):
    noisy = torch.randn(B, Cimg, H, W, generator=g)
    for kind, sigma in _sigmas(g, B).items():
        out = ops.precond_in(dv(noisy), dv(sigma), 0.5, CP)
        ref = R.precond_in(noisy, sigma, 0.5, CP)
        # a: c_in = rsqrt(sd^2 + s^2) (two squares, a sum, v_rsq 1 ulp) and the product: 8 U relative
        within(out[..., :Cimg], ref[..., :Cimg], 8 * U * ref[..., :Cimg].abs(), f"image channels[{kind}]")
        bit_equal(out[..., Cimg:], ref[..., Cimg:].to(bf16), f"padding channels[{kind}]")
        assert (out[..., Cimg] == 1).all() and (out[..., Cimg + 1:] == 0).all()


@pytest.mark.parametrize("H,W", [(1, 1), (28, 28), (5, 7)])
@pytest.mark.parametrize("CP", [8, 32])
@pytest.mark.parametrize("Cimg", [1, 3, 4])
def test_precond_in_edges(ops, Cimg, CP, H, W):
    _check_precond(ops, gen("pre", Cimg, CP, H, W), 3, Cimg, H, W, CP)


def test_precond_in_over_cap(ops):
    """257 * 64 * 64 = 1,052,672 pixels > 4096 * 256"""
    _check_precond(ops, gen("precap"), 257, 3, 64, 64, 8)


# ================================================================== conv_out
CO_SHAPES = [(100, 2, 2, 8, 1),        # HW < PS (256): one pixel per lane, two workgroups
             (3, 7, 7, 192, 3),
             (5, 28, 28, 64, 4),       # npix = 3920 (no multiple of 256), samples straddle workgroups
             (2, 8, 8, 512, 8),        # PS shrunk to 3 by the LDS limit (block = 192)
             (1, 15, 20, 1024, 8),     # PS = 1
             (200, 2, 2, 64, 3)]       # PS = 32 > HW = 4: the hw >= HW carry walks 8 samples per step, 4 workgroups


@pytest.mark.parametrize("B,H,W,C,Co", CO_SHAPES)
def test_conv_out_edges(ops, B, H, W, C, Co):
    g = gen("co", B, H, W, C, Co)
    x = rbf(g, B, H, W, C)
    wh = torch.randn(Co, C, generator=g) / math.sqrt(C)
    gain = torch.tensor(0.7)
    noisy = torch.randn(B, Co, H, W, generator=g)
    xd, whd, gd, nd = dv(x), dv(wh), dv(gain), dv(noisy)
    for kind, sigma in _sigmas(g, B).items():
        sd = dv(sigma)
        D_ref, F_ref = R.conv_out_fwd(x.float(), wh, gain, noisy, sigma, 0.5)
        D, Fraw = ops.conv_out_fwd(xd, whd, gd, nd, sd, 0.5)
        close_f32(D.cpu(), D_ref, 1e-5, f"D[{kind}]")
        close_f32(Fraw.cpu(), F_ref, 1e-5, f"Fraw[{kind}]")
        D2, none = ops.conv_out_fwd(xd, whd, gd, nd, sd, 0.5, want_fraw=False)
        assert none is None
        bit_equal(D2, D, f"D without Fraw[{kind}]")
        # dD correlated with F: d loss / d gain = sum dD c_out F is then a sum of mostly positive terms, and its relative
        # bound does not hinge on how far a random sum happens to cancel
        dD = torch.randn(B, Co, H, W, generator=g) + (F_ref / F_ref.square().mean().sqrt()).float()
        gx_ref, gw_ref, gg_ref = R.conv_out_bwd(x.float(), wh, gain, Fraw.cpu(), dD, sigma, 0.5)
        gg_out = torch.full((), 3.0, device=DEV)
        gx, gw, gg = ops.conv_out_bwd(xd, whd, gd, Fraw, dv(dD), sd, 0.5, gg_out=gg_out)
        # gx = sum_o dF_o wh[o,c], dF = dD c_out gain.  a: c_out gain to 8 U, Co products and sums: (Co + 10) U sum |dF_o wh|
        c_out = R.precond_scalars(sigma, 0.5, B)[1][:, None, None, None]
        absum = torch.einsum("bohw,oc->bhwc", (R.f64(dD) * c_out * 0.7).abs(), R.f64(wh).abs())
        within(gx, gx_ref, (Co + 10) * U * absum, f"gx[{kind}]")
        close_f32(gw.cpu(), gw_ref, 1e-4, f"gw_hat[{kind}]")
        assert gg.data_ptr() == gg_out.data_ptr()
        assert abs(gg_out.item() - 3.0 - gg_ref.item()) <= 1e-4 * abs(gg_ref.item()) + 1e-5, (gg_out.item(), gg_ref.item())


def test_conv_out_fwd_over_cap(ops):
    """129 * 1024 = 132,096 pixels > 4096 workgroups * 32 pixels"""
    g = gen("cocap")
    B, H, W, C, Co = 129, 32, 32, 64, 3
    x = rbf(g, B, H, W, C)
    wh = torch.randn(Co, C, generator=g) / math.sqrt(C)
    noisy, sigma, gain = torch.randn(B, Co, H, W, generator=g), torch.randn(B, generator=g).exp(), torch.tensor(0.7)
    D, Fraw = ops.conv_out_fwd(dv(x), dv(wh), dv(gain), dv(noisy), dv(sigma), 0.5)
    D_ref, F_ref = R.conv_out_fwd(x.float(), wh, gain, noisy, sigma, 0.5)
    close_f32(D.cpu(), D_ref, 1e-5, "D")
    close_f32(Fraw.cpu(), F_ref, 1e-5, "Fraw")
    # per sample as well: a fault confined to the last trip's pixels is 0.8% of the tensor
    per = ((R.f64(D) - D_ref).flatten(1).norm(dim=1) / D_ref.flatten(1).norm(dim=1)).max().item()
    assert per <= 1e-5, per


# ================================================================== layout converters
@pytest.mark.parametrize("B,C,H,W", [(1, 8, 1, 1), (3, 24, 7, 7), (2, 72, 5, 9)])
def test_layout_converters(ops, B, C, H, W):
    x = torch.randn(B, C, H, W, generator=gen("cv", B, C, H, W))
    y = ops.nchw_to_nhwc_bf16(dv(x))
    bit_equal(y, x.permute(0, 2, 3, 1).to(bf16), "nchw -> nhwc bf16")
    back = ops.nhwc_bf16_to_nchw(y)
    assert back.dtype == torch.float32
    bit_equal(back, y.float().permute(0, 3, 1, 2), "nhwc bf16 -> nchw")
    bit_equal(back, x.to(bf16).float(), "round trip")
    bit_equal(ops.nchw_to_nhwc_bf16(back), y, "second trip")


# ================================================================== argument rejection
def test_elementwise_ops_reject_bad_operands(ops):
    from tinyedm_amd import _lib
    z = lambda *s, dt=bf16: torch.zeros(*s, device=DEV, dtype=dt)       # noqa: E731
    x = z(2, 4, 4, 16)
    d = z(32, dt=torch.float32)
    lin, gain = z(2, 16, dt=torch.float32), z((), dt=torch.float32)
    img, sig = z(2, 3, 4, 4, dt=torch.float32), z(2, dt=torch.float32)
    wh = z(3, 16, dt=torch.float32)
    # refused by the Python wrapper: no entry point is called
    bad = [
        (TypeError, lambda: ops.pixelnorm_silu_fwd(x.float())),
        (TypeError, lambda: ops.silu_fwd(x.half())),
        (TypeError, lambda: ops.axpby(x, 1.0, x.float(), 1.0)),
        (TypeError, lambda: ops.pixelnorm_silu_bwd(x, d.double(), x, 1.0, x)),
        (TypeError, lambda: ops.precond_in(img.double(), sig, 0.5, 8)),
        (TypeError, lambda: ops.nchw_to_nhwc_bf16(img.to(bf16))),
        (TypeError, lambda: ops.nhwc_bf16_to_nchw(x.float())),
        (ValueError, lambda: ops.pixelnorm_silu_fwd(x.transpose(1, 2))),
        (ValueError, lambda: ops.silu_bwd(x, x.transpose(1, 2))),
        (ValueError, lambda: ops.pool2(x[:, :, :, :8])),
        (ValueError, lambda: ops.up2(x.transpose(1, 2))),
        (ValueError, lambda: ops.concat_gate_fwd(x, x[:, :2], z(2, 16, dt=torch.float32), False)),
        (ValueError, lambda: ops.mod_silu_drop_fwd(x, lin.t().contiguous().t(), gain, 0.0, 1, 2, 3)),
        (ValueError, lambda: ops.pool2(z(2, 3, 4, 16))),
        (ValueError, lambda: ops.pool2(z(2, 4, 5, 16))),
        (ValueError, lambda: ops.pool_pixelnorm_silu_fwd(z(2, 3, 4, 16))),
        (ValueError, lambda: ops.pool_pixelnorm_silu_fwd(z(2, 4, 5, 16))),
        (ValueError, lambda: ops.pool_pixelnorm_silu_fwd(z(1, 2, 2, 1032))),
        (ValueError, lambda: ops.up2(x, 1.0, add=x)),
        (ValueError, lambda: ops.up2(x, 1.0, add=z(2, 8, 8, 8))),
        (ValueError, lambda: ops.pixelnorm_silu_bwd(x, d, x, 1.0, x, gadd=z(2, 4, 4, 8))),
        (ValueError, lambda: ops.pixelnorm_silu_bwd(x, d[:31], x, 1.0, x)),
        (ValueError, lambda: ops.pool_pixelnorm_silu_bwd(x, d, x, 1.0, x, gadd=x)),
        (ValueError, lambda: ops.silu_bwd(x, x, gextra=z(2, 4, 4, 8))),
        (ValueError, lambda: ops.precond_in(img, z(3, dt=torch.float32), 0.5, 8)),
        (ValueError, lambda: ops.conv_out_fwd(x, wh, gain, img, z(5, dt=torch.float32), 0.5)),
        (ValueError, lambda: ops.conv_out_bwd(x, wh, gain, img, img, z(3, dt=torch.float32), 0.5)),
        (ValueError, lambda: ops.conv_out_bwd(x, wh, gain, img, img[:1], sig, 0.5)),
        (ValueError, lambda: ops.reduce_hw(x, C=8, c_off=4)),
        (ValueError, lambda: ops.reduce_hw(x, C=16, c_off=8)),
        (ValueError, lambda: ops.reduce_hw(x, y=z(2, 4, 4, 8))),
        (ValueError, lambda: ops.reduce_hw(x, y=z(2, 4, 2, 16))),
        (ValueError, lambda: ops.mod_silu_drop_fwd(x, z(2, 8, dt=torch.float32), gain, 0.0, 1, 2, 3)),
        (ValueError, lambda: ops.mod_silu_drop_bwd(x, lin, gain, z(2, 4, 4, 8), 0.0, 1, 2, 3)),
        (RuntimeError, lambda: ops.silu_fwd(x.cpu())),
    ]
    calls = _lib.N_CALLS
    for i, (exc, fn) in enumerate(bad):
        with pytest.raises(exc):
            fn()
        assert _lib.N_CALLS == calls, f"case {i} reached the library"
    # refused by the entry point's own argument check (EDM_REQUIRE, ahead of any launch)
    wide = z(1, 1, 1, 1032)
    lib_bad = [
        lambda: ops.pixelnorm_silu_fwd(z(2, 4, 4, 12)),                                    # C % 8 != 0
        lambda: ops.pixelnorm_silu_bwd(z(2, 4, 4, 12), d, None, 1.0, z(2, 4, 4, 12)),
        lambda: ops.silu_fwd(z(12)),
        lambda: ops.axpby(z(2, 3), 1.0),
        lambda: ops.pool2(z(2, 4, 4, 12)),
        lambda: ops.up2(z(2, 4, 4, 12)),
        lambda: ops.up2_silu(z(2, 4, 4, 12)),
        lambda: ops.concat_gate_fwd(z(2, 4, 4, 12), z(2, 4, 4, 12), z(2, 12, dt=torch.float32), False),
        lambda: ops.precond_in(img, sig, 0.5, 12),
        lambda: ops.precond_in(img, sig, 0.5, 0),                                           # CP <= Cimg
        lambda: ops.nhwc_bf16_to_nchw(z(2, 4, 4, 12)),
        lambda: ops.nchw_to_nhwc_bf16(z(2, 12, 4, 4, dt=torch.float32)),
        lambda: ops.conv_out_fwd(z(2, 4, 4, 12), z(3, 12, dt=torch.float32), gain, img, sig, 0.5),
        lambda: ops.pixelnorm_silu_fwd(wide),                                               # C = 1032 > 1024
        lambda: ops.pixelnorm_silu_bwd(wide, z(1, dt=torch.float32), wide, 1.0, wide),
        lambda: ops.pool_pixelnorm_silu_bwd(wide, z(1, dt=torch.float32), wide, 1.0, wide),
        lambda: ops.mod_silu_drop_bwd(wide, z(1, 1032, dt=torch.float32), gain, wide, 0.0, 1, 2, 3),
        lambda: ops.mod_silu_drop_bwd(wide, z(1, 1032, dt=torch.float32), gain, wide, 0.0, 1, 2, 3,
                                      gm_out=z(1, 1032, dt=torch.float32)),
        lambda: ops.mod_silu_drop_fwd(x, lin, gain, 1.0, 1, 2, 3),                          # pdrop = 1
    ]
    # P >= 2^31 pixels (the launch takes an int): not reachable through a tensor of a sane size, so at the entry points
    px, pd, st = ops._p(x), ops._p(d), ops._stream()
    lib_bad += [
        lambda: _lib.call("edm_pixelnorm_silu_fwd", px, px, px, pd, 1 << 31, 16, st),
        lambda: _lib.call("edm_pixelnorm_silu_bwd", px, pd, px, 1.0, px, None, px, 1 << 31, 16, st),
    ]
    for i, fn in enumerate(lib_bad):
        with pytest.raises(_lib.HipKernelError):
            fn()
    torch.cuda.synchronize()
