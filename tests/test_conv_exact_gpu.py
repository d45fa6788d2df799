"""Bit-exact tests of the MFMA convolution family (conv_igemm.hip, conv_igemm2.hip, conv_igemm5.hip, conv_igemm6.hip,
conv_wgrad2.hip, conv_wgrad1x1.hip, conv_wgrad3.hip) on integer operands (tests/conv_exact_ref.py): every product and
partial sum is an integer below 2^24 and every output is representable in the output type, so the result cannot depend
on summation order, split count, tile walk or team schedule and must EQUAL the fp64 reference.  A dropped tap on one
border column, a pixel row counted twice where two teams meet, a K share that runs past the end of K or a partial tile
summed from the wrong slot moves some output by at least 1 -- which a relative L2 norm over 10^5 outputs does not see.
On a mismatch the tests print how many elements differ and where: the pattern is the diagnosis."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_exact_ref as X

DEV = "cuda"
bf16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


class forced_igemm:
    """run the body on kernel generation `version` (ops.IGEMM_VERSION, as the igemm_version fixture of test_kernels_gpu)"""

    def __init__(self, ops, version):
        self.ops, self.version = ops, version

    def __enter__(self):
        self.old = self.ops.IGEMM_VERSION
        self.ops.IGEMM_VERSION = self.version

    def __exit__(self, *exc):
        self.ops.IGEMM_VERSION = self.old


def _report(what, got, want, names, extra=None, bad=None):
    """count of differing elements, the extent of the differences along each axis, the first few indices with got / expected"""
    bad = (got != want) if bad is None else bad
    idx = bad.nonzero()
    lines = [f"{what}: {idx.shape[0]} of {want.numel()} elements differ"]
    for a, nm in enumerate(names):
        u = idx[:, a].unique()
        lines.append(f"  {nm}: {u.numel()} distinct of {want.shape[a]}, {u[:12].tolist()}{' ...' if u.numel() > 12 else ''}")
    for i in idx[:8].tolist():
        i = tuple(i)
        lines.append(f"  {dict(zip(names, i))}: got {got[i].item()!r} expected {want[i].item()!r}"
                     + ("" if extra is None else f" ({extra[0]} {extra[1][i].item()!r})"))
    return "\n".join(lines)


def assert_equal(what, got, want, names):
    """got (device tensor, any float type) holds exactly the fp64 values `want`"""
    g = got.detach().cpu()
    if torch.equal(g, want.to(g.dtype)) and torch.equal(g.double(), want):
        return
    pytest.fail(_report(what, g.double(), want, names), pytrace=False)


NHWC = ("b", "h", "w", "co")
PACK = ("tap", "co", "ci")


# ------------------------------------------------------------------ 1. forward conv, every generation
@pytest.mark.parametrize("case", X.forward_cases(), ids=X.forward_id)
def test_conv_forward_is_exact(ops, case):
    B, H, W, Cin, Cout, taps, version, imgs, kernel = case
    c = X.conv_case(B, H, W, Cin, Cout, taps, imgs)
    with forced_igemm(ops, version):
        entry = ops._igemm_entry(B * H * W, W, Cout, taps, Cin)
        if kernel is not None:      # a forced generation runs the shape itself where conv_exact_ref.covers says so, else kernel 1
            assert entry == ops._ENTRY[kernel], (entry, kernel)
        y = ops.conv_igemm(c.x.to(DEV), c.wp.to(DEV), taps)
    assert y.dtype == bf16 and tuple(y.shape) == (B, H, W, Cout)
    assert_equal(f"conv_igemm {entry} {X.forward_id(case)} images {c.imgs}", y[c.imgs], c.ref, NHWC)


# ------------------------------------------------------------------ 2. linear epilogues
@pytest.mark.parametrize("version", X.IGEMM_VERSIONS, ids=[X.IGEMM_IDS[v] for v in X.IGEMM_VERSIONS])
@pytest.mark.parametrize("B,H,W,Cin,Cout,taps", X.RESIDUAL_SHAPES)
def test_conv_residual_epilogue_is_exact(ops, version, B, H, W, Cin, Cout, taps):
    """Y = 0.5 * conv + 2 * R with an integer residual: half-integers below 128, every one a bf16 value"""
    c, r, ref = X.residual_case(B, H, W, Cin, Cout, taps)
    with forced_igemm(ops, version):
        entry = ops._igemm_entry(B * H * W, W, Cout, taps, Cin)
        assert version == 0 or entry == ops._ENTRY[X.expected_kernel(version, W, Cin, taps)]
        y = ops.conv_igemm(c.x.to(DEV), c.wp.to(DEV), taps, residual=r.to(DEV), alpha=X.ALPHA, beta=X.BETA)
    assert_equal(f"residual form on {entry}", y, ref, NHWC)


@pytest.mark.parametrize("B,H,W,Cin,Cout,taps,version", X.DESCRIPTOR_CASES)
def test_conv_output_descriptor_is_exact(ops, B, H, W, Cin, Cout, taps, version):
    """out= with ldY > Cout and split=, residual form: the destination columns hold the fp64 reference exactly and the
    pre-filled columns beside them are unchanged"""
    c, r, ref = X.residual_case(B, H, W, Cin, Cout, taps)
    x, wp, res = c.x.to(DEV), c.wp.to(DEV), r.to(DEV)
    Cs, FILL = 64, 7.0
    with forced_igemm(ops, version):
        assert ops._KERNEL_ID[ops._igemm_entry(B * H * W, W, Cout, taps, Cin)] == version
        wide = torch.full((B, H, W, Cout + Cs), FILL, device=DEV, dtype=bf16)
        out = ops.conv_igemm(x, wp, taps, residual=res, alpha=X.ALPHA, beta=X.BETA, out=wide[..., :Cout])
        assert out.data_ptr() == wide.data_ptr()
        assert_equal(f"out= (ldY = {Cout + Cs}) on kernel {version}", wide[..., :Cout], ref, NHWC)
        assert bool((wide[..., Cout:] == FILL).all()), "columns outside the destination were written"
        for s in sorted({8, Cout // 2, Cout - 8}):
            if not (0 < s < Cout and s % 8 == 0):
                continue
            ya = torch.full((B, H, W, s), FILL, device=DEV, dtype=bf16)
            yb = torch.full((B, H, W, Cout - s), FILL, device=DEV, dtype=bf16)
            ops.conv_igemm(x, wp, taps, residual=res, alpha=X.ALPHA, beta=X.BETA, split=(s, ya, yb))
            assert_equal(f"split={s} left on kernel {version}", ya, ref[..., :s], NHWC)
            assert_equal(f"split={s} right on kernel {version}", yb, ref[..., s:], NHWC)


@pytest.mark.parametrize("B,H,W,Cin,Cout,C2,imgs", X.FOLD_SHAPES)
def test_conv3x3_fold_is_exact(ops, B, H, W, Cin, Cout, C2, imgs):
    """0.5 * conv3x3(x, W3) + 2 * conv1x1(x2, W1) in one launch, plain and into a column block of a wider buffer"""
    assert ops.conv3x3_fold_supported((B, H, W, Cin), Cout, C2)
    c = X.fold_case(B, H, W, Cin, Cout, C2, tuple(imgs))
    x, wp, x2, w2p = c.x.to(DEV), c.wp.to(DEV), c.x2.to(DEV), c.w2p.to(DEV)
    y = ops.conv3x3_fold(x, wp, x2, w2p, X.FOLD_A3, X.FOLD_A1)
    assert_equal("conv3x3_fold", y[c.imgs], c.ref, NHWC)
    FILL = 7.0
    wide = torch.full((B, H, W, Cout + 64), FILL, device=DEV, dtype=bf16)
    out = ops.conv3x3_fold(x, wp, x2, w2p, X.FOLD_A3, X.FOLD_A1, out=wide[..., :Cout])
    assert out.data_ptr() == wide.data_ptr()
    assert_equal("conv3x3_fold out=", wide[c.imgs][..., :Cout], c.ref, NHWC)
    assert torch.equal(wide[..., :Cout], y)                      # every image, not only the sampled ones
    assert bool((wide[..., Cout:] == FILL).all()), "columns outside the destination were written"


# ------------------------------------------------------------------ 3. raw weight-gradient slabs
def _check_slabs(what, slabs, ref):
    assert slabs.dtype == torch.float32 and tuple(slabs.shape[1:]) == tuple(ref.shape)
    assert torch.equal(slabs, slabs.round()), f"{what}: a slab holds a non-integer"
    assert_equal(f"{what}, {slabs.shape[0]} slabs", slabs.double().sum(0), ref, PACK)


@pytest.mark.parametrize("case,dedicated", [(c, d) for c in X.WGRAD_CASES for d in ((False, True) if c[5] == 1 else (True,))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("1x1-kernel" if v else "window-kernel"))
def test_conv_wgrad_slabs_are_exact(ops, case, dedicated):
    """ops.conv_wgrad: the rolling-window kernel (3x3, and 1x1 with WGRAD_1X1 off) and the dedicated 1x1 kernel"""
    c = X.wgrad_case(*case)
    old = ops.WGRAD_1X1
    ops.WGRAD_1X1 = dedicated
    try:
        slabs = ops.conv_wgrad(c.x.to(DEV), c.dy.to(DEV), case[5])
    finally:
        ops.WGRAD_1X1 = old
    _check_slabs(f"conv_wgrad {case}", slabs, c.ref)


def test_conv_wgrad_1x1_group_is_exact(ops):
    cases = [X.wgrad_case(*s, 1, int(k >= len(X.RAGGED_1X1))) for k, s in enumerate(X.GROUP_1X1)]
    slabs = ops.conv_wgrad_1x1_group([(c.x.to(DEV), c.dy.to(DEV)) for c in cases])
    torch.cuda.synchronize()
    for k, (c, sl) in enumerate(zip(cases, slabs)):
        _check_slabs(f"conv_wgrad_1x1_group layer {k} {X.GROUP_1X1[k]}", sl, c.ref)


# ------------------------------------------------------------------ 4. grouped stream-K 3x3 weight gradient
# With one-hot master rows k_wgrad3_finish computes, away from the row's 1.0, v = c0 * (scale * G[e]) with G the exact integer
# gradient.  fp32 roundings on the way (each at most 2^-24 relative): sqrtf(n), rn / sqn, eps + ., d * sqn, 1 / . (c0: 5),
# G * scale (6), c0 * . (7): 7 * 2^-24.  The fp64 reference rounds three times in fp32 inside O.rms_div / effective_weight
# (1 / sqrt(n), eps + ., sqrt(fan_in)): 3 * 2^-24.  With accumulate the sum g0 + v rounds once more, by at most
# 2^-24 |g0 + v| <= 6 * 2^-24 |v| for the operands of conv_exact_ref (|g0| <= 5 |v| where G != 0; checked on the CPU).
# Together at most 16 * 2^-24 = 2^-20 of |v|, while a missing or doubled term moves v by at least |v| / max|G| > 2^-14 |v|.
REL = 2.0 ** -20

W3_AXES = ("co", "ci", "ky", "kx")


def _ulp32(t):
    a = t.float().abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


@pytest.mark.parametrize("name", ["small", "wide", "teams", "ksplit", "ksplit-wide", "forty-three"])
def test_wgrad3_group_is_exact_up_to_the_projection(ops, name):
    group, layers = X.W3_GROUPS[name], X.w3_group(name)
    if name in X.W3_SPLIT_GROUPS:      # B is reduced: the layers that split in the full-size group still split here
        shapes = lambda grp: [(kw["B"], kw["H"], kw["W"], kw["Cin"], kw["Cout"]) for kw in grp]
        ks, ks0 = ops.wgrad3_plan_ksplit(shapes(group)), ops.wgrad3_plan_ksplit(shapes(X.W3_SPLIT_GROUPS[name]))
        assert [k > 1 for k in ks] == [k > 1 for k in ks0] and sum(k > 1 for k in ks) >= len(group) - 1, (ks, ks0)
    grads = [L.g0.clone().to(DEV) for L in layers]
    ops.wgrad3_group([(L.x.to(DEV), L.dy.to(DEV), L.wm.to(DEV), gr, None if L.perm is None else L.perm.to(DEV), L.scale,
                       L.accumulate) for L, gr in zip(layers, grads)])
    torch.cuda.synchronize()
    for k, (kw, L, gr) in enumerate(zip(group, layers, grads)):
        what = f"group {name} layer {k} {kw}"
        got = gr.cpu().double()
        v = L.ref - L.g0.double()                       # the kernel's own value; c0 * scale * G away from the 1.0
        off = ~L.star
        err = (got - L.ref).abs()
        bad = off & (err > REL * v.abs())
        if bool(bad.any()):
            pytest.fail(_report(what + f", off the 1.0 (worst {(err / v.abs().clamp_min(1e-300))[bad].max().item():.3e} relative)",
                                got, L.ref, W3_AXES, ("G", L.G), bad), pytrace=False)
        if not L.accumulate:
            nonzero = off & (L.G == 0) & (got != 0)
            if bool(nonzero.any()):
                pytest.fail(_report(what + ", G == 0 must give an exact zero", got, L.ref, W3_AXES, ("G", L.G), nonzero), pytrace=False)
        tol = REL * L.c0 * L.G.abs() + (_ulp32(L.ref) if L.accumulate else 0.0)
        bad = L.star & (err > tol)
        if bool(bad.any()):
            pytest.fail(_report(what + ", at the 1.0", got, L.ref, W3_AXES, ("G", L.G), bad), pytrace=False)


# ------------------------------------------------------------------ 5. weight packs as data movement
@pytest.mark.parametrize("O,I,taps,Ipad,perm", X.PACK_CASES)
def test_weight_packs_are_each_others_transpose(ops, O, I, taps, Ipad, perm):
    """the dgrad pack [taps][I][O] is the forward pack [taps][O][Ipad] of the same call with the taps flipped and the
    channels transposed, bit for bit; the forward pack's padding columns are zero"""
    g = torch.Generator().manual_seed(O + I + taps)
    k = 3 if taps == 9 else 1
    w = torch.randn(O, I, k, k, generator=g).to(DEV)
    p = torch.randperm(O, generator=g).to(torch.int32).to(DEV) if perm else None
    wf, wd, _ = ops.weight_prep(w, taps, Ipad=Ipad, perm=p)
    assert tuple(wf.shape) == (taps, O, Ipad or I) and tuple(wd.shape) == (taps, I, O)
    want = wf[:, :, :I].flip(0).transpose(1, 2).float().cpu().double()
    assert_equal("dgrad pack vs flipped, transposed forward pack", wd, want, ("tap", "ci", "co"))
    assert bool((wf[:, :, I:] == 0).all()) and bool((wf[:, :, :I] != 0).any())
