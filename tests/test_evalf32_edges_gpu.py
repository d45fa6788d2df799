"""Edge-shape parity of the fp32 evaluation path's elementwise kernels and of the split-bf16 pair format
(tinyedm_amd/csrc/eval_f32.hip) against the fp64 references and the exact pair restatement of tests/evalf32_ref.py
(themselves checked by tests/test_evalf32_ref_cpu.py).

Which path each shape reaches (every flat kernel caps its grid at 4096 workgroups -- gridf -- and goes round a grid-stride
loop; "over-cap" is the smallest size that sends it round a second, partly filled trip):
  * f32_pixelnorm_silu / f32_pool_pixelnorm_silu (one wave per pixel, four pixels per workgroup, lanes step c += 256):
    C = 4 one active lane; 252 / 256 / 260 the last lane of pass 1, a full pass, one active lane in pass 2; 768 three full
    passes; 1024 four (the limit of the pooled form, which keeps a row in registers); 1028 (plain kernel only) one lane in a
    fifth pass.  P = 1 / 3 / 5 output pixels: a workgroup with one or three working waves, and a second workgroup.
    Over-cap: P = 16384 + 3 at C = 4 (4096 workgroups x 4 waves).
  * flat quad kernels (f32_silu, f32_pool2, f32_up2, f32_up2_silu, f32_concat_gate, f32_skip_half; one float4 per lane):
    one quad in all (a (1,1,1,4) output; an upsample's smallest output is 2 x 2 pixels, four quads; a concat's is two);
    C = 4 with pairs (rows of 8 bf16: hi and lo of a pixel side by side); over-cap: 1 048 576 + 3 quads (+ 4 where the
    shape forces a multiple of four or two); B = 3 with HW = 1: the pix / HW lookup of the per-sample gate changes sample at
    every pixel; Ci != Cs: (4,4), (192,40), (64,768) move the boundary between the copied and the gated half of a row.
  * f32_skip_gate (one workgroup per sample, 1024 / (C/4) * (C/4) threads, rpp = threads / (C/4) pixel rows per pass):
    C = 4: 1024 threads, rpp 1024; 40: 1020 threads (a trailing partial wave that must sit the MLP out); 192, 576: 1008;
    1028: 771 threads, rpp 3; 4096: rpp 1.  HW = 1 / 3 / 49 / 1024 covers HW < rpp (idle row groups that must contribute
    zeros), HW == rpp and several passes.  R = max(1, C // 16) (the network's) and R = 1.  B = 1 and 3.
  * f32_precond_in (one lane per pixel): HW = 1 (p / HW == p), scalar sigma (stride 0) and per-sample sigma, Cimg = 1 / 3 / 4
    of CP = 8, the three sigmas 0.002 / 1 / 80 (c_in from 2 to 0.0125); over-cap: 3 x 349 527 pixels.
  * f32_conv_out (16 lanes per pixel, four pixels per wave trip, 16 pixels per workgroup): B*HW = 1 / 3 / 5 / 15 / 17 leave the
    last group of four partly filled (pv == false) in the first, second and fifth wave; C = 4: one lane of sixteen works;
    60 / 64 / 68: the last lane idle, a full trip, one lane in a second trip; 768: twelve trips.  Co = 1, 3, 4, 8 of the 8
    unrolled outputs.  Over-cap: 65536 + 5 pixels at C = 4 (B = 3: per-sample sigma across trips).
  * layout changes (one lane per element): C = 1, 3, 8, HW = 1, 49; over-cap: 1 048 576 + 5 elements.
  * f32_to_pairs (8 values per lane) / split_pack (one lane per padded element): see "pair format" below.

Comparison rules (the helpers below).  No case excludes elements; every output must be finite; every case seeds its own
generator from its parameters; every result goes through parity_log.record.
  * Data movement is bit-equal: f32_up2, the y of f32_up2_silu, both layout changes, precond_in's 1 and 0 channels, the
    input half of f32_concat_gate.
  * Pair format is bit-equal to the CPU restatement: f32_to_pairs == pairs_of, split_pack == split_pack_ref, on the tie
    patterns (low half 0x8000 under an even and an odd mantissa bit, both signs), +-0, one fp32 ulp either side of a tie
    and random mantissas at magnitudes from 2^-100 to 2^100.  Denormals, infinities and NaN are out of scope: the
    evaluation path never produces them and the matrix pipe flushes bf16 denormals anyway.
  * Every pairs=True output p, with v the fp64 reference of the value that is split: |value_of(p) - v| <= 2^-17 |v| + e,
    e the fp32 bound of the same kernel's plain output, and |lo| <= half a bf16 ulp of hi.
  * Pool: on short-mantissa inputs the four-term sum is exact and the result is bit-equal to the reference rounded to fp32;
    on random inputs |err| <= 3 U mean(|a|,|b|,|c|,|d|), U = 2^-24 (three additions; the * 0.25 is exact).
  * Other fp32 outputs keep the relative-L2 limits of test_f32_elementwise_vs_oracle (xn 1e-6, SiLU forms / gate / cat /
    conv_out 2e-6, precond_in 1e-6) AND a per-element bound |y - ref| <= k U |ref| + a, k and a derived next to each case
    from the operation count.
  * Measured allowances.  Where a value passes through __expf nobody has documented k, so none is invented: the kernel's
    documented expression is evaluated in numpy float32 on the CPU (evalf32_ref.mp_silu32 / skip_gate32: exp as
    exp2(x log2 e), |x| <= 8), its worst error against the fp64 reference is taken in units of U |ref|, and the kernel is
    allowed 4x that (the native exponential carries about an ulp plus the argument scaling, libm half an ulp).  The
    measurement is of the reference restated in fp32, never of the kernel; the figures stand at MEASURED_SILU and
    MEASURED_GATE.
  * Fused-form identities are torch.equal: pool + norm + SiLU == pool then norm + SiLU, upsample + SiLU == upsample then SiLU.
  * f32_skip_half into NaN-filled cat and sil leaves every input-half column NaN and every skip-half column finite.
  * Refusals are host checks before any launch: each raises and leaves sentinel-filled outputs untouched."""
import math
import os
import zlib

import numpy as np
import pytest
import torch

import evalf32_ref as R
from oracle import edm_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
bf16 = torch.bfloat16
U = 2.0 ** -24
OVER_QUADS = 1048576 + 3          # 4096 workgroups x 256 lanes, one quad each, + 3

# Measured allowances (see the docstring).
# mp_silu32 against mp_silu on the family's largest inputs, test_silu_edges' over-cap case (4 194 316 values of 2 * randn
# clamped to |x| <= 8; both pairs settings): worst error 9.03 U |ref| (at x near -5.6: the rounding of x log2 e); a sweep of
# 2^24 points over [-8, 8] gives 9.59.  Allowance 4 x 9.03 = 36.12 U |ref|, for every mp_silu output.
MEASURED_SILU = 9.03
SILU_K = 4 * MEASURED_SILU
# skip_gate32 against skip_gate, per case of test_skip_gate_edges, in U |ref|: (C, R) -> the eight (B, H, W) of GATE_BHW in
# order (None: not a case).  A case of B = 1 at C = 4 has four outputs, too few for their worst error to mean much, so each
# figure is the worst over the case's own inputs and seven further draws of the same shapes (gate_case(..., draw=1..7)).
# The figure grows where a gate saturates (HW = 1: the "mean" is one pixel, |W1 . m| is a few units, and the small gate
# values carry the exponential's whole argument error).  Allowance of a case: 4 x its figure.
MEASURED_GATE = {
    (4, 1): (2.52, 2.12, 1.32, 1.81, 5.60, 4.52, 1.79, 2.06),
    (40, 1): (3.95, 2.81, 2.04, 2.27, 4.34, 2.97, 2.39, 2.26),
    (40, 2): (9.12, 7.97, 2.23, 2.02, 7.87, 8.80, 2.30, 2.24),
    (192, 1): (3.02, 2.24, 2.32, 2.30, 6.63, 5.52, 2.60, 2.46),
    (192, 12): (15.11, 4.08, 2.39, 2.26, 13.81, 6.31, 2.43, 2.40),
    (576, 1): (4.27, 2.95, 2.30, 2.21, 13.00, 7.63, 2.63, 2.37),
    (576, 36): (12.97, 5.56, 2.45, 2.38, 18.86, 16.56, 2.57, 2.38),
    (1028, 1): (8.20, 5.03, 2.42, 2.06, 29.80, 8.86, 3.27, 2.59),
    (1028, 64): (15.97, 6.36, 2.79, 2.30, 26.23, 9.49, 3.05, 2.40),
    (4096, 1): (8.76, 3.52, 2.37, 2.14, 23.32, 15.38, 2.89, None),
    (4096, 256): (29.55, 11.49, 3.40, 2.50, 50.43, 22.80, 5.47, None),
}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def gen(*params):
    return torch.Generator().manual_seed(zlib.crc32(repr(params).encode()))


def dv(t):
    return None if t is None else t.to(DEV)


def _name(what):
    from_env = os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" ")[0]
    return f"evalf32_edges/{from_env}/{what}"


def rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def silu_input(g, *shape):
    """fp32 input of an mp_silu: 2 * randn, |x| <= 8 (the exponent's argument error stays small)"""
    return (torch.randn(*shape, generator=g) * 2).clamp_(-8.0, 8.0)


def short_mantissa(g, *shape):
    """fp32 values with 8 significant bits, magnitudes in [2^-8, ~2^4) or exactly 0: a four-term fp32 sum is exact (20 bits
    at most) whatever its order"""
    x = (torch.randn(*shape, generator=g) * 2).to(bf16).float()
    return torch.where(x.abs() < 2.0 ** -8, torch.zeros_like(x), x)


def bit_equal(y, ref, what):
    from parity_log import record
    y, ref = y.cpu(), ref.cpu()
    assert y.shape == ref.shape and y.dtype == ref.dtype, (what, y.shape, ref.shape, y.dtype, ref.dtype)
    if y.dtype in (torch.float32, bf16):         # (torch.equal would call +0 and -0 the same)
        same = torch.equal(y.view(torch.int32 if y.dtype == torch.float32 else torch.int16),
                           ref.view(torch.int32 if y.dtype == torch.float32 else torch.int16))
    else:
        same = torch.equal(y, ref)
    record(_name(what), 0.0 if same else 1.0, 0.0)
    assert same, f"{what}: not bit-equal"


def _per_element(y, ref, bound, what):
    from parity_log import record
    assert y.shape == ref.shape == bound.shape, (what, y.shape, ref.shape, bound.shape)
    assert torch.isfinite(y).all(), f"{what}: non-finite output"
    err = (y - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, 2.0), torch.zeros_like(err)))
    worst = ratio.max().item()
    record(_name(what), worst, 1.0)
    print(f"{_name(what)}: worst err/bound {worst:.3f}")
    if worst > 1.0:
        i = ratio.argmax().item()
        raise AssertionError(f"{what}: {(ratio > 1).sum().item()} of {ratio.numel()} elements over the bound; worst at flat index {i}: "
                             f"y={y.reshape(-1)[i].item():.9g} ref={ref.reshape(-1)[i].item():.9g} bound={bound.reshape(-1)[i].item():.3g}")


def check_f32(y, ref, l2, k, what, a=0.0):
    """fp32 output: relative L2 <= l2 (None: no L2 limit applies) and, every element, |y - ref| <= k U |ref| + a"""
    from parity_log import record
    assert y.dtype == torch.float32, what
    y = R.f64(y)
    assert y.shape == ref.shape and torch.isfinite(y).all(), f"{what}: shape or non-finite output"
    if l2 is not None:
        e = rel(y, ref)
        record(_name(what + ".l2"), e, l2)
        print(f"{_name(what)}: rel L2 {e:.3e} (limit {l2:.0e})")
        assert e <= l2, f"{what}: rel L2 {e:.3e}"
    _per_element(y, ref, k * U * ref.abs() + a, what)


def check_pairs(p, v, k, what, a=0.0):
    """pairs output [hi | lo] of a value whose fp64 reference is v and whose plain fp32 output is held to k U |v| + a:
    |hi + lo - v| <= 2^-17 |v| + k U |v| + a, and |lo| <= half a bf16 ulp of hi"""
    from parity_log import record
    assert p.dtype == bf16 and p.shape[:-1] == v.shape[:-1] and p.shape[-1] == 2 * v.shape[-1], (what, p.shape, v.shape)
    hi, lo = R.halves(p)
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all(), f"{what}: non-finite output"
    _per_element(hi + lo, v, (R.PAIR_REL + k * U) * v.abs() + a, what + ".value")
    over = (lo.abs() > R.half_ulp_bf16(hi)).sum().item()
    record(_name(what + ".hi_nearest"), float(over), 0.0)
    assert over == 0, f"{what}: {over} elements whose hi is not the bf16 nearest to hi + lo"


def restated_silu_ratio(x):
    """worst error of the fp32 restatement of mp_silu on x, in units of U |ref| (printed next to each case, never asserted)"""
    ref = R.mp_silu(x).numpy()
    err = np.abs(R.mp_silu32(x).astype(np.float64) - ref)
    nz = ref != 0
    return float((err[nz] / (U * np.abs(ref[nz]))).max()) if nz.any() else 0.0


def check_silu(s, x, pairs, what, l2_ref=None, a=0.0):
    """s = mp_silu(x) from a kernel, x the fp32 tensor the kernel applied it to: per element SILU_K U |ref| (+ a); against
    l2_ref (the reference chain's own value) 2e-6 in relative L2 for the fp32 form"""
    from parity_log import record
    ref = R.mp_silu(x)
    print(f"{_name(what)}: fp32 restatement at {restated_silu_ratio(x):.2f} U |ref| (allowance {SILU_K:.2f})")
    if pairs:
        check_pairs(s, ref, SILU_K, what, a=a)
    else:
        check_f32(s, ref, 2e-6, SILU_K, what, a=a)
        if l2_ref is not None:
            e = rel(R.f64(s), l2_ref)
            record(_name(what + ".chain_l2"), e, 2e-6)
            assert e <= 2e-6, f"{what}: rel L2 {e:.3e} against the reference chain"


# ================================================================== pair format
def bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


def pair_format_values(g, n_random):
    """the inputs the pair format is pinned on: tie patterns, +-0, one ulp either side of a tie, magnitudes 2^-100 .. 2^100"""
    ties = []
    for sign in (0x00000000, 0x80000000):
        for expo in (0x3F800000, 0x00800000 + (27 << 23), 0x7E800000 - (27 << 23), 0x40400000):     # 1, 2^-99, 2^99, 3
            for upper in (0x00000000, 0x00010000, 0x007E0000, 0x007F0000):                          # even / odd upper mantissa bit
                tie = (sign | expo | upper | 0x8000) & 0xFFFFFFFF
                ties += [tie, tie + 1, tie - 1]
    special = bits(ties + [0x00000000, 0x80000000])
    e = torch.randint(-100, 101, (n_random,), generator=g).float()
    m = 1.0 + torch.rand(n_random, generator=g)
    sgn = torch.where(torch.rand(n_random, generator=g) < 0.5, -1.0, 1.0)
    rnd = sgn * m * torch.exp2(e)
    # half of the random values keep only 17 mantissa bits with the lowest set: exact ties of the lo half as well
    half = n_random // 2
    w = rnd[:half].numpy().view(np.uint32)
    rnd[:half] = torch.from_numpy(((w & np.uint32(0xFFFFFF80)) | np.uint32(0x40)).view(np.float32).copy())
    return torch.cat((special, rnd))


@pytest.mark.parametrize("C", [8, 16, 264])
def test_f32_to_pairs_is_the_cpu_restatement(ops, C):
    """k_f32_to_pairs: C = 8 one lane per row, 16 two, 264 thirty-three (row = i / CL, c8 = i % CL with CL not a power of two)"""
    g = gen("pairs", C)
    v = pair_format_values(g, 8192)
    rows = -(-v.numel() // C)
    x = torch.cat((v, torch.randn(rows * C - v.numel(), generator=g))).view(1, 1, rows, C)
    x = x.view(-1)[torch.randperm(x.numel(), generator=g)].view(1, 1, rows, C)
    assert torch.isfinite(x).all() and ((x == 0) | (x.abs() >= 2.0 ** -101)).all()
    bit_equal(ops.f32_to_pairs(dv(x)), R.pairs_of(x), "pairs")


SPLIT_PACK = [(I, taps, Cout) for I in (4, 32, 40, 96) for taps in (1, 9) for Cout in (3, 72)]


@pytest.mark.parametrize("I,taps,Cout", SPLIT_PACK)
def test_split_pack_is_the_cpu_restatement(ops, I, taps, Cout):
    """k_split_pack: I = 4 / 40 / 96 pad to Ip = 32 / 64 / 96 (zero columns in all three thirds), I = 32 has none; taps = 9
    reads w_hat with stride 9; also the out= form into a NaN-filled buffer (every element, padding included, is written)"""
    g = gen("pack", I, taps, Cout)
    n = Cout * I * taps
    v = pair_format_values(g, n)
    w = v[torch.randperm(v.numel(), generator=g)[:n]].view(Cout, I * taps).contiguous()
    ref = R.split_pack_ref(w, taps)
    bit_equal(ops.split_pack(dv(w), taps), ref, "pack")
    out = torch.full(ref.shape, float("nan"), dtype=bf16, device=DEV)
    assert ops.split_pack(dv(w), taps, out=out) is out
    bit_equal(out, ref, "pack_out")


# ================================================================== pixel norm + mp_silu, and the pooled form
PN_C = [4, 252, 256, 260, 768, 1024]
PN_P = [1, 3, 5]
PN_OVER = 16384 + 3


def norm_k(C):
    """relative error of x * (1 / (eps + sqrt(sum_C v^2) / sqrt(C))) in fp32: C squares and C - 1 additions of non-negative terms,
    any order: C U on the sum, halved by the square root; then sqrt, sqrt(C), divide, add, reciprocal, multiply: 6 U"""
    return C / 2 + 6


def _check_pnorm(x_row, xn, s, pairs, a_xn=None):
    """x_row: the fp64 row the norm is taken of.  xn against the reference; s against mp_silu of the STORED xn per element
    and against the reference chain in relative L2"""
    C = x_row.shape[-1]
    xn_ref, s_ref = R.pixelnorm_silu(x_row)
    check_f32(xn, xn_ref, 1e-6, norm_k(C), "xn", a=0.0 if a_xn is None else a_xn)
    assert R.f64(xn).abs().max().item() <= 8.0
    check_silu(s, xn.cpu(), pairs, "s", l2_ref=s_ref)


@pytest.mark.parametrize("pairs", [False, True], ids=["f32", "pairs"])
@pytest.mark.parametrize("C,P", [(C, P) for C in PN_C + [1028] for P in PN_P] + [(4, PN_OVER)])
def test_pixelnorm_silu_edges(ops, C, P, pairs):
    x = silu_input(gen("pn", C, P), 1, 1, P, C)
    xn, s = ops.f32_pixelnorm_silu(dv(x), pairs=pairs)
    _check_pnorm(R.f64(x), xn, s, pairs)


def _pool_case(ops, x, pairs):
    """pooled form on a random fp32 input.  The pooled row carries dp = 3 U mean|.| per element (below); to first order that
    moves xn = p / d(p) by dp / d + |xn| |dp|_2 / |p|_2 (the row's own error, and the norm's relative change)"""
    xn, s = ops.f32_pool_pixelnorm_silu(dv(x), pairs=pairs)
    x64 = R.f64(x)
    p = R.pool2(x64)
    C = p.shape[-1]
    dp = 3 * U * R.pool2(x64.abs())
    d = R.NORM_EPS + p.square().sum(-1, keepdim=True).sqrt() / math.sqrt(C)
    xn_ref = p / d
    a = dp / d + xn_ref.abs() * dp.square().sum(-1, keepdim=True).sqrt() / p.square().sum(-1, keepdim=True).sqrt().clamp_min(1e-300)
    _check_pnorm(p, xn, s, pairs, a_xn=a)
    # the fused form is the two-kernel sequence, bit for bit
    xn0, s0 = ops.f32_pixelnorm_silu(ops.f32_pool2(dv(x)), pairs=pairs)
    bit_equal(xn, xn0, "xn==pool>norm")
    bit_equal(s, s0, "s==pool>norm")


@pytest.mark.parametrize("pairs", [False, True], ids=["f32", "pairs"])
@pytest.mark.parametrize("P", PN_P)
@pytest.mark.parametrize("C", PN_C)
def test_pool_pixelnorm_silu_edges(ops, C, P, pairs):
    _pool_case(ops, silu_input(gen("ppn", C, P), 1, 2, 2 * P, C), pairs)


@pytest.mark.parametrize("pairs", [False, True], ids=["f32", "pairs"])
def test_pool_pixelnorm_silu_over_cap(ops, pairs):
    _pool_case(ops, silu_input(gen("ppno"), 1, 2, 2 * PN_OVER, 4), pairs)


def test_pool_pixelnorm_silu_two_rows_and_samples(ops):
    """B = 2, 3 x 5 output pixels: the (b, h, w) decomposition of the output pixel and the row stride 2 W C of the input"""
    _pool_case(ops, silu_input(gen("ppn2"), 2, 6, 10, 260), True)


# ================================================================== flat quad kernels
FLAT_SHAPES = [(1, 1, 1, 4), (3, 1, 1, 8), (2, 3, 5, 12), (1, 1, OVER_QUADS, 4)]


@pytest.mark.parametrize("pairs", [False, True], ids=["f32", "pairs"])
@pytest.mark.parametrize("shape", FLAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_silu_edges(ops, shape, pairs):
    x = silu_input(gen("silu", shape, pairs), *shape)
    check_silu(ops.f32_silu(dv(x), pairs=pairs), x, pairs, "s")


@pytest.mark.parametrize("shape", FLAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool2_edges(ops, shape):
    """`shape` is the OUTPUT shape.  Short-mantissa input: bit-equal to the fp64 mean rounded to fp32; random input:
    |err| <= 3 U mean(|a|,|b|,|c|,|d|) (three additions, each within U of a partial sum that the sum of magnitudes bounds)"""
    B, H, W, C = shape
    g = gen("pool", shape)
    xs = short_mantissa(g, B, 2 * H, 2 * W, C)
    bit_equal(ops.f32_pool2(dv(xs)), R.pool2(xs).float(), "exact")
    assert torch.equal(R.pool2(xs).float().double(), R.pool2(xs))            # (the mean of such inputs IS an fp32 number)
    x = torch.randn(B, 2 * H, 2 * W, C, generator=g)
    check_f32(ops.f32_pool2(dv(x)), R.pool2(x), None, 0.0, "random", a=3 * U * R.pool2(x.abs()))


UP_IN_SHAPES = [(1, 1, 1, 4), (3, 1, 1, 8), (2, 3, 5, 12), (1, 1, (OVER_QUADS + 3) // 4, 4)]      # INPUT shapes: 4x the quads


@pytest.mark.parametrize("shape", UP_IN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_up2_and_up2_silu_edges(ops, shape):
    g = gen("up", shape)
    x = silu_input(g, *shape)
    x.view(-1)[0] = -0.0                                                      # a copy keeps the sign of zero
    y_ref = R.up2(x).float()
    y0 = ops.f32_up2(dv(x))
    bit_equal(y0, y_ref, "up2")
    for pairs in (False, True):
        y, s = ops.f32_up2_silu(dv(x), pairs=pairs)
        bit_equal(y, y_ref, f"up2_silu.y[pairs={pairs}]")
        check_silu(s, y_ref, pairs, f"up2_silu.s[pairs={pairs}]")
        bit_equal(s, ops.f32_silu(y0, pairs=pairs), f"s==up>silu[pairs={pairs}]")


# (B, H, W, Ci, Cs): one pixel with the smallest halves; B = 3 at HW = 1; the three channel splits; over-cap
CAT_SHAPES = [(1, 1, 1, 4, 4), (3, 1, 1, 4, 4), (3, 1, 1, 192, 40), (2, 3, 5, 192, 40), (3, 1, 1, 64, 768), (2, 3, 5, 64, 768),
              (2, 1, (OVER_QUADS + 5) // 4, 4, 4)]


def _cat_inputs(shape):
    B, H, W, Ci, Cs = shape
    g = gen("cat", shape)
    inp, skip = silu_input(g, B, H, W, Ci), silu_input(g, B, H, W, Cs)
    gate = torch.rand(B, Cs, generator=g) * 0.98 + 0.01
    return inp, skip, gate


def _silu_of_product_a(v):
    """mp_silu of a product rounded to fp32 (|dv| <= U |v|) against mp_silu of the exact product: |mp_silu'(v)| U |v|"""
    return R.mp_silu_grad(v).abs() * U * v.abs()


@pytest.mark.parametrize("pairs", [False, True], ids=["f32", "pairs"])
@pytest.mark.parametrize("want_silu", [False, True], ids=["cat", "cat+silu"])
@pytest.mark.parametrize("shape", CAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_concat_gate_edges(ops, shape, want_silu, pairs):
    """cat: the input half is a copy (bit-equal; as pairs, bit-equal to pairs_of), the skip half one multiply: k = 1.
    sil: mp_silu of the stored cat (fp32 form); as pairs, of the exact product, whose rounding adds _silu_of_product_a"""
    B, H, W, Ci, Cs = shape
    inp, skip, gate = _cat_inputs(shape)
    cat, sil = ops.f32_concat_gate(dv(inp), dv(skip), dv(gate), want_silu, pairs=pairs)
    assert (sil is not None) == want_silu
    cat_ref, _ = R.concat_gate(inp, skip, gate)
    Ct = Ci + Cs
    if pairs:
        bit_equal(torch.cat((cat[..., :Ci], cat[..., Ct:Ct + Ci]), -1), R.pairs_of(inp), "cat.input_half")
        check_pairs(cat, cat_ref, 1.0, "cat")
        if want_silu:
            bit_equal(torch.cat((sil[..., :Ci], sil[..., Ct:Ct + Ci]), -1), ops.f32_silu(dv(inp), pairs=True), "sil.input_half==silu")
            check_silu(sil, cat_ref.float(), True, "sil", a=_silu_of_product_a(cat_ref))
    else:
        bit_equal(cat[..., :Ci], inp, "cat.input_half")
        check_f32(cat, cat_ref, 2e-6, 1.0, "cat")
        if want_silu:
            check_silu(sil, cat.cpu(), False, "sil", l2_ref=R.mp_silu(cat_ref))


@pytest.mark.parametrize("with_sil", [False, True], ids=["cat", "cat+sil"])
@pytest.mark.parametrize("shape", CAT_SHAPES[:-1] + [(1, 1, OVER_QUADS, 4, 4)], ids=lambda s: "x".join(map(str, s)))
def test_skip_half_edges(ops, shape, with_sil):
    """into NaN-filled cat / sil: the input-half columns stay NaN (nothing else is written), the skip-half columns are the
    pairs of skip * gate (one multiply, k = 1) and of mp_silu of it"""
    B, H, W, Ci, Cs = shape
    _, skip, gate = _cat_inputs(shape)
    Ct = Ci + Cs
    cat = torch.full((B, H, W, 2 * Ct), float("nan"), dtype=bf16, device=DEV)
    sil = torch.full_like(cat, float("nan")) if with_sil else None
    ops.f32_skip_half(dv(skip), dv(gate), cat, sil)
    v = R.skip_half(skip, gate)
    for name, t, chk in (("cat", cat, lambda q: check_pairs(q, v, 1.0, "cat.skip_half")),
                         ("sil", sil, lambda q: check_silu(q, v.float(), True, "sil.skip_half",
                                                           a=_silu_of_product_a(v)))):
        if t is None:
            continue
        t = t.cpu()
        assert torch.isnan(t[..., :Ci].float()).all() and torch.isnan(t[..., Ct:Ct + Ci].float()).all(), f"{name}: input half written"
        chk(torch.cat((t[..., Ci:Ct], t[..., Ct + Ci:]), -1))


# ================================================================== ScaleLong gate
GATE_C = [4, 40, 192, 576, 1028, 4096]
GATE_BHW = [(B, H, W) for B in (1, 3) for H, W in ((1, 1), (3, 1), (7, 7), (32, 32))]      # B x HW in {1, 3, 49, 1024}


def gate_case(C, Rn, bhw, draw=0):
    B, H, W = bhw
    g = gen("gate", C, Rn, bhw) if draw == 0 else gen("gate", C, Rn, bhw, draw)
    skip = torch.randn(B, H, W, C, generator=g)
    w1h = O.effective_weight(torch.randn(Rn, C + 1, 1, 1, generator=g)).view(Rn, C + 1).contiguous()
    w2h = O.effective_weight(torch.randn(C, Rn, 1, 1, generator=g)).view(C, Rn).contiguous()
    return skip, w1h, w2h


def gate_cases():
    """the whole cross, less B = 3 at HW = 1024 and C = 4096 (a 50 MB skip; B = 1 there is the 16 MB ceiling of this file)"""
    return [(C, Rn, bhw) for C in GATE_C for Rn in sorted({1, max(1, C // 16)}) for bhw in GATE_BHW
            if bhw[0] * bhw[1] * bhw[2] * C <= 4 << 20]


def restated_gate_ratio(skip, w1h, w2h):
    """worst error of the fp32 restatement of the gate, in units of U |ref|"""
    ref = R.skip_gate(skip, w1h, w2h).numpy()
    return float((np.abs(R.skip_gate32(skip, w1h, w2h).astype(np.float64) - ref) / (U * ref)).max())


@pytest.mark.parametrize("C,Rn,bhw", gate_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_skip_gate_edges(ops, C, Rn, bhw):
    skip, w1h, w2h = gate_case(C, Rn, bhw)
    gate = ops.f32_skip_gate(dv(skip), dv(w1h), dv(w2h))
    ref = R.skip_gate(skip, w1h, w2h)
    assert 1 / (1 + math.exp(8)) <= ref.min().item() and ref.max().item() <= 1 / (1 + math.exp(-8))     # both exponents within +-8
    k = 4 * MEASURED_GATE[(C, Rn)][GATE_BHW.index(bhw)]
    print(f"{_name('gate')}: fp32 restatement here at {restated_gate_ratio(skip, w1h, w2h):.2f} U |ref| (allowance {k:.2f})")
    check_f32(gate, ref, 2e-6, k, "gate")


# ================================================================== preconditioning in / conv_out
SIGMAS = [0.002, 1.0, 80.0]
SD = 0.5            # exact in fp32, like its square


def _sigma(mode, B):
    if mode == "per-sample":
        return torch.tensor([SIGMAS[b % 3] for b in range(B)])
    return torch.tensor([mode])


def _check_precond_in(ops, noisy, sigma, Cimg):
    """c_in = 1 / sqrt(sd^2 + s^2): s * s, the sum (sd^2 exact), sqrt (halves the 2 U, adds 1), reciprocal, the product with
    noisy: k = 5.  The 1 and the 0 channels are constants: bit-equal"""
    out = ops.f32_precond_in(dv(noisy), dv(sigma), SD, 8)
    ref = R.precond_in(noisy, sigma, SD, 8)
    check_f32(out[..., :Cimg].contiguous(), ref[..., :Cimg], 1e-6, 5.0, "c_in*noisy")
    bit_equal(out[..., Cimg:], ref[..., Cimg:].float(), "one_and_zeros")
    check_f32(out, ref, 1e-6, 5.0, "all")


@pytest.mark.parametrize("mode", SIGMAS + ["per-sample"])
@pytest.mark.parametrize("hw", [(1, 1), (7, 7)], ids=["hw1", "hw49"])
@pytest.mark.parametrize("Cimg", [1, 3, 4])
def test_precond_in_edges(ops, Cimg, hw, mode):
    B = 3
    noisy = torch.randn(B, Cimg, *hw, generator=gen("pin", Cimg, hw, mode)) * 3
    _check_precond_in(ops, noisy, _sigma(mode, B), Cimg)


@pytest.mark.parametrize("mode", [1.0, "per-sample"])
def test_precond_in_over_cap(ops, mode):
    noisy = torch.randn(3, 1, 349527, 1, generator=gen("pino", mode)) * 3           # 1 048 581 pixels
    _check_precond_in(ops, noisy, _sigma(mode, 3), 1)


CO_PIX = [(1, 1, 1), (3, 1, 1), (1, 5, 1), (3, 1, 5), (1, 17, 1)]                    # B*HW = 1, 3, 5, 15, 17


def _check_conv_out(ops, g, bhw, C, Co, mode, what, l2=2e-6):
    """acc = sum_c x w in any order: C products and C - 1 additions, C U sum|x w|; * gain * c_out: 2 U, c_out itself 5 U
    (s s, the sum, sqrt, s sd, divide): (C + 7) U S gain c_out with S = sum|x||w| >= |acc|.  noisy * c_skip: 1 U, c_skip 4 U
    (s s, sum, divide; sd^2 exact): 5 U |noisy| c_skip.  The final addition: U |D|."""
    B, H, W = bhw
    x = torch.randn(B, H, W, C, generator=g)
    wh = torch.randn(Co, C, generator=g) / math.sqrt(C)
    noisy = torch.randn(B, Co, H, W, generator=g) * 3
    sigma = _sigma(mode, B)
    go = torch.tensor(0.9)
    D = ops.f32_conv_out(dv(x), dv(wh), dv(go), dv(noisy), dv(sigma), SD)
    ref = R.conv_out(x, wh, go.item(), noisy, sigma, SD)
    c_skip, c_out, _ = R.precond_scalars(sigma, SD, B)
    S = torch.einsum("bhwc,oc->bohw", R.f64(x).abs(), R.f64(wh).abs())
    a = U * ((C + 7) * S * float(go.double()) * c_out[:, None, None, None] + 5 * R.f64(noisy).abs() * c_skip[:, None, None, None])
    check_f32(D, ref, l2, 1.0, what, a=a)
    return R.f64(D).reshape(-1), ref.reshape(-1)


@pytest.mark.parametrize("mode", SIGMAS + ["per-sample"])
@pytest.mark.parametrize("C", [4, 60, 64, 68, 768])
def test_conv_out_edges(ops, C, mode):
    """every Co and pixel count at this C and sigma: each launch is held per element, and the case -- all of its launches'
    outputs together, a launch of one pixel being a handful of numbers -- to 2e-6 in relative L2"""
    from parity_log import record
    outs = [_check_conv_out(ops, gen("co", C, mode, Co, bhw), bhw, C, Co, mode, f"D[Co={Co},{'x'.join(map(str, bhw))}]", l2=None)
            for Co in (1, 3, 4, 8) for bhw in CO_PIX]
    e = rel(torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]))
    record(_name("D.l2"), e, 2e-6)
    assert e <= 2e-6, e


@pytest.mark.parametrize("mode", [1.0, "per-sample"])
@pytest.mark.parametrize("Co", [3, 8])
def test_conv_out_over_cap(ops, Co, mode):
    _check_conv_out(ops, gen("coo", Co, mode), (3, 21847, 1), 4, Co, mode, "D")      # 65 541 pixels


# ================================================================== layout changes
@pytest.mark.parametrize("shape", [(2, C, h, w) for C in (1, 3, 8) for h, w in ((1, 1), (7, 7))] + [(3, 1, 349527, 1), (1, 3, 5, 69907)],
                         ids=lambda s: "x".join(map(str, s)))
def test_layout_edges(ops, shape):
    x = torch.randn(*shape, generator=gen("layout", shape))           # NCHW
    y = ops.f32_nchw_to_nhwc(dv(x))
    bit_equal(y, R.nchw_to_nhwc(x).float(), "nchw_to_nhwc")
    z = torch.randn(shape[0], shape[2], shape[3], shape[1], generator=gen("layout2", shape))      # NHWC
    bit_equal(ops.f32_nhwc_to_nchw(dv(z)), R.nhwc_to_nchw(z).float(), "nhwc_to_nchw")


# ================================================================== refusals
SENTINEL = 1536.0          # (a bf16 number as well)


def _sent(*shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, dtype=dtype, device=DEV)


def _untouched(*ts):
    return all(bool((t.float() == SENTINEL).all()) for t in ts)


def test_refusals_raise_before_any_launch(ops):
    """host checks: C % 4 != 0 (every quad kernel), odd H or W for the pool, C > 1024 for the pooled norm, C % 8 != 0 for
    f32_to_pairs.  The wrappers raise, and so do the entry points themselves, with their sentinel-filled outputs untouched"""
    from tinyedm_amd import _lib
    from tinyedm_amd.ops import _p, _stream
    g = gen("refuse")
    x6 = dv(torch.randn(1, 2, 2, 6, generator=g))
    # (the plain f32_silu is flat: it needs numel % 4 only; its pairs form needs rows of whole quads)
    for fn in (ops.f32_pixelnorm_silu, lambda t: ops.f32_silu(t, pairs=True), lambda t: ops.f32_silu(t[:, :1, :1].contiguous()),
               ops.f32_pool2, ops.f32_up2, ops.f32_up2_silu, ops.f32_pool_pixelnorm_silu):
        with pytest.raises(Exception):
            fn(x6)
    gate6 = dv(torch.rand(1, 6, generator=g))
    x8 = dv(torch.randn(1, 2, 2, 8, generator=g))
    with pytest.raises(Exception):
        ops.f32_concat_gate(x8, x6, gate6, True)
    with pytest.raises(Exception):
        ops.f32_skip_gate(x6, dv(torch.randn(1, 7, generator=g)), dv(torch.randn(6, 1, generator=g)))
    cat, sil = _sent(1, 2, 2, 28, dtype=bf16), _sent(1, 2, 2, 28, dtype=bf16)
    with pytest.raises(Exception):
        ops.f32_skip_half(x6, gate6, cat, sil)
    assert _untouched(cat, sil)
    with pytest.raises(Exception):
        ops.f32_conv_out(x6, dv(torch.randn(3, 6, generator=g)), dv(torch.tensor(0.9)), dv(torch.randn(1, 3, 2, 2, generator=g)),
                         dv(torch.tensor([1.0])), SD)
    # odd H or W for the pool and the pooled norm; C > 1024 for the pooled norm; C % 8 for the pairs
    for shape in ((1, 3, 2, 8), (1, 2, 3, 8)):
        xo = dv(torch.randn(*shape, generator=g))
        for fn in (ops.f32_pool2, ops.f32_pool_pixelnorm_silu):
            with pytest.raises(ValueError):
                fn(xo)
    with pytest.raises(ValueError):
        ops.f32_pool_pixelnorm_silu(dv(torch.randn(1, 2, 2, 1028, generator=g)))
    for C in (4, 12):
        with pytest.raises(ValueError):
            ops.f32_to_pairs(dv(torch.randn(1, 1, 3, C, generator=g)))
    # the entry points' own checks
    a, b = _sent(64), _sent(64)
    pb = _sent(128, dtype=bf16)
    xin = dv(torch.randn(4 * 1028, generator=g))
    for name, args in (("edm_f32_pixelnorm_silu", (_p(xin), _p(a), _p(b), 4, 6, 0, _stream())),
                       ("edm_f32_silu", (_p(xin), _p(a), 6, 0, _stream())),
                       ("edm_f32_pool2", (_p(xin), _p(a), 1, 1, 1, 6, _stream())),
                       ("edm_f32_up2", (_p(xin), _p(a), 1, 2, 2, 6, _stream())),
                       ("edm_f32_up2", (_p(xin), _p(a), 1, 3, 2, 4, _stream())),
                       ("edm_f32_up2_silu", (_p(xin), _p(a), _p(b), 1, 2, 3, 4, 0, _stream())),
                       ("edm_f32_pool_pixelnorm_silu", (_p(xin), _p(a), _p(b), 1, 1, 1, 1028, 0, _stream())),
                       ("edm_f32_pool_pixelnorm_silu", (_p(xin), _p(a), _p(b), 1, 1, 1, 6, 0, _stream())),
                       ("edm_f32_concat_gate", (_p(xin), _p(xin), _p(xin), _p(a), _p(b), 1, 1, 4, 6, 0, _stream())),
                       ("edm_f32_skip_half", (_p(xin), _p(xin), _p(pb), _p(pb), 1, 1, 6, 4, _stream())),
                       ("edm_f32_skip_gate", (_p(xin), _p(xin), _p(xin), _p(a), 1, 1, 6, 1, _stream())),
                       ("edm_f32_conv_out", (_p(xin), _p(xin), _p(xin), _p(xin), _p(xin), 0, SD, _p(a), 1, 1, 6, 3, _stream())),
                       ("edm_f32_to_pairs", (_p(xin), _p(pb), 2, 12, _stream()))):
        with pytest.raises(_lib.HipKernelError):
            _lib.call(name, *args)
    torch.cuda.synchronize()
    assert _untouched(a, b, pb)
