"""Integer operands for the MFMA convolution family and their plain fp64 references.

The conv and weight-gradient kernels are linear with fp32 accumulation.  Fed small integers, every product and every
partial sum is an integer far below 2^24, so the fp32 result does not depend on summation order, split count, tile walk
or team schedule, and every output is representable in the output type: the kernel must reproduce the fp64 reference
bit for bit, and a missing, duplicated or misplaced term moves some output by at least 1.

Recipes (tests/test_conv_exact_cpu.py checks the conditions on every case the GPU file runs):
  forward / dgrad    x = {-1, 0, 1} * bernoulli(p), p = min(1, 256 / K) with K the reduction length, w = +-1 dense
                     -> |ref| <= 128 and ref == bf16(ref), also after alpha = 0.5 (half-integers below 128 have 8 bits)
  weight gradient    x, dy dense in {-2..2} -> |sum| <= 4 * B * H * W < 2^24
Shape lists are read from the tests they extend, so the two cannot drift apart.  Everything here runs on the CPU; operands
are cached per case (module scope) and shared by the kernel generations that run them."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

import test_kernels_gpu as K
import test_wgrad3_gpu as W3
from oracle import edm_oracle as O

bf16 = torch.bfloat16


def _cases(fn, names):
    """the argvalues of fn's @pytest.mark.parametrize(names, ...)"""
    for m in fn.pytestmark:
        if m.name == "parametrize" and m.args[0] == names:
            return list(m.args[1])
    raise LookupError(f"{fn.__name__} has no parametrize over {names!r}")


def _gen(*key):
    """generator seeded by a fixed polynomial mix of the key (the same tensors on every interpreter and machine)"""
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _tern(shape, p, g):
    """{-1, 0, 1} * bernoulli(p)"""
    t = torch.randint(-1, 2, shape, generator=g).float()
    return t if p >= 1.0 else t * (torch.rand(shape, generator=g) < p).float()


def _sign(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def _ints(shape, lim, g):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def is_bf16_exact(t):
    return torch.equal(t.double(), t.to(bf16).double())


def conv_nhwc_f64(x, wp, taps):
    """x (B, H, W, Cin), wp (taps, Cout, Cin) in the forward pack's order (tap = ky * k + kx) -> fp64 (B, H, W, Cout)"""
    k = 3 if taps == 9 else 1
    w = wp.double().view(k, k, wp.shape[1], wp.shape[2]).permute(2, 3, 0, 1)
    return F.conv2d(x.double().permute(0, 3, 1, 2), w, padding=k // 2).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------ 1. forward conv, every generation
IGEMM_VERSIONS = [0, 1, 2, 5, 6]
IGEMM_IDS = {0: "auto", 1: "v1", 2: "v2", 5: "s", 6: "v6"}

CONV_SHAPES = list(K.CONV_SHAPES)
BORDER_SHAPES = _cases(K.test_conv3x3_v6_border_paths, "B,H,W,Cin,Cout,imgs")
# degenerate maps: one pixel per image, fewer pixels than any tile, a single row, W = 64 with three rows, an odd width
# past 32; each on the generations whose covers-rule admits it (forcing another one would only run kernel 1 again)
DEGENERATE = [(3, 1, 1, 64, 64), (2, 2, 2, 64, 72), (1, 1, 16, 256, 64), (2, 3, 64, 64, 64), (1, 2, 33, 64, 64)]


def covers(version, W, Cin, taps):
    """What this file expects of the kernels' covers-rules (edm_conv_v2_covers, edm_conv_s_covers, edm_conv_v6_covers): the
    forced generation runs the shape itself -- otherwise the plan hands it to kernel 1.  Written out here, not asked of the
    library, so that a case cannot pass on another kernel than the one it names after a rule changes
    (tests/test_conv_exact_cpu.py holds this table against edm_conv_plan; the GPU test holds the launch against it)."""
    return {1: True,
            2: taps == 1 or W <= 64,
            5: taps == 9 and Cin % 256 == 0 and Cin <= 2016 and W <= 16,
            6: taps == 9 and Cin % 64 == 0 and Cin <= 2016 and W <= 64}[version]


def expected_kernel(version, W, Cin, taps):
    """kernel id a forced case must run on (None for the automatic plan, which depends on how well the shape fills the chip)"""
    return None if version == 0 else version if covers(version, W, Cin, taps) else 1

ConvCase = namedtuple("ConvCase", "x wp ref imgs")      # x bf16 NHWC, wp bf16 pack, ref fp64 NHWC of the images `imgs`


@functools.lru_cache(maxsize=None)
def conv_case(B, H, W, Cin, Cout, taps, imgs=None):
    g = _gen(1, B, H, W, Cin, Cout, taps)
    x = _tern((B, H, W, Cin), min(1.0, 256.0 / (taps * Cin)), g)
    wp = _sign((taps, Cout, Cin), g)
    sel = list(range(B)) if imgs is None else list(imgs)
    return ConvCase(x.to(bf16), wp.to(bf16), conv_nhwc_f64(x[sel], wp, taps), sel)


def forward_cases():
    """(B, H, W, Cin, Cout, taps, version, imgs, kernel): every case of the forward test; kernel = expected_kernel(...).
    CONV_SHAPES and the border shapes force every generation at taps 9 and 1, as the igemm_version fixture of
    test_kernels_gpu does (a generation that does not cover the shape runs kernel 1); the degenerate maps run only where
    the forced generation covers them."""
    out = []
    for (B, H, W, Cin, Cout, imgs) in [s + (None,) for s in CONV_SHAPES] + BORDER_SHAPES:
        imgs = None if imgs is None else tuple(imgs)
        for taps in (9, 1):
            out += [(B, H, W, Cin, Cout, taps, v, imgs, expected_kernel(v, W, Cin, taps)) for v in IGEMM_VERSIONS]
    for (B, H, W, Cin, Cout) in DEGENERATE:
        for taps in (9, 1):
            out += [(B, H, W, Cin, Cout, taps, v, None, expected_kernel(v, W, Cin, taps)) for v in IGEMM_VERSIONS
                    if v == 0 or covers(v, W, Cin, taps)]
    return out


def forward_id(c):
    B, H, W, Cin, Cout, taps, v = c[:7]
    return f"{B}x{H}x{W}x{Cin}-{Cout}-t{taps}-{IGEMM_IDS[v]}"


# ------------------------------------------------------------------ 2. linear epilogues
ALPHA, BETA, RES_LIM = 0.5, 2.0, 8
# (B, H, W, Cin, Cout, taps): the existing residual test's shape, ragged pixel and channel tiles, a 1x1, more than one tile
RESIDUAL_SHAPES = [(2, 16, 16, 128, 128, 9), (5, 7, 7, 256, 72, 9), (3, 5, 7, 128, 72, 1), (1, 32, 32, 64, 128, 9)]
# every generation that has the output-descriptor form, at the small shapes of test_conv_output_descriptor
DESCRIPTOR_CASES = [c for c in _cases(K.test_conv_output_descriptor, "B,H,W,Cin,Cout,taps,version") if c[0] < 128]


@functools.lru_cache(maxsize=None)
def residual_case(B, H, W, Cin, Cout, taps):
    """(conv case, r bf16 NHWC, fp64 ALPHA * conv + BETA * r)"""
    c = conv_case(B, H, W, Cin, Cout, taps)
    r = _ints((B, H, W, Cout), RES_LIM, _gen(2, B, H, W, Cin, Cout, taps))
    return c, r.to(bf16), ALPHA * c.ref + BETA * r.double()


FOLD_A3, FOLD_A1 = 0.5, 2.0
# the layers of test_conv3x3_fold_skip_projection, each at the smallest B for which conv3x3_fold_supported still holds (the
# fold needs enough tiles to fill the chip; tests/test_conv_exact_cpu.py checks that B - 1 is refused), with the reference
# on the first and last image and on the two in the middle
FOLD_MIN_B = [32, 127, 76, 505]
FOLD_FULL_SHAPES = _cases(K.test_conv3x3_fold_skip_projection, "B,H,W,Cin,Cout,C2,imgs")
FOLD_SHAPES = [(B, H, W, Cin, Cout, C2, [0, B // 2 - 1, B // 2, B - 1])
               for B, (_, H, W, Cin, Cout, C2, _) in zip(FOLD_MIN_B, FOLD_FULL_SHAPES)]

FoldCase = namedtuple("FoldCase", "x wp x2 w2p ref imgs")


@functools.lru_cache(maxsize=None)
def fold_case(B, H, W, Cin, Cout, C2, imgs):
    """FOLD_A3 * conv3x3(x, wp) + FOLD_A1 * conv1x1(x2, w2p): one reduction of 9 * Cin + C2 terms, so both inputs take the
    density of that length (the reference stays an integer or half-integer below 128)"""
    g = _gen(3, B, H, W, Cin, Cout, C2)
    p = min(1.0, 256.0 / (9 * Cin + C2))
    x, x2 = _tern((B, H, W, Cin), p, g), _tern((B, H, W, C2), p, g)
    wp, w2p = _sign((9, Cout, Cin), g), _sign((1, Cout, C2), g)
    sel = list(imgs)
    ref = FOLD_A3 * conv_nhwc_f64(x[sel], wp, 9) + FOLD_A1 * conv_nhwc_f64(x2[sel], w2p, 1)
    return FoldCase(x.to(bf16), wp.to(bf16), x2.to(bf16), w2p.to(bf16), ref, sel)


# ------------------------------------------------------------------ 3. raw weight-gradient slabs
WGRAD_LIM = 2
RAGGED_1X1 = _cases(K.test_conv_wgrad_1x1_ragged, "B,H,W,Cin,Cout")
WIDE_3X3 = _cases(K.test_conv_wgrad_wide_images, "B,H,W,Cin,Cout")
# (B, H, W, Cin, Cout, taps)
WGRAD_CASES = ([s + (t,) for s in K.CONV_SHAPES[:6] for t in (9, 1)]        # the shapes of test_weight_prep_dgrad_and_wgrad
               + [s + (1,) for s in RAGGED_1X1] + [s + (9,) for s in WIDE_3X3])
# the grouped 1x1 launch: the first five of test_wgrad1x1_grouped_launch_matches_per_layer_kernels (they are the ragged
# list) and one repeat; its B = 128 entries stay with that test
GROUP_1X1 = RAGGED_1X1 + RAGGED_1X1[:1]

WgradCase = namedtuple("WgradCase", "x dy ref")        # x, dy bf16 NHWC; ref fp64 (taps, Cout, Cin), packed order


@functools.lru_cache(maxsize=None)
def wgrad_case(B, H, W, Cin, Cout, taps, salt=0):
    g = _gen(4, B, H, W, Cin, Cout, taps, salt)
    x, dy = _ints((B, H, W, Cin), WGRAD_LIM, g), _ints((B, H, W, Cout), WGRAD_LIM, g)
    return WgradCase(x.to(bf16), dy.to(bf16), wgrad_f64(x, dy, taps))


def wgrad_f64(x, dy, taps):
    """dW[t, co, ci] = sum over pixels of dy[p, co] * x[p + off(t), ci], fp64, NHWC operands"""
    Cin, Cout = x.shape[-1], dy.shape[-1]
    if taps == 1:
        return (dy.double().reshape(-1, Cout).t() @ x.double().reshape(-1, Cin)).view(1, Cout, Cin)
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), w, padding=1).backward(dy.double().permute(0, 3, 1, 2))
    return w.grad.permute(2, 3, 0, 1).reshape(9, Cout, Cin).contiguous()


def wgrad_sum_bound(B, H, W):
    return 4 * B * H * W


# ------------------------------------------------------------------ 4. grouped stream-K 3x3 weight gradient
def _with_B(group, Bs):
    return [dict(kw, B=B) for kw, B in zip(group, Bs)]


# per layer, the smallest B at which the plan still splits the layer's K range (the plan of a layer does not depend on its
# neighbours; tests/test_conv_exact_cpu.py checks that B - 1 no longer splits); the 256-channel layer never splits and stays
KSPLIT_MIN_B = [3, 9, 9, 4, 15, 3]
KSPLIT_WIDE_MIN_B = [3, 1]
W3_GROUPS = {
    "small": W3.GROUP_SMALL, "wide": W3.GROUP_WIDE, "teams": W3.GROUP_TEAMS,
    "ksplit": _with_B(W3.GROUP_KSPLIT, KSPLIT_MIN_B), "ksplit-wide": _with_B(W3.GROUP_KSPLIT_WIDE, KSPLIT_WIDE_MIN_B),
    "forty-three": (W3.GROUP_SMALL * 6)[:43],
}
W3_SPLIT_GROUPS = {"ksplit": W3.GROUP_KSPLIT, "ksplit-wide": W3.GROUP_KSPLIT_WIDE}      # reduced group -> the group it came from


def star_column(r, n):
    """column of the single 1.0 in master row r (n = I * 9 columns)"""
    return (7 * r + 3) % n


def one_hot_master(Cout, I):
    """Master weight whose every row is a single 1.0 at star_column(r): the projection of k_wgrad3_finish then reads
    ss = rn = 1 exactly, and away from that column the kernel's value is c0 * scale * G[e] (G the integer gradient)."""
    n = I * 9
    w = torch.zeros(Cout, n)
    r = torch.arange(Cout)
    w[r, star_column(r, n)] = 1.0
    return w.view(Cout, I, 3, 3)


W3Layer = namedtuple("W3Layer", "x dy wm g0 perm scale accumulate G ref c0 star")


def w3_layer(g, B, H, W, Cin, Cout, I=None, perm=False, scale=1.0, accumulate=False, master=None):
    """One layer of a group, as test_wgrad3_gpu._layer builds it but with integer operands and the one-hot master weight.
    G: the raw fp64 gradient w.r.t. the effective weight (exact integers, master order); ref: fp64 autograd through
    O.effective_weight, times scale, plus g0; c0 = 1 / (d sqrt(n)) of the one-hot row; star: mask of the e* elements.
    g0 (accumulate) is uniform in [-2, 2]: the bound of the GPU test needs |g0| <= 5 |c0 scale G| wherever G != 0.
    master: a callable (g, G) -> fp32 master weight (Cout, I, 3, 3) that replaces the one-hot rows; the reference is then
    weights_ref.project in fp64 (O.effective_weight takes its norm in fp32), and c0 / star are None."""
    I = Cin if I is None else I
    x = _ints((B, Cin, H, W), WGRAD_LIM, g)
    if I < Cin:
        x[:, I:] = 0.0
    dy = _ints((B, Cout, H, W), WGRAD_LIM, g)
    wm = one_hot_master(Cout, I)
    p = torch.randperm(Cout, generator=g) if perm else None
    dy_master = dy
    if p is not None:                               # packed output channel r is master output channel p[r]
        dy_master = torch.empty_like(dy)
        dy_master[:, p] = dy
    w64 = wm.double().clone().requires_grad_(True)
    what = O.effective_weight(w64)
    what.retain_grad()
    F.conv2d(x[:, :I].double(), what, padding=1).backward(dy_master.double())
    g0 = torch.rand(Cout, I, 3, 3, generator=g) * 4 - 2 if accumulate else torch.zeros(Cout, I, 3, 3)
    n = I * 9
    c0 = 1.0 / ((float(O.EPS) + 1.0 / n ** 0.5) * n ** 0.5)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(bf16)
    G, ref, star = what.grad.clone(), w64.grad * scale + g0.double(), wm.bool()
    if master is not None:                          # (after every draw of the default form: the operands stay the same)
        import weights_ref
        wm = master(g, G)
        ref = g0.double() + weights_ref.project(scale * G, wm.double())
        c0 = star = None
    return W3Layer(nhwc(x), nhwc(dy), wm, g0, None if p is None else p.to(torch.int32), scale, accumulate, G, ref, c0, star)


@functools.lru_cache(maxsize=None)
def w3_group(name):
    group = W3_GROUPS[name]
    g = _gen(5, len(group), sum(kw["B"] * kw["Cin"] for kw in group))
    return [w3_layer(g, **kw) for kw in group]


# ------------------------------------------------------------------ 5. weight packs
# (O, I, taps, Ipad, perm): conv_in's padded pack with a row permutation, 3x3 and 1x1 layers, a pack padded past a ragged I
PACK_CASES = [(64, 4, 9, 32, True), (192, 128, 9, None, False), (72, 64, 1, None, True), (64, 24, 9, 32, False),
              (256, 512, 1, None, False)]
