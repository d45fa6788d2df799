"""Plain fp64 references, rounding bounds and case tables for the weight side (csrc/weights.hip and the twin projection
of k_wgrad3_finish).  No GPU and no tinyedm_amd import: tests/test_weights_ref_cpu.py checks this file on the CPU,
tests/test_weights_gpu.py holds the kernels against it.

Operations (n = fan_in = I * taps, one norm per output row o, eps = 1e-4, a master weight is (O, I, taps) with taps = k * k):
  normalize_master   w / (eps + ||w_o|| / sqrt(n))                      the forced in-place normalisation of a training forward
  effective          normalize_master(w) / sqrt(n)                      w_hat, what every layer multiplies with
  project            gradient through w_hat:  c0 * (a - w * c1),  d = eps + ||w_o|| / sqrt(n),  c0 = 1 / (d sqrt(n)),
                     c1 = <a_o, w_o> / (d ||w_o|| sqrt(n));  a zero row has c1 = 0, so it is a / (eps sqrt(n))
  finish             g0 + project(scale * sum_s slabs[s, t, r, :I]) in master order, packed row r = master row perm[r]

Index maps from a master-order (O, I, taps) array `hat` (packed row r = master row perm[r], or r without a perm):
  pack_fwd           out[t, r, i]            = hat[perm[r], i, t],   (taps, O, Ipad), columns i >= I are zero
  pack_dgrad         out[taps - 1 - t, i, r] = hat[perm[r], i, t],   (taps, I, O): channels transposed, taps flipped
  pack_fwd_frag      element (co, ci, t) at [t][ci >> 5][co >> 5][(ci >> 4) & 1][32 * ((ci >> 3) & 1) + (co & 31)][ci & 7]
  pack_dgrad_frag    the same map with co and ci swapped and the taps flipped:
                     element (co, ci, t) at [taps - 1 - t][co >> 5][ci >> 5][(co >> 4) & 1][32 * ((co >> 3) & 1) + (ci & 31)][co & 7]
The two fragment-major maps need O % 32 == 0 and I % 32 == 0 and have no perm and no padding.

Bounds.  u = 2^-24 is the fp32 unit roundoff: one correctly rounded operation is within u of its exact result, relatively.
The library is built with -O3 -ffp-contract=fast and without fast-math, so `/` is the correctly rounded IEEE division
(u) and a contracted multiply-add rounds once where the bounds below allow two; sqrtf and rsqrtf are allowed 1 ulp = 2 u
(the HIP math-function accuracy table).  A sum of m terms in ANY order, partial sums in fp32, is within (m - 1) u of the
exact sum, relative to the sum of the magnitudes of its terms (first order in u; every bound below is doubled, which covers
the second-order terms for m u < 1e-3, i.e. for every n a 64 KiB row can hold).

  Normalisation.  ss = sum of n squares: n roundings of the products and n - 1 of the sums, all terms non-negative:
  (n + 1) u relative in any order.  rn = sqrtf(ss): (n + 1) u / 2 + 2 u.  r = rn * rsqrtf(n): + 2 u + u.  So
      e_r = ((n + 1) / 2 + 5) u
  d = eps + r: the error of r enters with weight r / d, the fp32 constant 1e-4f is within u of eps, the sum rounds once:
      e_d = e_r * r / d + 2 u
  master:  w * (1 / d): a division and a multiply:                       e_d + 2 u
  hat:     m * (rsqrtf(n) / d), d from the row m as stored:              e_d + 2 u (rsqrtf) + 2 u = e_d + 4 u
  Each is relative to the reference value, elementwise, and doubled.  A zero row gives d = eps and an exact zero.

  Projection.  a_e = scale * (sum of S slab values): (S - 1) u for the sum in any order, u for the multiply -- the issue's
  (S + 1) u is used:
      da_e   = (S + 1) u |scale| sum_s |slab_s,e|
  dot = sum_e a_e w_e, n products and n - 1 sums in any order, of the ROUNDED a_e:
      ddot   = (n + 2) u sum_e |a_e w_e| + sum_e da_e |w_e|
  ss, rn as above: e_rn = (n + 1) u / 2 + 2 u;  sqn = sqrtf(n): 2 u;  r = rn / sqn: u;  e_d = (e_rn + 3 u) r / d + 2 u.
      c0 = 1 / (d * sqn):            e_c0 = e_d + 2 u + u + u = e_d + 4 u
      c1 = dot / (d * rn * sqn):     dc1  = ddot / (d rn sqn) + |c1| (e_d + e_rn + 2 u + 2 u + u)
  result v = c0 * (a_e - w_e * c1), three roundings (product, difference, product):
      dv_e   = c0 (da_e + |w_e| dc1 + u |w_e c1| + u |a_e - w_e c1|) + (e_c0 + u) |v_e|
  and u |g0 + v| more when the kernel adds onto an old gradient.  Everything is a function of the inputs (sums of
  magnitudes), elementwise, and doubled.  For a zero row c1 = dc1 = 0 and r / d = 0.

For n in the thousands the worst-case elementwise bound is a few 1e-4 of the row's magnitude and would hide a lost eps on
the rows where eps matters least, so every check also requires a relative L2 error of at most 1e-5."""
import functools
import math
from collections import namedtuple

import torch

EPS = 1e-4
U = 2.0 ** -24
L2_LIMIT = 1e-5
f64 = torch.float64


# ------------------------------------------------------------------------------------------------ references
def _rows(w):
    return w.reshape(w.shape[0], -1)


def normalize_master(w64, eps=EPS):
    w = _rows(w64.to(f64))
    n = w.shape[1]
    return (w / (eps + w.norm(dim=1, keepdim=True) / math.sqrt(n))).reshape(w64.shape)


def effective(w64, eps=EPS):
    return normalize_master(w64, eps) / math.sqrt(_rows(w64).shape[1])


def project(a64, w64, eps=EPS):
    a, w = _rows(a64.to(f64)), _rows(w64.to(f64))
    n = w.shape[1]
    sqn = math.sqrt(n)
    rn = w.norm(dim=1, keepdim=True)
    d = eps + rn / sqn
    c0 = 1.0 / (d * sqn)
    dot = (a * w).sum(dim=1, keepdim=True)
    c1 = torch.where(rn > 0, dot / (d * rn.clamp_min(1e-300) * sqn), torch.zeros_like(dot))
    return (c0 * (a - w * c1)).reshape(w64.shape)


def _perm_index(perm, O):
    return torch.arange(O) if perm is None else perm.long()


def slab_sum(slabs64, I, taps, perm, scale):
    """scale * sum_s slabs[s, t, r, :I] in master order (O, I, taps)"""
    S, T, O, Ipad = slabs64.shape
    assert T == taps and Ipad >= I
    packed = scale * slabs64[..., :I].to(f64).sum(0)              # (taps, O, I), packed rows
    a = torch.empty(O, I, taps, dtype=f64)
    a[_perm_index(perm, O)] = packed.permute(1, 2, 0)
    return a


def finish(slabs64, w64, I, taps, perm, scale, g0):
    w = w64.to(f64).reshape(w64.shape[0], I, taps)
    return g0.to(f64).reshape(w.shape) + project(slab_sum(slabs64, I, taps, perm, scale), w)


# ------------------------------------------------------------------------------------------------ index maps
def pack_fwd(hat, taps, Ipad, perm):
    O = hat.shape[0]
    h = hat.reshape(O, -1, taps)
    I = h.shape[1]
    out = torch.zeros(taps, O, Ipad, dtype=hat.dtype)
    out[:, :, :I] = h[_perm_index(perm, O)].permute(2, 0, 1)
    return out


def pack_dgrad(hat, taps, perm):
    O = hat.shape[0]
    h = hat.reshape(O, -1, taps)
    return h[_perm_index(perm, O)].flip(2).permute(2, 1, 0).contiguous()


def pack_fwd_frag(hat):
    """(O, I, taps) -> (taps, I / 32, O / 32, 2, 64, 8)"""
    O, I, T = hat.shape
    assert O % 32 == 0 and I % 32 == 0
    # co = 32 cb + l31; ci = 32 c + 16 ks + 8 g + e  ->  [t][c][cb][ks][32 g + l31][e]
    h = hat.reshape(O // 32, 32, I // 32, 2, 2, 8, T)
    return h.permute(6, 2, 0, 3, 4, 1, 5).reshape(T, I // 32, O // 32, 2, 64, 8).contiguous()


def pack_dgrad_frag(hat):
    """(O, I, taps) -> (taps, O / 32, I / 32, 2, 64, 8)"""
    return pack_fwd_frag(hat.flip(2).transpose(0, 1))


# ------------------------------------------------------------------------------------------------ bounds
def _e_d(n, rn, eps):
    """(relative error of d = eps + rn / sqrt(n), relative error of rn, d)"""
    sqn = math.sqrt(n)
    r = rn / sqn
    d = eps + r
    e_rn = ((n + 1) / 2 + 2) * U
    return (e_rn + 3 * U) * r / d + 2 * U, e_rn, d        # (rn * rsqrtf(n) and rn / sqrtf(n) both cost 3 u)


def normalize_bound(w64, eps=EPS):
    """|stored master - normalize_master(w)| elementwise"""
    w = _rows(w64.to(f64))
    e_d, _, _ = _e_d(w.shape[1], w.norm(dim=1, keepdim=True), eps)
    return (2 * (e_d + 2 * U) * _rows(normalize_master(w64, eps)).abs()).reshape(w64.shape)


def effective_bound(w64, eps=EPS):
    """|hat - effective(w)| elementwise, w the master the kernel read (or just stored)"""
    w = _rows(w64.to(f64))
    e_d, _, _ = _e_d(w.shape[1], w.norm(dim=1, keepdim=True), eps)
    return (2 * (e_d + 4 * U) * _rows(effective(w64, eps)).abs()).reshape(w64.shape)


def project_bound(a64, da, w64, out64=None, eps=EPS):
    """|kernel - project(a, w)| elementwise; da: elementwise bound on the error of the kernel's a; out64: the value after
    adding onto an old gradient (None: the kernel stores v itself)"""
    a, w, da = _rows(a64.to(f64)), _rows(w64.to(f64)), _rows(da.to(f64))
    n = w.shape[1]
    sqn = math.sqrt(n)
    rn = w.norm(dim=1, keepdim=True)
    e_d, e_rn, d = _e_d(n, rn, eps)
    c0 = 1.0 / (d * sqn)
    e_c0 = e_d + 4 * U
    live = rn > 0
    den = (d * rn * sqn).clamp_min(1e-300)
    dot = (a * w).sum(dim=1, keepdim=True)
    c1 = torch.where(live, dot / den, torch.zeros_like(dot))
    ddot = (n + 2) * U * (a * w).abs().sum(dim=1, keepdim=True) + (da * w.abs()).sum(dim=1, keepdim=True)
    dc1 = torch.where(live, ddot / den + c1.abs() * (e_d + e_rn + 5 * U), torch.zeros_like(dot))
    v = c0 * (a - w * c1)
    dv = c0 * (da + w.abs() * dc1 + U * (w * c1).abs() + U * (a - w * c1).abs()) + (e_c0 + U) * v.abs()
    if out64 is not None:
        dv = dv + U * _rows(out64.to(f64)).abs()
    return (2 * dv).reshape(w64.shape)


def finish_bound(slabs64, w64, I, taps, perm, scale, g0, accumulate):
    """|kernel - finish(...)| elementwise"""
    S, T, O, Ipad = slabs64.shape
    w = w64.to(f64).reshape(O, I, taps)
    a = slab_sum(slabs64, I, taps, perm, scale)
    da = (S + 1) * U * slab_sum(slabs64.abs(), I, taps, perm, abs(scale))
    out = g0.to(f64).reshape(w.shape) + project(a, w) if accumulate else None
    return project_bound(a, da, w, out)


Check = namedtuple("Check", "ok worst l2 finite")


def check(got, ref, bound, l2=L2_LIMIT):
    """|got - ref| <= bound elementwise (an exact zero error passes a zero bound) and rel L2 <= l2"""
    got, ref, bound = got.detach().cpu().to(f64), ref.to(f64), bound.to(f64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if not bool(torch.isfinite(got).all()):
        return Check(False, float("inf"), float("inf"), False)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = ratio.max().item() if ratio.numel() else 0.0
    r = ((got - ref).norm() / (ref.norm() + 1e-300)).item()
    return Check(worst <= 1.0 and r <= l2, worst, r, True)


# ------------------------------------------------------------------------------------------------ inputs
def gen(*key):
    """generator seeded by a fixed polynomial mix of the key (the same tensors on every interpreter and machine)"""
    seed = 7
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def master_rows(g, O, n, zero_row=None):
    """fp32 (O, n): rows with rms spread log-uniformly over 1e-4 .. 1e2 (eps = 1e-4 moves the result by between 50 % and
    1e-6), the extremes always present when O >= 3; row `zero_row` (default O // 2, none when O == 1) is all zero"""
    w = torch.randn(O, n, generator=g, dtype=f64)
    w = w / w.pow(2).mean(dim=1, keepdim=True).sqrt().clamp_min(1e-30)
    ex = torch.rand(O, generator=g, dtype=f64) * 6 - 4
    if O >= 3:
        ex[0], ex[O - 1] = -4.0, 2.0
    w = (w * (10.0 ** ex)[:, None]).float()
    if zero_row is None and O > 1:
        zero_row = O // 2
    if zero_row is not None:
        w[zero_row] = 0.0
    return w


def make_perm(g, O):
    """a row permutation that is not its own inverse (O >= 3), int32"""
    p = torch.randperm(O, generator=g)
    if O >= 3 and torch.equal(torch.argsort(p), p):
        p = p.roll(1)
        if torch.equal(torch.argsort(p), p):
            p = torch.arange(O).roll(1)
    return p.to(torch.int32)


BETA = 0.7


def slabs_for(g, S, taps, O, I, Ipad, w, perm, scale):
    """fp32 slabs (S, taps, O, Ipad) whose scaled sum is a = randn + BETA * w (a and w correlated: with independent a and w
    the projected component is only 1 / sqrt(n) of the gradient and a wrong c1 would hide); the padding columns are NaN"""
    wp = w.reshape(O, I, taps)[_perm_index(perm, O)].permute(2, 0, 1).double()        # (taps, O, I) packed
    part = torch.randn(S, taps, O, I, generator=g, dtype=f64) / math.sqrt(S) + BETA * wp / S
    slabs = torch.full((S, taps, O, Ipad), float("nan"))
    slabs[..., :I] = (part / scale).float()
    return slabs


# ------------------------------------------------------------------------------------------------ case tables
# a. modules of the multi-tensor prep plan: (name, kind, O, I, k, ipad, perm, frag, cat)
PrepMod = namedtuple("PrepMod", "name kind O I k ipad perm frag cat")


def _m(name, O, I, k, kind="conv", ipad=None, perm=False, frag=False, cat=False):
    return PrepMod(name, kind, O, I, k, ipad, perm, frag, cat)


PREP_MODULES = [
    _m("scalar_n27_padded", 64, 3, 3, ipad=32),          # scalar normalisation (n = 27), padded 8-wide forward pack
    _m("regs_ragged_n36", 64, 4, 3, ipad=32),            # register path with a ragged float4 (n = 36)
    _m("rb2_ragged_group", 3, 64, 3),                    # rb = 2, last group rbc = 1, scalar dgrad stores
    _m("groups_32_4", 36, 64, 1),                        # groups of 32 and 4: the non-8 dgrad path
    _m("perm_72", 72, 64, 1, perm=True),                 # hat stays in master order
    _m("ipad10_scalar_fwd", 16, 10, 1),                  # Ipad % 8 != 0: scalar forward stores
    _m("lin10", 256, 10, 1, kind="linear"),              # Linear(10, 256): scalar rows of 10, hat only
    _m("cat_lin64", 256, 64, 1, kind="linear", cat=True),   # Linear(64, 256) and Linear(64, 40) passed as `cat` (one
    _m("cat_lin64_b", 40, 64, 1, kind="linear", cat=True),  # in_features, as the plan requires): wcat rows back to back
    _m("regs_last_n5120", 8, 5120, 1),                   # last register-path size
    _m("long_first_n5124", 8, 5124, 1),                  # first long-row size
    _m("long_n5184", 5, 576, 3),                         # three trips, ragged last, rb = 8
    _m("long_n13824", 5, 1536, 3),                       # rb = 2
    _m("long_scalar_n4095", 6, 455, 3),                  # long scalar rows
    _m("frag_64x256", 64, 256, 3, frag=True),            # the production fragment case, rb = 16
    _m("frag_32x64", 32, 64, 3, frag=True),
    _m("frag_64x32", 64, 32, 3, frag=True),
]
# run again, one plan each, with the tile size set so that rb is 8, 4, 2 and 1
PREP_RB_MODULES = [m for m in PREP_MODULES if m.frag] + [_m("ragged_72x64", 72, 64, 3, frag=True),
                                                         _m("ragged_40x64", 40, 64, 3, frag=True)]
PREP_RBS = [8, 4, 2, 1]


def expected_rb(O, n, tile_bytes=96 * 1024):
    rb = 32
    while rb > 1 and (rb * n * 2 > tile_bytes or rb > O):
        rb //= 2
    return rb


@functools.lru_cache(maxsize=None)
def prep_master(name):
    """(w0 fp32 (O, I, taps), perm int32 or None) of a module of PREP_MODULES / PREP_RB_MODULES"""
    k, m = next((k, m) for k, m in enumerate(PREP_MODULES + PREP_RB_MODULES) if m.name == name)
    g = gen(11, k, m.O, m.I, m.k)
    taps = m.k * m.k
    w = master_rows(g, m.O, m.I * taps).reshape(m.O, m.I, taps)
    return w, (make_perm(g, m.O) if m.perm else None)


# b. ops.wgrad_finish: (S, taps, O, I, Ipad), each with perm on / off, accumulate on / off and scale in {1, 0.37}
FINISH_CASES = [
    (1, 1, 16, 64, 64),             # single slab
    (2, 1, 16, 64, 64),             # S <= 3 with G = 2
    (3, 9, 8, 32, 32),              # S <= 3 with G = 2, 3x3
    (3, 1, 8, 2048, 2048),          # S <= 3, the longest row that still gets G = 2: 1024 work items, one per thread
    (3, 1, 4, 4096, 4096),          # S <= 3 with G = 1: all four vectors of a thread's trip in use
    (4, 1, 16, 256, 256),           # eight-wide loop not entered
    (8, 1, 16, 64, 64),             # G = 8
    (20, 1, 16, 512, 512),          # G = 8 with a tail of 2 or 3 slabs per group (the unrolled trip is not entered)
    (20, 1, 8, 2048, 2048),         # unrolled trip plus tail with G = 2
    (37, 9, 8, 64, 64),             # odd slab count: G = 4, one unrolled trip and a tail of one or two slabs
    (5, 9, 16, 3, 8),               # scalar path
    (4, 1, 10, 10, 10),             # scalar path
    (6, 9, 16, 4, 32),              # vector path with padding
    (2, 9, 3, 1536, 1536),          # n = 13824, near the 64 KiB row limit (S <= 3, G = 1, the trip's last vectors idle)
]
FINISH_VARIANTS = [(perm, acc, scale) for perm in (False, True) for acc in (False, True) for scale in (1.0, 0.37)]


def finish_G(S, taps, I, Ipad, block=1024):
    """s-groups per vector of the per-tensor finish (block = 1024) and of the multi-tensor finish (512): the host loops of
    edm_wgrad_finish / edm_wgrad_finish_multi, kept here so that a case's comment can be asserted"""
    n = I * taps
    E = n // 4 if I % 4 == 0 and Ipad % 4 == 0 else n
    G = 1
    while G < 8 and 2 * G <= S and E * 2 * G <= block and (2 * G + 1) * n * 4 <= 96 * 1024:
        G *= 2
    return G


# c. ops.wgrad_finish_multi: (S, taps, O, I, Ipad, perm, accumulate, scale); the first eight are the shapes of
# test_wgrad3_gpu.test_wgrad_finish_multi_matches_the_per_tensor_finish
MULTI_CASES = [
    (8, 1, 256, 256, 256, False, False, 1.0), (16, 1, 768, 256, 256, True, True, 0.7), (4, 1, 256, 768, 768, False, True, 1.0),
    (2, 1, 64, 1280, 1280, False, False, 0.5), (3, 9, 32, 4, 32, False, True, 1.0), (1, 1, 10, 3, 8, False, False, 1.0),
    (5, 9, 64, 64, 64, True, False, 1.3), (8, 1, 256, 512, 512, False, True, 1.0),
    # a run of five O = 1 items (the row-to-item walk); the third is an all-zero row
    (3, 1, 1, 64, 64, False, False, 1.0), (2, 1, 1, 10, 12, False, True, 0.37), (4, 1, 1, 256, 256, False, False, 1.0),
    (1, 9, 1, 8, 8, False, True, 1.0), (5, 1, 1, 64, 64, False, False, 0.37),
    (4, 9, 32, 112, 112, True, True, 0.37),      # n = 1008: the prefetched 3x3 form
    (4, 9, 32, 128, 128, False, True, 1.0),      # n = 1152: the late-load form
]
MULTI_ZERO_O1 = 10                                # index of the O = 1 item whose only row is zero
# 41 items: the second launch of ops.wgrad_finish_multi is taken
MULTI_41 = [(1 + k % 5, 1, 1 + k % 3, 8 + 4 * (k % 4), 8 + 4 * (k % 4), k % 2 == 1, k % 3 == 0, (1.0, 0.37)[k % 2])
            for k in range(41)]

FinishCase = namedtuple("FinishCase", "slabs w g0 perm I taps scale accumulate ref bound")


@functools.lru_cache(maxsize=None)
def finish_case(S, taps, O, I, Ipad, perm, accumulate, scale, salt=0, zero_row=None):
    """operands of one finish (CPU, fp32) with the fp64 reference and its bound.  g0 is what the gradient buffer holds
    before the call: added onto with accumulate, overwritten without (the reference then starts from zero)."""
    g = gen(12, S, taps, O, I, Ipad, perm, accumulate, int(scale * 100), salt)
    w = master_rows(g, O, I * taps, zero_row=zero_row).reshape(O, I, taps)
    p = make_perm(g, O) if perm else None
    slabs = slabs_for(g, S, taps, O, I, Ipad, w, p, scale)
    g0 = torch.randn(O, I, taps, generator=g)
    base = g0 if accumulate else torch.zeros_like(g0)
    clean = slabs[..., :I]
    ref = finish(clean.double(), w.double(), I, taps, p, scale, base)
    bound = finish_bound(clean.double(), w.double(), I, taps, p, scale, base, accumulate)
    return FinishCase(slabs, w, g0, p, I, taps, scale, accumulate, ref, bound)


def multi_case(k, c, salt=1):
    zero = 0 if (salt == 1 and k == MULTI_ZERO_O1) else None
    return finish_case(*c, salt=salt * 1000 + k, zero_row=zero)


# d. k_wgrad3_finish with a real master: three groups of tests/conv_exact_ref.py and the late-load layer
# (n = 9 * 832 = 7488 > 7168)
W3_REAL_GROUPS = ["small", "ksplit", "single", "late"]
W3_LATE_LAYER = dict(B=2, H=8, W=8, Cin=832, Cout=64)


def w3_master(g, G):
    """master (Cout, I, 3, 3) for conv_exact_ref.w3_layer(master=...): rows along randn + BETA * G / rms(G) (G: the layer's
    raw integer gradient, so that the gradient and the master are correlated), rms spread as in master_rows, one zero row"""
    Cout = G.shape[0]
    Gr = _rows(G.to(f64))
    w = torch.randn(Gr.shape, generator=g, dtype=f64) + BETA * Gr / Gr.pow(2).mean(dim=1, keepdim=True).sqrt().clamp_min(1e-30)
    w = w / w.pow(2).mean(dim=1, keepdim=True).sqrt()
    ex = torch.rand(Cout, generator=g, dtype=f64) * 6 - 4
    ex[0], ex[Cout - 1] = -4.0, 2.0
    w = (w * (10.0 ** ex)[:, None]).float()
    w[Cout // 2] = 0.0
    return w.reshape(G.shape)


@functools.lru_cache(maxsize=None)
def w3_real_group(name):
    """(layer keywords, conv_exact_ref.W3Layer with the master of w3_master) of a group of W3_REAL_GROUPS.  The integer
    operands come from tests/conv_exact_ref.py, imported here and not at the top: this module stays free of the kernels'
    test files for everything else."""
    import conv_exact_ref as X
    import test_wgrad3_gpu as W3
    group = {"small": X.W3_GROUPS["small"], "ksplit": X.W3_GROUPS["ksplit"], "single": W3.GROUP_SMALL[1:2],
             "late": [W3_LATE_LAYER]}[name]
    g = gen(13, len(group), sum(kw["B"] * kw["Cin"] for kw in group))
    return group, [X.w3_layer(g, master=w3_master, **kw) for kw in group]


def w3_bound(L):
    """bound of one such layer: the raw gradient is exact, so a = scale * G carries the rounding of that multiply alone"""
    a = L.scale * L.G
    da = U * a.abs() if L.scale != 1.0 else torch.zeros_like(a)
    return project_bound(a, da, L.wm.double(), L.ref if L.accumulate else None)
