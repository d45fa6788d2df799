"""Block-wise error of the attention kernels: fp64 references, a second legitimate placement of the roundings that sizes the
limits, the block metric and its report, structured operands with exactly known answers, and the case lists shared by
tests/test_attention_blocks_cpu.py and tests/test_attention_blocks_gpu.py.  CPU only; nothing of the code under test is
imported (the oracle's rounding primitives and the channel permutation of tests/test_kernels_gpu.py are).

Layouts.  The reference views the qkv conv's output as (B, heads, d, 3, N), channel = head*3d + dd*3 + which
(networks.py:194); the kernels take NHWC with the packed channel order [head][q|k|v][d].  Everything here works in
  y     (B, heads, d, N)        gqkv  (B, heads, d, 3, N)
and `unpack_y` / `unpack_gqkv` / `packed_nchw` move between that and what the kernels read and write.

A BLOCK is one (sample, head, 32-token tile) of y, one (sample, head, part in q/k/v, 32-token tile) of gqkv; the last tile
holds N % 32 tokens.  `block_errors` returns the relative L2 of every block.  A block whose reference norm is below 1e-3 of
the rms norm of the blocks of its part (dq of every token but the excited one; dq and dk of a one-token map, which are
exactly zero) has no scale of its own and is judged absolutely, ||err|| / that rms norm.  Where a whole part is that small
against the tensor (the one-token map again: its rms norm is 0, and a kernel that forms dP and delta = <dO, y> in two
summation orders leaves dS = p (dP - delta) at 1e-7 of dO, not at 0) the rms norm over all blocks of the tensor takes its
place: q, k and v gradients of one attention share their scale.

Limit of a case and direction: min(whole-tensor limit of the existing tests, 2 x worst block of `stand_in` against
`reference`), computed from the reference side alone.  The factor 2: the smallest blocks are one token x one head's channels
(32..192 elements), so their rounding noise fluctuates, and the backward kernels also round the dS / P MFMA operands to bf16,
which the stand-in does not."""
import functools
import math

import torch

from oracle import edm_oracle as O
from test_kernels_gpu import _qkv_perm

TILE = 32
FWD_L2, FWD_MX = 6e-3, 3e-2          # the whole-tensor limits of test_attention_fwd_bwd and its siblings
BWD_L2, BWD_MX = 1.5e-2, 6e-2
F32_LIMIT, SPLIT_LIMIT = 5e-6, 2e-5  # test_f32_attention_vs_fp64, test_split_attention_vs_fp64

# ---------------------------------------------------------------------------------------------------------------- cases
# (B, H, W, heads, head_dim).  ops.attention_fwd / attention_bwd -- head dim 64 runs attention.hip, nt = ceil(N / 32) picks
# NT = 1 / 2 / 4 / 8: N = 1, 32 (NT 1, one token and full), 33 (NT 2, one token in the last tile), 65, 100, 128 (NT 4: one
# token in the last tile, masked, full), 225, 256 (NT 8: one token in the last tile, full); B = 3 x 2 heads (grid indexing)
SHORT_CASES = [(1, 1, 1, 1, 64), (1, 4, 8, 1, 64), (1, 3, 11, 1, 64), (1, 5, 13, 1, 64), (1, 10, 10, 2, 64),
               (2, 8, 16, 1, 64), (1, 15, 15, 1, 64), (1, 16, 16, 2, 64), (3, 8, 8, 2, 64)]
# the streamed head dims of attention_generic.hip at N = 49 (two tiles, ragged), 100 (NT 4 masked), 128 (NT 4 full); 144 at 256
GENERIC_CASES = [(B, H, W, heads, hd) for hd in (32, 128, 144, 192) for (B, H, W, heads) in
                 ((1, 7, 7, 2), (1, 10, 10, 1), (1, 8, 16, 1))] + [(1, 16, 16, 1, 144)]
# ops.attention_qkv_fwd / attention_qkv_bwd: C = 256, 4 heads; N = 49, 66 (NT 2), 196, 256 (NT 8, ragged and full)
FUSED_C, FUSED_HEADS, FUSED_ALPHA = 256, 4, 0.7071
FUSED_CASES = [(B, H, W) for (H, W) in ((7, 7), (6, 11), (14, 14), (16, 16)) for B in (3, 9)]
# ops.attention_long_fwd / attention_long_bwd: SHAPES of tests/test_attention_long_gpu.py (see there for what each reaches)
# and its 256-token case
LONG_CASES = [(1, 17, 17, 1, 64), (2, 18, 18, 2, 64), (1, 24, 24, 1, 32), (1, 17, 17, 1, 144), (1, 20, 20, 1, 128),
              (1, 17, 17, 2, 192), (2, 32, 32, 1, 64), (1, 64, 64, 1, 64), (3, 16, 16, 2, 64)]
# ops.f32_attention: the shapes of test_f32_attention_vs_fp64, one sample at 1024 tokens; ops.split_attention: those of
# test_split_attention_vs_fp64
F32_CASES = [(2, 8, 8, 4, 64), (2, 16, 16, 4, 64), (3, 7, 7, 2, 32), (1, 4, 4, 2, 128), (1, 16, 16, 4, 144), (2, 8, 8, 4, 192),
             (1, 9, 9, 2, 144), (1, 20, 20, 2, 64), (1, 32, 32, 1, 32)]
SPLIT_CASES = [(2, 8, 8, 4, 64), (3, 16, 16, 4, 64), (2, 7, 7, 2, 64), (1, 14, 14, 4, 64), (2, 11, 11, 1, 64)]


def q(x):
    return x.to(torch.bfloat16).to(x.dtype)


# -------------------------------------------------------------------------------------------------------------- layouts
def to_blocks_qkv(ref_nchw, heads):
    """(B, 3C, H, W) in the reference's channel order -> (B, heads, d, 3, N)"""
    B, C3 = ref_nchw.shape[:2]
    return ref_nchw.reshape(B, heads, C3 // (3 * heads), 3, -1)


def to_blocks_y(y_nchw, heads):
    """(B, C, H, W), channel = head*d + dd -> (B, heads, d, N)"""
    B, C = y_nchw.shape[:2]
    return y_nchw.reshape(B, heads, C // heads, -1)


def packed_nchw(ref_nchw, heads):
    """reference channel order -> the kernels' packed order [head][q|k|v][d] (still NCHW)"""
    return ref_nchw[:, _qkv_perm(ref_nchw.shape[1] // 3, heads)]


def unpack_y(y_nhwc, heads):
    """a kernel's y (B, H, W, C) -> (B, heads, d, N) fp64 on the CPU"""
    return to_blocks_y(y_nhwc.detach().double().cpu().permute(0, 3, 1, 2), heads)


def unpack_gqkv(g_nhwc, heads):
    """a kernel's gqkv (B, H, W, 3C) in packed channel order -> (B, heads, d, 3, N) fp64 on the CPU"""
    g = g_nhwc.detach().double().cpu().permute(0, 3, 1, 2)
    inv = torch.argsort(_qkv_perm(g.shape[1] // 3, heads))
    return to_blocks_qkv(g[:, inv], heads)


# ----------------------------------------------------------------------------------------------------------- references
def _attend(qkv, gy, heads, stand_in):
    x = qkv.detach().double().clone().requires_grad_(True)
    d = x.shape[2]
    t = O.q_bf16(O.rms_div(x, [2]))
    qq, kk, vv = t.unbind(3)
    s = torch.einsum("bhdi,bhdj->bhij", qq, kk) / math.sqrt(d)
    if stand_in:
        e = torch.exp(s - s.amax(dim=-1, keepdim=True))
        y = torch.einsum("bhij,bhdj->bhdi", O.q_bf16(e), vv) / e.sum(-1)[:, :, None, :]
    else:
        y = torch.einsum("bhij,bhdj->bhdi", O.q_bf16(torch.softmax(s, dim=-1)), vv)
    y.backward(gy.double())
    y, g = y.detach(), x.grad
    return (q(y), q(g)) if stand_in else (y, g)


def reference(qkv, gy, heads):
    """qkv (B, heads, d, 3, N), gy (B, heads, d, N), bf16-representable -> y (B, heads, d, N), gqkv (B, heads, d, 3, N):
    the algorithm of networks.py:194-202 in fp64 with the oracle's rounding points -- pixel norm rounded, softmax
    probabilities rounded -- and autograd through them (what test_attention_fwd_bwd builds inline)"""
    return _attend(qkv, gy, heads, False)


def stand_in(qkv, gy, heads):
    """a correct kernel's placement of the roundings: p = bf16(exp(s - max)) into the P.V product, normalised afterwards by
    the fp32 sum of the unrounded exponentials (the kernels' docstrings), y and gqkv rounded to bf16.  Sizes the limits only."""
    return _attend(qkv, gy, heads, True)


def _fused(x, w_qkv, w_out, gout, alpha, heads, fn):
    B, C, H, W = x.shape
    qkv = O.q_bf16(torch.einsum("oc,bchw->bohw", w_qkv.double(), x.double()))
    gy = O.q_bf16(alpha * torch.einsum("oc,bohw->bchw", w_out.double(), gout.double()))
    return fn(to_blocks_qkv(qkv, heads), to_blocks_y(gy, heads), heads)


def reference_fused(x, w_qkv, w_out, gout, alpha, heads):
    """x, gout (B, C, H, W); w_qkv (3C, C) effective weight in the reference's row order, w_out (C, C): `reference` behind the
    qkv conv (its output rounded to bf16) with dO = bf16(alpha * W_out^T gout) -> y, gqkv = d loss / d qkv_conv(x)
    (test_attnfused_gpu.py::_reference, test_attention_qkv_bwd)"""
    return _fused(x, w_qkv, w_out, gout, alpha, heads, reference)


def stand_in_fused(x, w_qkv, w_out, gout, alpha, heads):
    return _fused(x, w_qkv, w_out, gout, alpha, heads, stand_in)


def reference_f32(qkv, heads):
    """qkv (B, heads, d, 3, N) fp32 -> y in fp64: the reference's arithmetic without any rounding (the fp32 kernels)"""
    t = qkv.double()
    d = t.shape[2]
    t = t / (1e-4 + t.norm(dim=2, keepdim=True) / math.sqrt(d))
    qq, kk, vv = t.unbind(3)
    p = torch.softmax(torch.einsum("bhdi,bhdj->bhij", qq, kk) / math.sqrt(d), dim=-1)
    return torch.einsum("bhij,bhdj->bhdi", p, vv)


# --------------------------------------------------------------------------------------------------------- block metric
def _block_norms(x, tile):
    """x (B, heads, d, [3,] N) -> norms (B, heads, [3,] ceil(N / tile))"""
    N = x.shape[-1]
    nt = (N + tile - 1) // tile
    sq = (x.double() ** 2).sum(2)                                   # (B, heads, [3,] N)
    pad = sq.new_zeros(*sq.shape[:-1], nt * tile)
    pad[..., :N] = sq
    return pad.view(*sq.shape[:-1], nt, tile).sum(-1).sqrt()


def block_errors(got, ref, tile=TILE):
    """-> (errors, worst): errors (B, heads, ntiles) for y (B, heads, d, N), (B, heads, 3, ntiles) for gqkv (B, heads, d, 3, N),
    the relative L2 of each block (absolute against the part's rms block norm where the block has no scale, see the module
    docstring); worst = the index tuple of the largest"""
    assert got.shape == ref.shape and got.dim() in (4, 5)
    en, rn = _block_norms(got.double() - ref.double(), tile), _block_norms(ref, tile)
    parts = rn.dim() == 4
    dims = (0, 1, 3) if parts else (0, 1, 2)
    rms = (rn ** 2).mean(dim=dims, keepdim=True).sqrt()             # per part
    rms_all = (rn ** 2).mean().sqrt()
    rms = torch.where(rms < 1e-3 * rms_all, rms_all.expand_as(rms), rms).expand_as(rn)
    small = rn < 1e-3 * rms
    den = torch.where(small, rms, rn)
    err = torch.where(en == 0, torch.zeros_like(en), en / den)      # (0 / 0: an all-zero tensor reproduced exactly)
    worst = tuple(int(i) for i in (err == err.max()).nonzero()[0])
    return err, worst


def worst_block(got, ref, tile=TILE):
    err, worst = block_errors(got, ref, tile)
    return err[worst].item()


def block_limit(stand, ref, whole):
    """min(the whole-tensor limit, 2 x the stand-in's worst block)"""
    return min(whole, 2.0 * worst_block(stand, ref))


def report(what, err, limit, tile=TILE):
    """how many blocks exceed the limit, their extent along sample / head / part / tile, the first few with their figures (the
    pattern of the failing blocks is the diagnosis; after test_conv_exact_gpu._report)"""
    names = ("sample", "head", "part", "tile") if err.dim() == 4 else ("sample", "head", "tile")
    bad = ~(err <= limit)
    idx = bad.nonzero()
    lines = [f"{what}: {idx.shape[0]} of {err.numel()} blocks over the limit {limit:.3e} (worst {err.max().item():.3e}, "
             f"median {err.median().item():.3e})"]
    for a, nm in enumerate(names):
        u = idx[:, a].unique()
        lines.append(f"  {nm}: {u.numel()} distinct of {err.shape[a]}, {u[:12].tolist()}{' ...' if u.numel() > 12 else ''}")
    order = sorted(idx.tolist(), key=lambda i: -float(err[tuple(i)]))
    for i in order[:8]:
        i = tuple(i)
        d = dict(zip(names, i))
        if "part" in d:
            d["part"] = "qkv"[d["part"]]
        lines.append(f"  {d} tokens {i[-1] * tile}..: {err[i].item():.3e}")
    return "\n".join(lines)


def blocks_ok(err, limit):
    return bool(torch.isfinite(err).all()) and bool((err <= limit).all())


def whole_tensor_ok(got, ref, l2, mx):
    """the two assertions of test_kernels_gpu.close_bf16"""
    got, ref = got.double(), ref.double()
    rel = ((got - ref).norm() / (ref.norm() + 1e-30)).item()
    mxe = (got - ref).abs().max().item() / ref.abs().max().item()
    return rel <= l2 and (got - ref).abs().max().item() <= mx * ref.abs().max().item() + 1e-6, rel, mxe


# ------------------------------------------------------------------------------------------------------------- operands
def operands(B, H, W, heads, hd, seed=None):
    """test_attention_fwd_bwd's operands (its seed by default): qkv (B, 3C, H, W) in the reference's channel order and
    gy (B, C, H, W), fp32, bf16-representable"""
    g = torch.Generator().manual_seed(B + H + heads + hd if seed is None else seed)
    C = hd * heads
    qkv = q(torch.randn(B, 3 * C, H, W, generator=g))
    return qkv, q(torch.randn(B, C, H, W, generator=g))


@functools.lru_cache(maxsize=None)
def case(B, H, W, heads, hd):
    """a random case, computed once and left unchanged: operands (NCHW, reference channel order), the reference, the
    stand-in's worst blocks and the two limits"""
    qkv, gy = operands(B, H, W, heads, hd)
    xb, gb = to_blocks_qkv(qkv, heads), to_blocks_y(gy, heads)
    y, g = reference(xb, gb, heads)
    ys, gs = stand_in(xb, gb, heads)
    return dict(qkv=qkv, gy=gy, y=y, gqkv=g, stand_fwd=worst_block(ys, y), stand_bwd=worst_block(gs, g),
                lim_fwd=block_limit(ys, y, FWD_L2), lim_bwd=block_limit(gs, g, BWD_L2))


def fused_operands(B, H, W, seed=None):
    g = torch.Generator().manual_seed(B * 100 + H + W + 1 if seed is None else seed)
    C = FUSED_C
    x = q(torch.randn(B, C, H, W, generator=g))
    w = q(torch.randn(3 * C, C, generator=g) / math.sqrt(C))          # effective weights, the reference's row order
    wo = q(torch.randn(C, C, generator=g) / math.sqrt(C))
    gout = q(torch.randn(B, C, H, W, generator=g))
    return x, w, wo, gout


@functools.lru_cache(maxsize=None)
def fused_case(B, H, W):
    x, w, wo, gout = fused_operands(B, H, W)
    y, g = reference_fused(x, w, wo, gout, FUSED_ALPHA, FUSED_HEADS)
    ys, gs = stand_in_fused(x, w, wo, gout, FUSED_ALPHA, FUSED_HEADS)
    return dict(x=x, w=w, wo=wo, gout=gout, y=y, gqkv=g, stand_fwd=worst_block(ys, y), stand_bwd=worst_block(gs, g),
                lim_fwd=block_limit(ys, y, FWD_L2), lim_bwd=block_limit(gs, g, BWD_L2))


@functools.lru_cache(maxsize=None)
def f32_case(B, H, W, heads, hd, scale=1.0, seed=None):
    """fp32 operands as test_f32_attention_vs_fp64 (scale 1) / test_split_attention_vs_fp64 (scale 1.7) draw them"""
    g = torch.Generator().manual_seed(B + H + hd if seed is None else seed)
    qkv = torch.randn(B, 3 * heads * hd, H, W, generator=g) * scale
    return dict(qkv=qkv, y=reference_f32(to_blocks_qkv(qkv, heads), heads))


# -------------------------------------------------------------------------------------------------- structured operands
def signs(*shape, generator):
    return torch.randint(0, 2, shape, generator=generator).float() * 2 - 1


def uniform_case(B, N, heads, hd, seed, q_is_k=False):
    """(a) every q, k, v entry +-1 and all keys of a head equal: the normalised operands are exactly +-1 in bf16
    (1 / (1 + 1e-4) rounds to 1), every logit of a row is equal, p is uniform and y[:, i] = m / N, m = sum_j v_j.
    q_is_k: every query equals its head's key, so the common logit is sqrt(d), the fixed offset of the kernels that have no
    running maximum.  -> qkv (B, heads, d, 3, N) fp32, m / N (B, heads, d, N) fp64"""
    g = torch.Generator().manual_seed(seed)
    k = signs(B, heads, hd, 1, generator=g).expand(B, heads, hd, N)
    qq = k if q_is_k else signs(B, heads, hd, N, generator=g)
    v = signs(B, heads, hd, N, generator=g)
    qkv = torch.stack((qq, k, v), dim=3).contiguous()
    return qkv, (v.double().sum(-1, keepdim=True) / N).expand(B, heads, hd, N).contiguous()


def uniform_fused_case(B, N, seed, q_is_k=False):
    """(a) behind the qkv conv: x entries +-1, channels 0..127 constant over the tokens, 128..255 random per token; the rows
    of W_qkv are one-hot with value 1, the k rows select from [0, 128), the v rows (and the q rows, unless q_is_k makes each
    q row its k row) from [128, 256).  -> x (B, C, N), w (3C, C) in the reference's row order, m / N (B, heads, d, N)"""
    g = torch.Generator().manual_seed(seed)
    C, heads = FUSED_C, FUSED_HEADS
    d = C // heads
    x = torch.cat((signs(B, C // 2, 1, generator=g).expand(B, C // 2, N), signs(B, C // 2, N, generator=g)), dim=1).contiguous()
    sel = torch.empty(heads, d, 3, dtype=torch.long)
    sel[:, :, 1] = torch.randint(0, C // 2, (heads, d), generator=g)
    sel[:, :, 0] = sel[:, :, 1] if q_is_k else torch.randint(C // 2, C, (heads, d), generator=g)
    sel[:, :, 2] = torch.randint(C // 2, C, (heads, d), generator=g)
    w = torch.zeros(3 * C, C)
    w[torch.arange(3 * C), sel.reshape(-1)] = 1.0
    v = x[:, sel[:, :, 2].reshape(-1)].view(B, heads, d, N)
    return x, w, (v.double().sum(-1, keepdim=True) / N).expand(B, heads, d, N).contiguous()


def uniform_check(y, want, N, placement="unnormalised"):
    """-> None or a message.  placement = where the kernel rounds the (uniform) probabilities to bf16:
    "unnormalised"  p = exp(s - max) = 1 into P.V, the row sum N divides afterwards (attention.hip): y == m / N where N is a
                    power of two, else |y - m/N| <= 2^-8 |m/N| + 2^-20, one bf16 rounding of an fp32 quotient;
    "normalised"    bf16(p / sum) = bf16(1 / N) into P.V (attention_generic.hip, the oracle's own placement): the fp32
                    accumulator holds m * bf16(1 / N) exactly (16 significant bits), so y == bf16(m * bf16(1 / N)) at every
                    N -- which is m / N where N is a power of two;
    "fixed-offset"  kernels without a running maximum at a logit off the offset: p = exp(s - offset) enters P.V rounded to
                    bf16 and the row sum unrounded, so y = bf16(m/N * bf16(p)/p * (1 + fp32 noise)): two factors within 2^-8
                    of 1 (the unit roundoff of bf16), |y - m/N| <= (2^-7 + 2^-15) |m/N| + 2^-20 at every N"""
    y, want = y.double(), want.double()
    if placement == "fixed-offset":
        bad = (y - want).abs() > (2.0 ** -7 + 2.0 ** -15) * want.abs() + 2.0 ** -20
    elif placement == "normalised":
        pb = torch.tensor(1.0 / N, dtype=torch.float32).to(torch.bfloat16).double()
        bad = y != ((want * N).round() * pb).float().to(torch.bfloat16).double()
    elif N & (N - 1) == 0:
        bad = y != want
    else:
        bad = (y - want).abs() > 2.0 ** -8 * want.abs() + 2.0 ** -20
    if not bad.any():
        return None
    idx = bad.nonzero()
    lines = [f"{idx.shape[0]} of {y.numel()} elements off m / N"]
    for a, nm in enumerate(("sample", "head", "dim", "token")):
        u = idx[:, a].unique()
        lines.append(f"  {nm}: {u.numel()} distinct of {y.shape[a]}, {u[:12].tolist()}{' ...' if u.numel() > 12 else ''}")
    for i in idx[:6].tolist():
        i = tuple(i)
        lines.append(f"  {i}: got {y[i].item()!r} expected {want[i].item()!r}")
    return "\n".join(lines)


def excited_tokens(N):
    """(b) token 0, the last token, the first token of the last 32-token tile"""
    return sorted({0, N - 1, TILE * ((N - 1) // TILE)})
