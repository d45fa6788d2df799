"""The attention kernels judged per BLOCK -- one (sample, head, 32-token tile) of y, one (sample, head, part in q/k/v, 32-token
tile) of gqkv -- and on structured operands with exactly known answers.  The whole-tensor limits of the existing attention
tests (rel L2 6e-3 / 1.5e-2 over every head, sample and token at once) leave 2-7x slack over the bf16 rounding floor; a fault
confined to one token tile of one head fits inside it (tests/test_attention_blocks_cpu.py shows two that do).  Ragged last
tiles, tile seams and head-to-workgroup maps are where these kernels carry their special code.

Reference, stand-in, metric, report and case lists: tests/attention_blocks_ref.py.

LIMIT RULE, random operands (bf16-representable, seeded per case).  Per case and direction
    limit = min(whole-tensor limit of the existing tests, 2 x worst block of stand_in against reference),
computed on the CPU from the reference side alone, never from a kernel's output; the stand-in rounds p = exp(s - max) to bf16
before the normalisation and rounds the outputs to bf16, as the kernels' docstrings say they do.  Every block is judged,
every output is finite, every worst block is recorded under attnblocks/ (parity_log).  The fp32 kernels keep the project's own
limits (5e-6 f32_attention, 2e-5 split_attention) per block against the fp64 result of the fp32 operands.

PATHS AND MEASURED WORST BLOCKS (MI355X: worst block over the cases, the range of the cases' limits, worst measured / limit)
  ops.attention_fwd / attention_bwd, head dim 64 -- attention.hip, NT = ceil(N / 32) tiles in registers:
    N = 1 (NT 1, one token), 32 (NT 1 full), 33 (NT 2, one token in the last tile), 65 / 100 / 128 (NT 4: one token in the
    last tile, masked, full), 225 / 256 (NT 8, 8 waves: one token in the last tile, full), 3 samples x 2 heads at N = 64
  head dims 32 / 128 / 144 / 192 -- attention_generic.hip, streamed operands: N = 49, 100, 128; 144 also at 256
      forward  2.98e-3 (1x15x15x1x64), limits 4.8e-3 .. 6.0e-3 and 0 at N = 1 (y = v, met exactly), 0.51 of the limit
      backward 2.78e-3 (1x10x10x1x192), limits 3.3e-3 (N = 1) .. 7.6e-3, 0.51 of the limit
  ops.attention_qkv_fwd / attention_qkv_bwd, C = 256, 4 heads -- attention_fused.hip: N = 49, 66 (NT 2, ring of 4), 196, 256
    (NT 8, ring of 7, ragged and full); forward with ATTN_HP = 0 / 1 / 2 / 4 heads per workgroup and EDM_ATTN_STAGE_FWD = 0 / 1,
    backward with EDM_ATTN_STAGE = 1 / 0; B = 3 and 9 (the grid is padded to 8 samples; the head-to-workgroup map changes
    with HP and B)
      forward  4.06e-3 (9x6x11, every hp and stage alike), limits 5.5e-3 .. 6.0e-3, 0.68 of the limit: the kernel rounds the
               qkv conv's fp32 sums where the reference rounds fp64 ones, and a q / k / v entry that lands on the other side
               of a bf16 tie moves one token's row
      backward 3.42e-3 (9x6x11), limits 5.7e-3 .. 8.9e-3, 0.52 of the limit
  ops.attention_long_fwd / attention_long_bwd -- attention_long.hip, key tiles of 64, query-major and key-major backward:
    SHAPES of tests/test_attention_long_gpu.py (289 .. 4096 tokens) and its 256-token case
      forward  3.18e-3 (1x17x17x2x192), limits 5.6e-3 .. 6.0e-3, 0.56 of the limit
      backward 3.01e-3 (1x17x17x1x144), limits 5.7e-3 .. 6.3e-3, 0.52 of the limit
  ops.f32_attention -- k_attn_f32_g, 64 queries per workgroup -- and ops.split_attention -- attention_split.hip: forward
    only, the shapes of test_f32_attention_vs_fp64 / test_split_attention_vs_fp64
      f32_attention 8.6e-7 (1x32x32x1x32; limit 5e-6), split_attention 6.9e-6 (3x16x16x4x64; limit 2e-5)
  (b) below: excited blocks 4.09e-3 attention.hip / generic, 3.22e-3 long, 2.90e-3 fused; limits 5.1e-3 .. 1.5e-2, at most
      0.68 of the limit

STRUCTURED OPERANDS
  (a) uniform softmax: every q, k, v entry +-1, all keys of a head equal -> normalised operands exactly +-1, p uniform,
      y = m / N with m = sum_j v_j.  A masked-tail key that leaks changes the divisor.  What "exactly" means follows from
      where a kernel rounds the probabilities (attention_blocks_ref.uniform_check):
      attention.hip      p = exp(s - max) = 1 into P.V, the fp32 sum N divides afterwards: torch.equal with m / N where N is
                         a power of two, |y - m/N| <= 2^-8 |m/N| + 2^-20 elsewhere (one bf16 rounding of an fp32 quotient).
      attention_generic  rounds p / sum = 1 / N to bf16 before P.V (the oracle's own placement), so the accumulator holds
                         m * bf16(1/N) exactly: torch.equal with bf16(m * bf16(1/N)) at EVERY N, which is m / N where N is
                         a power of two.  Two roundings: at N = 225, m = -7 it gives -2^-5, 4.5e-3 from m / N, which the
                         one-rounding bound does not allow a correct kernel.
      fused, long        no running maximum: p = exp(s - offset) goes into P.V rounded to bf16 and into the row sum
                         unrounded (attention_fused.hip 4., attention_long.hip "l = sum p in fp32, bf16(p) into the PV
                         MFMA"), so y = m/N * bf16(p)/p, which is m / N only where p is a bf16.  They run (a) twice: with
                         every query equal to its head's key -- s = sqrt(d), the offset, p = 1 -- under attention.hip's
                         assertions; and with random q under |y - m/N| <= (2^-7 + 2^-15) |m/N| + 2^-20, two factors within
                         2^-8 of 1 (bf16(p)/p and the output rounding), where a leaked zero key (p = exp(-sqrt(d)) against
                         real keys at exp(s - sqrt(d)), s ~ N(0, 1)) moves the divisor by tens of percent.
      fp32 kernels       the normalised operands are +-1 / (1 + 1e-4), not rounded, so y = m / N / (1 + 1e-4); per element
                         |y - that| <= limit x max(|m/N|, 1/sqrt(N)) with the kernel's own limit -- 1/sqrt(N) is the rms of
                         m / N, the floor an element with m = 0 needs (an fp32 sum of N terms +-c/N need not cancel to 0).
  (b) one excited query: gy (fused: gout behind a permutation matrix W_out) non-zero at one token i0 of one (sample, head),
      i0 = token 0 / the first token of the last tile / the last token.  dq is exactly zero at every other token and dq, dk,
      dv are exactly zero in every other (sample, head): dO = 0 gives delta = 0, dP = 0, dS = p * 0, and the norm backward of
      a zero gradient is zero.  The excited (sample, head)'s blocks meet the block limit of its own stand-in.
  (c) isolation: the y of one (sample, head) is bit-identical after every other sample's and head's operands are replaced
      (fused: the other heads' rows of W_qkv and the other samples' x)."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from parity_log import record

import attention_blocks_ref as A

DEV = "cuda"
bf16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def _ids(c):
    return "x".join(str(v) for v in c)


def nhwc(x, dtype=bf16):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV)


def _packed(qkv_ref_nchw, heads):
    return nhwc(A.packed_nchw(qkv_ref_nchw, heads))


def _judge(name, got, ref, limit):
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err, worst = A.block_errors(got, ref)
    w = err[worst].item()
    record("attnblocks/" + name, w, limit)
    print(f"{name}: worst block {w:.3e} at {worst}, limit {limit:.3e}")
    if not A.blocks_ok(err, limit):
        pytest.fail(A.report(name, err, limit), pytrace=False)


def _attn(ops, family, qkv, gy, heads):
    """-> y, gqkv (gqkv None where gy is None) of attention.hip / attention_generic.hip ("short") or attention_long.hip"""
    if family == "short":
        y = ops.attention_fwd(qkv, heads)
        return y, None if gy is None else ops.attention_bwd(qkv, y, gy, heads)
    y, stat = ops.attention_long_fwd(qkv, heads)
    return y, None if gy is None else ops.attention_long_bwd(qkv, y, gy, stat, heads)


def _wf(w, heads=A.FUSED_HEADS):
    """(3C, C) in the reference's row order -> the forward pack (1, 3C, C), rows [head][q|k|v][d]"""
    C = w.shape[1]
    return A.packed_nchw(w.view(1, 3 * C, C), heads).contiguous().to(bf16).to(DEV)


def _wd(wo):
    """(O, I) -> dgrad pack (1, I, O)"""
    return wo.t().contiguous().view(1, wo.shape[1], wo.shape[0]).to(bf16).to(DEV)


class _hp:
    def __init__(self, ops, hp):
        self.ops, self.hp = ops, hp

    def __enter__(self):
        self.old = self.ops.ATTN_HP
        self.ops.ATTN_HP = self.hp

    def __exit__(self, *a):
        self.ops.ATTN_HP = self.old


def _fused_supported(ops, N):
    if not ops._lib.call("edm_attention_qkv_supported", N, A.FUSED_C, A.FUSED_HEADS):
        pytest.skip("shape not covered by the fused kernel")


# ------------------------------------------------------------------------------------------- 3. random operands, per block
@pytest.mark.parametrize("shape", A.SHORT_CASES + A.GENERIC_CASES, ids=_ids)
def test_attention_blocks(ops, shape):
    B, H, W, heads, hd = shape
    c = A.case(*shape)
    y, gqkv = _attn(ops, "short", _packed(c["qkv"], heads), nhwc(c["gy"]), heads)
    _judge(f"attention_fwd[{_ids(shape)}]", A.unpack_y(y, heads), c["y"], c["lim_fwd"])
    _judge(f"attention_bwd[{_ids(shape)}]", A.unpack_gqkv(gqkv, heads), c["gqkv"], c["lim_bwd"])


@pytest.mark.parametrize("shape", A.LONG_CASES, ids=_ids)
def test_attention_long_blocks(ops, shape):
    B, H, W, heads, hd = shape
    c = A.case(*shape)
    y, gqkv = _attn(ops, "long", _packed(c["qkv"], heads), nhwc(c["gy"]), heads)
    _judge(f"attention_long_fwd[{_ids(shape)}]", A.unpack_y(y, heads), c["y"], c["lim_fwd"])
    _judge(f"attention_long_bwd[{_ids(shape)}]", A.unpack_gqkv(gqkv, heads), c["gqkv"], c["lim_bwd"])


@pytest.mark.parametrize("shape", A.FUSED_CASES, ids=_ids)
@pytest.mark.parametrize("hp", [0, 1, 2, 4])
@pytest.mark.parametrize("stage", ["0", "1"])
def test_attention_qkv_fwd_blocks(ops, shape, hp, stage, monkeypatch):
    monkeypatch.setenv("EDM_ATTN_STAGE_FWD", stage)
    B, H, W = shape
    _fused_supported(ops, H * W)
    c = A.fused_case(*shape)
    with _hp(ops, hp):
        y, stat = ops.attention_qkv_fwd(nhwc(c["x"]), _wf(c["w"]), A.FUSED_HEADS)
    assert torch.isfinite(stat).all()
    _judge(f"attention_qkv_fwd[{_ids(shape)} hp{hp} stage{stage}]", A.unpack_y(y, A.FUSED_HEADS), c["y"], c["lim_fwd"])


@pytest.mark.parametrize("shape", A.FUSED_CASES, ids=_ids)
@pytest.mark.parametrize("stage", ["1", "0"])
def test_attention_qkv_bwd_blocks(ops, shape, stage, monkeypatch):
    monkeypatch.setenv("EDM_ATTN_STAGE", stage)
    B, H, W = shape
    _fused_supported(ops, H * W)
    c = A.fused_case(*shape)
    x, wf = nhwc(c["x"]), _wf(c["w"])
    y, stat = ops.attention_qkv_fwd(x, wf, A.FUSED_HEADS)
    gqkv = ops.attention_qkv_bwd(x, y, nhwc(c["gout"]), stat, wf, _wd(c["wo"]), A.FUSED_HEADS, alpha=A.FUSED_ALPHA)
    _judge(f"attention_qkv_bwd[{_ids(shape)} stage{stage}]", A.unpack_gqkv(gqkv, A.FUSED_HEADS), c["gqkv"], c["lim_bwd"])


@pytest.mark.parametrize("shape", A.F32_CASES, ids=_ids)
def test_f32_attention_blocks(ops, shape):
    B, H, W, heads, hd = shape
    c = A.f32_case(*shape)
    y = ops.f32_attention(nhwc(c["qkv"], torch.float32), heads)
    _judge(f"f32_attention[{_ids(shape)}]", A.unpack_y(y, heads), c["y"], A.F32_LIMIT)


@pytest.mark.parametrize("shape", A.SPLIT_CASES, ids=_ids)
def test_split_attention_blocks(ops, shape):
    B, H, W, heads, hd = shape
    c = A.f32_case(*shape, scale=1.7, seed=B + H + heads)
    y = ops.split_attention(nhwc(c["qkv"], torch.float32), heads)
    _judge(f"split_attention[{_ids(shape)}]", A.unpack_y(y, heads), c["y"], A.SPLIT_LIMIT)


# --------------------------------------------------------------------------------------------- 4a. uniform softmax
def _uniform(ops, family, N, hd, q_is_k, B=2, heads=2):
    qkv, want = A.uniform_case(B, N, heads, hd, seed=N + hd, q_is_k=q_is_k)
    y, _ = _attn(ops, family, _packed(qkv.reshape(B, 3 * heads * hd, 1, N), heads), None, heads)
    y = A.unpack_y(y, heads)
    assert torch.isfinite(y).all()
    return y, want


def _fail_if(msg, what):
    if msg is not None:
        pytest.fail(f"{what}: {msg}", pytrace=False)


@pytest.mark.parametrize("N,hd", [(N, 64) for N in (32, 64, 128, 256, 33, 49, 65, 225)]
                         + [(N, hd) for hd in (32, 128, 144, 192) for N in (64, 49)] + [(256, 144), (225, 192)])
def test_uniform_softmax(ops, N, hd):
    """attention.hip (head dim 64: NT 1 / 2 / 4 / 8, full and with a ragged or one-token last tile) and
    attention_generic.hip: random q"""
    y, want = _uniform(ops, "short", N, hd, q_is_k=False)
    _fail_if(A.uniform_check(y, want, N, "unnormalised" if hd == 64 else "normalised"), f"attention_fwd N {N} d {hd}")


@pytest.mark.parametrize("N,hd", [(N, 64) for N in (32, 64, 128, 256, 1024, 33, 49, 65, 225, 289)]
                         + [(289, 144), (256, 192), (320, 32), (100, 128)])
@pytest.mark.parametrize("q_is_k", [True, False], ids=["q=k", "random-q"])
def test_uniform_softmax_long(ops, N, hd, q_is_k):
    """attention_long.hip (fixed offset sqrt(d)): q = k under the exact assertions, random q under the two-rounding bound"""
    y, want = _uniform(ops, "long", N, hd, q_is_k, B=1 if N >= 1024 else 2)
    _fail_if(A.uniform_check(y, want, N, "unnormalised" if q_is_k else "fixed-offset"), f"attention_long_fwd N {N} d {hd}")


@pytest.mark.parametrize("N", [64, 128, 256, 33, 49, 65, 225])
@pytest.mark.parametrize("hp", [0, 1, 2, 4])
@pytest.mark.parametrize("q_is_k", [True, False], ids=["q=k", "random-q"])
def test_uniform_softmax_fused(ops, N, hp, q_is_k):
    """attention_fused.hip (fixed offset 8) behind one-hot W_qkv rows, every heads-per-workgroup variant, 3 samples"""
    _fused_supported(ops, N)
    B = 3
    x, w, want = A.uniform_fused_case(B, N, seed=N, q_is_k=q_is_k)
    with _hp(ops, hp):
        y, stat = ops.attention_qkv_fwd(nhwc(x.view(B, A.FUSED_C, 1, N)), _wf(w), A.FUSED_HEADS)
    y = A.unpack_y(y, A.FUSED_HEADS)
    assert torch.isfinite(y).all() and torch.isfinite(stat).all()
    _fail_if(A.uniform_check(y, want, N, "unnormalised" if q_is_k else "fixed-offset"), f"attention_qkv_fwd N {N} hp {hp}")
    if q_is_k:      # p = 1 for every key: stat = 1 / N up to the fp32 reciprocal (two ulp allowed)
        assert (stat.double().cpu() * N - 1).abs().max().item() <= 2.0 ** -21


def _uniform_f32(y, want, N, limit):
    want = want / (1.0 + 1e-4)
    bad = (y - want).abs() > limit * torch.clamp(want.abs(), min=1.0 / math.sqrt(N))
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        return f"{int(bad.sum())} of {y.numel()} elements off m / N / (1 + 1e-4); first {i}: got {y[i].item()!r} expected {want[i].item()!r}"
    return None


@pytest.mark.parametrize("N,hd", [(32, 64), (49, 64), (256, 64), (289, 64), (1024, 64), (49, 144), (64, 32), (320, 192)])
def test_uniform_softmax_f32(ops, N, hd):
    B, heads = (1, 1) if N >= 1024 else (2, 2)
    qkv, want = A.uniform_case(B, N, heads, hd, seed=N + hd)
    y = A.unpack_y(ops.f32_attention(nhwc(qkv.reshape(B, 3 * heads * hd, 1, N), torch.float32), heads), heads)
    assert torch.isfinite(y).all()
    _fail_if(_uniform_f32(y, want, N, A.F32_LIMIT), f"f32_attention N {N} d {hd}")


@pytest.mark.parametrize("N", [49, 64, 225, 256])
def test_uniform_softmax_split(ops, N):
    B, heads, hd = 2, 2, 64
    qkv, want = A.uniform_case(B, N, heads, hd, seed=N + hd)
    y = A.unpack_y(ops.split_attention(nhwc(qkv.reshape(B, 3 * heads * hd, 1, N), torch.float32), heads), heads)
    assert torch.isfinite(y).all()
    _fail_if(_uniform_f32(y, want, N, A.SPLIT_LIMIT), f"split_attention N {N}")


# --------------------------------------------------------------------------------------------- 4b. one excited query
def _zero_elsewhere(name, g, b0, h0, i0):
    """g (B, heads, d, 3, N): dq exactly zero off token i0, everything exactly zero off (b0, h0); -0.0 is a zero"""
    assert torch.isfinite(g).all(), name
    nz = g.abs() != 0
    off = nz.clone()
    off[b0, h0] = False
    if off.any():
        idx = off.nonzero()
        pytest.fail(f"{name}: {idx.shape[0]} non-zero gradient elements outside (sample {b0}, head {h0}); samples "
                    f"{idx[:, 0].unique().tolist()} heads {idx[:, 1].unique().tolist()} parts {idx[:, 3].unique().tolist()} "
                    f"tokens {idx[:, 4].unique()[:12].tolist()}", pytrace=False)
    dq = nz[b0, h0, :, 0].any(0)
    dq[i0] = False
    if dq.any():
        pytest.fail(f"{name}: dq non-zero at tokens {dq.nonzero()[:, 0][:16].tolist()} (excited token {i0})", pytrace=False)
    assert nz[b0, h0, :, 0, i0].any() and nz[b0, h0, :, 1].any() and nz[b0, h0, :, 2].any(), f"{name}: the excited gradient is zero"


@functools.lru_cache(maxsize=None)
def _excited_case(N, hd, b0, h0, i0):
    B, heads = 2, 2
    qkv, gy = A.operands(B, 1, N, heads, hd, seed=N + hd + i0)
    g1 = torch.zeros_like(gy)
    g1.view(B, heads, hd, N)[b0, h0, :, i0] = gy.view(B, heads, hd, N)[b0, h0, :, i0]
    xb, gb = A.to_blocks_qkv(qkv, heads), A.to_blocks_y(g1, heads)
    _, g = A.reference(xb, gb, heads)
    _, gs = A.stand_in(xb, gb, heads)
    sl = (slice(b0, b0 + 1), slice(h0, h0 + 1))
    return qkv, g1, g, A.block_limit(gs[sl], g[sl], A.BWD_L2)


@pytest.mark.parametrize("family,N,hd", [("short", 100, 64), ("short", 225, 64), ("short", 33, 64), ("short", 100, 144),
                                         ("short", 49, 32), ("long", 289, 64), ("long", 324, 192), ("long", 100, 128)])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["first", "tile-start", "last"])
def test_one_excited_query(ops, family, N, hd, which):
    heads, b0, h0 = 2, 1, 0
    toks = A.excited_tokens(N)
    i0 = toks[min(which, len(toks) - 1)]
    qkv, gy, g_ref, limit = _excited_case(N, hd, b0, h0, i0)
    _, gqkv = _attn(ops, family, _packed(qkv, heads), nhwc(gy), heads)
    g = A.unpack_gqkv(gqkv, heads)
    name = f"excited/{family}[N{N} d{hd} i{i0}]"
    _zero_elsewhere(name, g, b0, h0, i0)
    _judge(name, g[b0:b0 + 1, h0:h0 + 1], g_ref[b0:b0 + 1, h0:h0 + 1], limit)


@functools.lru_cache(maxsize=None)
def _excited_fused_case(H, W, b0, h0, i0):
    B, C, heads, N = 2, A.FUSED_C, A.FUSED_HEADS, H * W
    d = C // heads
    x, w, _, gout = A.fused_operands(B, H, W, seed=N + i0)
    g = torch.Generator().manual_seed(N)
    pi = torch.randperm(C, generator=g)                # dO[c] = alpha * gout[pi[c]]
    wo = torch.zeros(C, C)
    wo[pi, torch.arange(C)] = 1.0
    g1 = torch.zeros_like(gout)
    rows = pi[h0 * d:(h0 + 1) * d]
    g1.view(B, C, N)[b0, rows, i0] = gout.view(B, C, N)[b0, rows, i0]
    _, gr = A.reference_fused(x, w, wo, g1, A.FUSED_ALPHA, heads)
    _, gs = A.stand_in_fused(x, w, wo, g1, A.FUSED_ALPHA, heads)
    sl = (slice(b0, b0 + 1), slice(h0, h0 + 1))
    return x, w, wo, g1, gr, A.block_limit(gs[sl], gr[sl], A.BWD_L2)


@pytest.mark.parametrize("H,W", [(14, 14), (6, 11)])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["first", "tile-start", "last"])
@pytest.mark.parametrize("stage", ["1", "0"])
def test_one_excited_query_fused(ops, H, W, which, stage, monkeypatch):
    monkeypatch.setenv("EDM_ATTN_STAGE", stage)
    _fused_supported(ops, H * W)
    heads, b0, h0 = A.FUSED_HEADS, 1, 2
    i0 = A.excited_tokens(H * W)[which]
    x, w, wo, gout, g_ref, limit = _excited_fused_case(H, W, b0, h0, i0)
    xd, wf = nhwc(x), _wf(w)
    y, stat = ops.attention_qkv_fwd(xd, wf, heads)
    gqkv = ops.attention_qkv_bwd(xd, y, nhwc(gout), stat, wf, _wd(wo), heads, alpha=A.FUSED_ALPHA)
    g = A.unpack_gqkv(gqkv, heads)
    name = f"excited/fused[{H}x{W} i{i0} stage{stage}]"
    _zero_elsewhere(name, g, b0, h0, i0)
    _judge(name, g[b0:b0 + 1, h0:h0 + 1], g_ref[b0:b0 + 1, h0:h0 + 1], limit)


# --------------------------------------------------------------------------------------------- 4c. isolation, forward
def _others_replaced(qkv, heads, b0, h0, seed, rounded=True):
    """(B, 3C, H, W) in the reference's channel order: new random values everywhere but in (sample b0, head h0)"""
    g = torch.Generator().manual_seed(seed)
    new = torch.randn(qkv.shape, generator=g)
    new = A.q(new) if rounded else new
    A.to_blocks_qkv(new, heads)[b0, h0] = A.to_blocks_qkv(qkv, heads)[b0, h0]
    return new


def _same_bits(name, y1, y2, heads, b0, h0):
    d = y1.shape[-1] // heads
    a, b = y1[b0, :, :, h0 * d:(h0 + 1) * d], y2[b0, :, :, h0 * d:(h0 + 1) * d]
    assert not torch.equal(y1, y2), f"{name}: the other heads' outputs did not change"
    if not torch.equal(a, b):
        bad = (a != b).view(-1, d)
        pytest.fail(f"{name}: y of (sample {b0}, head {h0}) changed with the other samples' / heads' operands at "
                    f"{int(bad.sum())} elements, tokens {bad.any(1).nonzero()[:, 0][:16].tolist()}", pytrace=False)


@pytest.mark.parametrize("family,H,W,hd", [("short", 10, 10, 64), ("short", 15, 15, 64), ("short", 7, 7, 144),
                                           ("short", 10, 10, 32), ("long", 17, 17, 64), ("long", 18, 18, 192)])
def test_forward_isolation(ops, family, H, W, hd):
    B, heads, b0, h0 = 3, 2, 1, 1
    qkv, _ = A.operands(B, H, W, heads, hd)
    y1, _ = _attn(ops, family, _packed(qkv, heads), None, heads)
    y2, _ = _attn(ops, family, _packed(_others_replaced(qkv, heads, b0, h0, 5), heads), None, heads)
    _same_bits(f"{family} {H}x{W} d{hd}", y1, y2, heads, b0, h0)


@pytest.mark.parametrize("kernel,H,W,hd", [("f32", 10, 10, 64), ("f32", 17, 17, 144), ("f32", 7, 7, 32), ("split", 10, 10, 64),
                                           ("split", 15, 15, 64)])
def test_forward_isolation_f32(ops, kernel, H, W, hd):
    B, heads, b0, h0 = 3, 2, 1, 1
    fn = ops.f32_attention if kernel == "f32" else ops.split_attention
    qkv = torch.randn(B, 3 * heads * hd, H, W, generator=torch.Generator().manual_seed(H + hd))
    y1 = fn(nhwc(qkv, torch.float32), heads)
    y2 = fn(nhwc(_others_replaced(qkv, heads, b0, h0, 5, rounded=False), torch.float32), heads)
    _same_bits(f"{kernel} {H}x{W} d{hd}", y1, y2, heads, b0, h0)


@pytest.mark.parametrize("H,W", [(14, 14), (6, 11), (16, 16)])
@pytest.mark.parametrize("hp", [0, 1, 2, 4])
def test_forward_isolation_fused(ops, H, W, hp):
    _fused_supported(ops, H * W)
    B, heads, C, b0, h0 = 3, A.FUSED_HEADS, A.FUSED_C, 1, 2
    x, w, _, _ = A.fused_operands(B, H, W)
    g = torch.Generator().manual_seed(9)
    x2 = A.q(torch.randn(x.shape, generator=g))
    x2[b0] = x[b0]
    w2 = A.q(torch.randn(w.shape, generator=g) / math.sqrt(C))
    w2.view(heads, -1, C)[h0] = w.view(heads, -1, C)[h0]            # reference rows head*3d + dd*3 + which: a head's 3d rows
    with _hp(ops, hp):
        y1, _ = ops.attention_qkv_fwd(nhwc(x), _wf(w), heads)
        y2, _ = ops.attention_qkv_fwd(nhwc(x2), _wf(w2), heads)
    _same_bits(f"fused {H}x{W} hp{hp}", y1, y2, heads, b0, h0)
