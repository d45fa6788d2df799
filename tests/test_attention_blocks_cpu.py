"""The reference side of tests/test_attention_blocks_gpu.py, without a GPU (tests/attention_blocks_ref.py):

 * for every case of the GPU file the stand-in -- a second legitimate placement of the roundings -- stays under the case's
   block limit against the reference, i.e. the reference alone is quiet at block granularity;
 * two local faults (one token of dK 12 % short, one tile of dV 5 % too large) pass the whole-tensor assertions of
   test_attention_fwd_bwd and are caught block-wise;
 * the structured operands have the exactly predictable references the GPU file relies on."""
import math

import pytest
import torch

from oracle import edm_oracle as O

import attention_blocks_ref as A


def _ids(c):
    return "x".join(str(v) for v in c)


def _check_stand_in(c, heads):
    for d, whole in (("fwd", A.FWD_L2), ("bwd", A.BWD_L2)):
        stand, lim = c["stand_" + d], c["lim_" + d]
        print(f"{d}: stand-in worst block {stand:.3e}, limit {lim:.3e}")
        assert math.isfinite(stand) and stand <= lim <= whole, (d, stand, lim)
    assert torch.isfinite(c["y"]).all() and torch.isfinite(c["gqkv"]).all()


@pytest.mark.parametrize("shape", A.SHORT_CASES + A.GENERIC_CASES + [s for s in A.LONG_CASES if s not in A.SHORT_CASES],
                         ids=_ids)
def test_stand_in_is_under_the_block_limit(shape):
    _check_stand_in(A.case(*shape), shape[3])


@pytest.mark.parametrize("shape", A.FUSED_CASES, ids=_ids)
def test_stand_in_is_under_the_block_limit_fused(shape):
    _check_stand_in(A.fused_case(*shape), A.FUSED_HEADS)


def test_block_limits_sit_near_the_rounding_floor():
    """the stand-in's worst block over the short cases is a few 1e-3, the scale of one bf16 rounding, so the block limits
    are far below the whole-tensor one in the backward direction"""
    worst_f = max(A.case(*s)["stand_fwd"] for s in A.SHORT_CASES + A.GENERIC_CASES)
    worst_b = max(A.case(*s)["stand_bwd"] for s in A.SHORT_CASES + A.GENERIC_CASES)
    print(f"worst stand-in block: fwd {worst_f:.3e} bwd {worst_b:.3e}")
    assert worst_f <= 5e-3 and worst_b <= 5e-3


@pytest.mark.parametrize("shape,part,sample,head,tokens,factor", [
    ((1, 15, 15, 1, 64), 1, 0, 0, (224, 225), 0.88),       # dK of the single token of the last 32-token tile, 12 % short
    ((2, 16, 16, 4, 64), 2, 0, 0, (64, 96), 1.05),         # dV of one tile of one head, 5 % too large
], ids=["dk-last-token-12pct", "dv-one-tile-5pct"])
def test_local_faults_pass_the_whole_tensor_assertions_and_fail_block_wise(shape, part, sample, head, tokens, factor):
    c = A.case(*shape)
    got = A.q(c["gqkv"]).clone()
    err0, _ = A.block_errors(got, c["gqkv"])
    assert A.blocks_ok(err0, c["lim_bwd"]), A.report("undamaged", err0, c["lim_bwd"])
    got[sample, head, :, part, tokens[0]:tokens[1]] *= factor
    ok, rel, mxe = A.whole_tensor_ok(got, c["gqkv"], A.BWD_L2, A.BWD_MX)
    err, worst = A.block_errors(got, c["gqkv"])
    print(f"whole-tensor rel L2 {rel:.3e}, max err / max ref {mxe:.3e}, worst block {err[worst].item():.3e} at {worst}, "
          f"limit {c['lim_bwd']:.3e}")
    assert ok, (rel, mxe)                                  # the existing assertions do not see it
    assert not A.blocks_ok(err, c["lim_bwd"])
    assert worst == (sample, head, part, tokens[0] // A.TILE)
    assert int((err > c["lim_bwd"]).sum()) == 1
    text = A.report("gqkv", err, c["lim_bwd"])
    assert "1 of" in text and f"'part': '{'qkv'[part]}'" in text


def test_block_errors_layout_and_the_blocks_without_a_scale():
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(2, 3, 8, 3, 70, generator=g, dtype=torch.float64)
    ref[1, 2, :, 0, 32:64] = 0                             # a block without a scale of its own
    got = ref.clone()
    got[0, 1, :, 2, 64:] *= 1.5                            # the 6-token last tile
    got[1, 2, :, 0, 40] = 1e-3
    err, worst = A.block_errors(got, ref)
    assert err.shape == (2, 3, 3, 3) and worst == (0, 1, 2, 2)
    assert abs(err[worst].item() - 0.5) < 1e-12
    rms = (A._block_norms(ref, 32)[:, :, 0] ** 2).mean().sqrt().item()
    assert abs(err[1, 2, 0, 1].item() - 1e-3 * math.sqrt(8) / rms) < 1e-12
    assert int((err > 0).sum()) == 2
    ey, wy = A.block_errors(got[:, :, :, 2], ref[:, :, :, 2])
    assert ey.shape == (2, 3, 3) and wy == (0, 1, 2)
    # a part that is zero throughout is judged against the tensor's scale, an all-zero tensor only by equality
    ref[:, :, :, 0] = 0
    got = ref.clone()
    got[0, 0, :, 0, 0] = 1e-9
    assert 0 < A.block_errors(got, ref)[0].max().item() < 1e-9
    z = torch.zeros(1, 1, 4, 3, 5, dtype=torch.float64)
    assert A.block_errors(z, z)[0].max().item() == 0
    assert math.isinf(A.block_errors(z + 1e-30, z)[0].max().item())


def test_unpacking_inverts_the_packed_channel_order():
    B, H, W, heads, hd = 2, 3, 5, 2, 32
    qkv, gy = A.operands(B, H, W, heads, hd)
    packed = A.packed_nchw(qkv, heads).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(A.unpack_gqkv(packed, heads), A.to_blocks_qkv(qkv, heads).double())
    # packed order is [head][q|k|v][d]
    t = A.to_blocks_qkv(qkv, heads)
    assert torch.equal(packed[1, 2, 4].view(heads, 3, hd)[1, 2], t[1, 1, :, 2, 2 * W + 4])
    assert torch.equal(A.unpack_y(gy.permute(0, 2, 3, 1), heads), A.to_blocks_y(gy, heads).double())


@pytest.mark.parametrize("hd", [32, 64, 128, 144, 192])
@pytest.mark.parametrize("N", [32, 49, 64, 225, 256])
def test_uniform_softmax_reference_is_m_over_n(hd, N):
    """(a): normalised operands exactly +-1, p uniform, y = m * bf16(1 / N) (= m / N where N is a power of two)"""
    for q_is_k in (False, True):
        qkv, want = A.uniform_case(2, N, 2, hd, seed=hd + N, q_is_k=q_is_k)
        t = O.q_bf16(O.rms_div(qkv.double(), [2]))
        assert torch.equal(t, qkv.double())
        qq, kk, vv = t.unbind(3)
        s = torch.einsum("bhdi,bhdj->bhij", qq, kk) / math.sqrt(hd)
        assert (s.amax(-1) == s.amin(-1)).all()
        if q_is_k:
            assert (s == math.sqrt(hd)).all() or hd not in (64, 144)
            assert (s - math.sqrt(hd)).abs().max().item() < 1e-12
        p = torch.softmax(s, dim=-1)
        assert (p.amax(-1) == p.amin(-1)).all() and (p - 1.0 / N).abs().max().item() < 1e-17
        y, _ = A.reference(qkv, torch.zeros_like(want), 2)
        pb = float(torch.tensor(1.0 / N, dtype=torch.float64).to(torch.bfloat16))
        assert (y - want * N * pb).abs().max().item() <= 1e-12
        assert A.uniform_check(A.q(want.float()) if N & (N - 1) == 0 else want, want, N) is None
        assert A.uniform_check(A.q(y.float()), want, N, "normalised") is None       # the oracle's placement, rounded once more
        assert A.uniform_check(want * (1 + 2.0 ** -6), want, N, "fixed-offset") is not None
        assert torch.equal((want * N).round() / N, want) and (want.abs() <= 1).all()
        if N & (N - 1) == 0:
            assert torch.equal(y, want) and torch.equal(A.q(want), want)      # m / N is a bf16 where N <= 256 is 2^k


def test_uniform_softmax_behind_the_qkv_conv():
    for q_is_k in (False, True):
        x, w, want = A.uniform_fused_case(2, 49, seed=3, q_is_k=q_is_k)
        qkv = torch.einsum("oc,bcn->bon", w.double(), x.double())
        assert (qkv.abs() == 1).all()
        t = A.to_blocks_qkv(qkv, A.FUSED_HEADS)
        assert (t[:, :, :, 1] == t[:, :, :, 1, :1]).all()              # all keys of a head are equal
        assert bool((t[:, :, :, 0] == t[:, :, :, 1]).all()) == q_is_k
        assert torch.equal(t[:, :, :, 2].sum(-1) / 49, want[..., 0])
        assert (w.sum(1) == 1).all() and (w.abs().sum(1) == 1).all()


@pytest.mark.parametrize("hd,N", [(64, 100), (144, 100), (64, 289), (32, 49)])
def test_one_excited_query_reference_is_zero_elsewhere(hd, N):
    """(b): gy non-zero at one token of one (sample, head): dq is exactly zero at every other token, and dq, dk, dv are exactly
    zero in every other (sample, head)"""
    B, heads, b0, h0 = 2, 2, 1, 0
    qkv, gy = A.operands(B, 1, N, heads, hd, seed=hd + N)
    for i0 in A.excited_tokens(N):
        gb = torch.zeros_like(A.to_blocks_y(gy, heads))
        gb[b0, h0, :, i0] = A.to_blocks_y(gy, heads)[b0, h0, :, i0]
        for fn in (A.reference, A.stand_in):
            _, g = fn(A.to_blocks_qkv(qkv, heads), gb, heads)
            other = torch.ones(B, heads, dtype=torch.bool)
            other[b0, h0] = False
            assert (g[other].abs() == 0).all()
            dq = g[b0, h0, :, 0]
            assert (dq[:, torch.arange(N) != i0].abs() == 0).all()
            assert dq[:, i0].abs().max() > 0 and g[b0, h0, :, 1].abs().min(0).values.max() > 0


def test_excited_tokens():
    assert A.excited_tokens(100) == [0, 96, 99] and A.excited_tokens(225) == [0, 224] and A.excited_tokens(289) == [0, 288]
    assert A.excited_tokens(196) == [0, 192, 195] and A.excited_tokens(256) == [0, 224, 255]
