"""The factored output end on the GPU (tinyedm_amd/csrc/tail_lowrank.hip).

Kernel parity is against the fp64 restatement tests/tail_lowrank_ref.py (pinned to autograd by test_tail_lowrank_cpu.py) on
the SAME operands -- dF and Wc are fp32, X is bf16 -- so the bounds are those of the arithmetic alone:
  * dgrad: an fp32 sum of 9 Co products (at most (9 Co + 2) * 2^-24 of the sum of |terms|: one rounding per fused
    multiply-add and one for the scale) rounded once to bf16: at most half a unit in the last of its 8 significant bits,
    2^(e - 8) for a value in [2^e, 2^(e + 1)) -- the exact bound of ONE round-to-nearest, which a second rounding exceeds;
  * wgrad / expand: an fp32 sum of n terms in some fixed order: at most (n + 8) * 2^-24 of the sum of |terms| whatever
    the order (n = B H W pixels, or the C channels of the expansion)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_lowrank_ref as R  # noqa: E402
from oracle import edm_oracle as O  # noqa: E402

DEV = "cuda"
SHAPES = [(3, 5, 7, 32, 3), (2, 8, 8, 64, 4), (1, 1, 1, 8, 3)]      # B, H, W, C, Co
# the widths above 4, which the reduction runs with 2 channels per thread: the smallest and the largest
WIDE = [(2, 5, 7, 32, 5), (2, 4, 6, 16, 8)]
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def _nchw64(x):     # NHWC (gpu) -> NCHW fp64 (cpu)
    return x.float().cpu().permute(0, 3, 1, 2).double()


def _inputs(B, H, W, C, Co, seed=11):
    g = torch.Generator().manual_seed(seed)
    dF = torch.randn(B, Co, H, W, generator=g)
    Wc = torch.randn(Co, 9, C, generator=g) / 3
    X = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    return dF, Wc, X


@pytest.mark.parametrize("B,H,W,C,Co", SHAPES + WIDE)
def test_dgrad3x3_vs_fp64(ops, B, H, W, C, Co):
    from parity_log import record
    dF, Wc, _ = _inputs(B, H, W, C, Co)
    scale = 0.6
    ga = _nchw64(ops.lowrank_dgrad3x3(dF.to(DEV), Wc.to(DEV), scale))
    ref = R.dgrad(dF.double(), Wc.double(), scale)
    S = R.dgrad(dF.double().abs(), Wc.double().abs(), scale)
    half_ulp = 2.0 ** (torch.floor(torch.log2(ref.abs())) - 8)             # (0 where ref == 0)
    lim = half_ulp + 2 * (9 * Co + 2) * U * S + 1e-30
    worst = ((ga - ref).abs() / lim).max().item()
    print(f"lowrank_dgrad3x3 {B}x{H}x{W}x{C} Co={Co}: worst error / bound = {worst:.3f}")
    record(f"tail_lowrank/dgrad3x3_{B}x{H}x{W}x{C}_co{Co}", worst, 1.0)
    assert ga.shape == ref.shape and worst <= 1.0


@pytest.mark.parametrize("taps", [1, 9])
@pytest.mark.parametrize("B,H,W,C,Co", SHAPES + WIDE)
def test_wgrad_vs_fp64_and_bit_equal(ops, B, H, W, C, Co, taps):
    from parity_log import record
    dF, _, X = _inputs(B, H, W, C, Co)
    aux = torch.randn(B, Co, H, W, generator=torch.Generator().manual_seed(5))
    acc = torch.full((), 0.25, device=DEV)
    G, s = ops.lowrank_wgrad(dF.to(DEV), X.to(DEV), taps, aux=aux.to(DEV), aux_out=acc)
    G2, s2 = ops.lowrank_wgrad(dF.to(DEV), X.to(DEV), taps, aux=aux.to(DEV))
    G3, _ = ops.lowrank_wgrad(dF.to(DEV), X.to(DEV), taps)
    assert torch.equal(G, G2) and torch.equal(G, G3)            # deterministic: two runs are bit-equal
    assert s is acc
    x64 = _nchw64(X)
    ref = R.wgrad(dF.double(), x64, taps)
    S = R.wgrad_abs(dF.double(), x64, taps)
    lim = (B * H * W + 8) * U * S + 1e-30
    worst = ((G.cpu().double() - ref).abs() / lim).max().item()
    print(f"lowrank_wgrad taps={taps} {B}x{H}x{W}x{C} Co={Co}: worst error / bound = {worst:.3f}")
    record(f"tail_lowrank/wgrad_t{taps}_{B}x{H}x{W}x{C}_co{Co}", worst, 1.0)
    assert tuple(G.shape) == (Co, taps, C) and worst <= 1.0
    n = aux.numel()
    alim = (n + 8) * U * aux.double().abs().sum().item()
    assert abs(s2.item() - aux.double().sum().item()) <= alim
    assert abs(acc.item() - 0.25 - aux.double().sum().item()) <= alim + 2 * U      # accumulated (+=) into aux_out


@pytest.mark.parametrize("C,Ci,Co", [(32, 32, 3), (64, 24, 4), (8, 8, 3)])
def test_expansions_vs_fp64(ops, C, Ci, Co):
    g = torch.Generator().manual_seed(2)
    wout = torch.randn(Co, C, generator=g)
    w2 = torch.randn(C, Ci, 3, 3, generator=g).to(torch.bfloat16)                 # the bf16 values the dgrad multiplies
    wd = w2.permute(2, 3, 1, 0).reshape(9, Ci, C).flip(0).contiguous()             # dgrad pack: [8 - t][ci][c]
    Wc = ops.lowrank_expand_wc(wout.to(DEV), wd.to(DEV)).cpu().double()
    ref = R.wc_from(wout.double(), w2.double())
    S = R.wc_from(wout.double().abs(), w2.double().abs())
    assert ((Wc - ref).abs() <= (C + 8) * U * S + 1e-30).all()
    G = torch.randn(Co, 9, Ci, generator=g)
    slab = ops.lowrank_expand_slab(wout.to(DEV), G.to(DEV), 0.6).cpu().double()
    assert tuple(slab.shape) == (1, 9, C, Ci)
    ref = R.expand_dw(wout.double(), G.double(), 0.6)                               # (C, Ci, 3, 3)
    S = R.expand_dw(wout.double().abs(), G.double().abs(), 0.6)
    got = slab[0].permute(1, 2, 0).reshape(C, Ci, 3, 3)                             # [t][c][i] -> [c][i][t]
    assert ((got - ref).abs() <= (Co + 4) * U * S + 1e-30).all()


@pytest.mark.parametrize("pdrop", [0.0, 0.13])
@pytest.mark.parametrize("B,H,W,C,Co", SHAPES)
def test_fused_modulation_backward_is_the_two_launch_form(ops, B, H, W, C, Co, pdrop):
    """the fused form = lowrank_dgrad3x3 followed by mod_silu_drop_bwd: gr bit for bit (the same arithmetic on the same
    bf16 ga2), the modulation sums up to the order of their atomics; with the dropout mask regenerated (Philox), with NaN
    marks in r1, and with the raw sums left in a shared gm buffer"""
    dF, Wc, X = _inputs(B, H, W, C, Co, seed=23)
    g = torch.Generator().manual_seed(4)
    lin = (torch.randn(B, C + 16, generator=g) * 0.3).to(DEV)[:, 8:8 + C]
    gain = torch.tensor(0.8, device=DEV)
    seed, sub, step = 0x1234567812345678, 9, 3
    r1 = X.to(DEV)
    ga = ops.lowrank_dgrad3x3(dF.to(DEV), Wc.to(DEV), 0.6)
    gr0, glin0, gg0 = ops.mod_silu_drop_bwd(r1, lin, gain, ga, pdrop, seed, sub, step)
    gr1, glin1, gg1 = ops.lowrank_dgrad3x3_modbwd(dF.to(DEV), Wc.to(DEV), 0.6, r1, lin, gain, pdrop, seed, sub, step)
    assert torch.equal(gr0, gr1)
    scale = glin0.abs().max().item() + 1e-30
    assert (glin0 - glin1).abs().max().item() <= 1e-5 * scale * max(1, H * W // 16)
    assert abs(gg0.item() - gg1.item()) <= 1e-4 * (abs(gg0.item()) + scale)
    if pdrop > 0:
        keep = ops.dropout_mask(r1.numel(), pdrop, seed, sub, step, DEV).view_as(r1).bool()
        marked = torch.where(keep, r1, torch.full_like(r1, float("nan")))
        gm = torch.zeros(B, C + 8, device=DEV)
        gr2, none1, none2 = ops.lowrank_dgrad3x3_modbwd(dF.to(DEV), Wc.to(DEV), 0.6, marked, lin, gain, pdrop, seed, sub, step,
                                                        gm_out=gm[:, 8:], u_marked=True)
        assert none1 is None and none2 is None and torch.equal(gr0, gr2)
        assert torch.isfinite(gm).all() and (gm[:, :8] == 0).all()
        assert ((gm[:, 8:] * gain - glin0).abs().max().item()) <= 1e-5 * scale * max(1, H * W // 16)


def test_conv_out_bwd_x_alone_and_df(ops):
    """edm_conv_out_bwd without its weight-gradient half writes the same gx; dF, aux of lowrank_df against fp64"""
    B, H, W, C, Co = 3, 5, 7, 32, 3
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16).to(DEV)
    wh = (torch.randn(Co, C, generator=g) / 6).to(DEV)
    gain_out = torch.tensor(0.7, device=DEV)
    Fraw, dD = torch.randn(B, Co, H, W, generator=g).to(DEV), torch.randn(B, Co, H, W, generator=g).to(DEV)
    sigma = (torch.rand(B, generator=g) + 0.2).to(DEV)
    gx0, gw0, gg0 = ops.conv_out_bwd(x, wh, gain_out, Fraw, dD, sigma, 0.5)
    gx1 = ops.conv_out_bwd_x(wh, gain_out, dD, sigma, 0.5, C)
    assert torch.equal(gx0, gx1)
    dF, aux = ops.lowrank_df(dD, Fraw, gain_out, sigma, 0.5)
    s = sigma.double().cpu().view(B, 1, 1, 1)
    cout = s * 0.5 / (s * s + 0.25).sqrt()
    assert torch.allclose(dF.cpu().double(), dD.cpu().double() * cout * 0.7, rtol=1e-6, atol=0)
    assert torch.allclose(aux.cpu().double(), dD.cpu().double() * cout * Fraw.cpu().double(), rtol=1e-6, atol=0)
    # the one-tap reduction is conv_out's weight gradient, its aux sum the gain's
    G, sg = ops.lowrank_wgrad(dF, x, 1, aux=aux)
    assert torch.allclose(G.view(Co, C), gw0, rtol=1e-4, atol=1e-5 * gw0.abs().max().item())
    assert abs(sg.item() - gg0.item()) <= 1e-4 * abs(gg0.item()) + 1e-6


# ------------------------------------------------------------------------------------------------ block level
class _Net:
    """a one-level network (64 channels, 8x8) whose last decoder block + conv_out run alone, gradients in a flat arena"""

    def __init__(self):
        import tinyedm_amd as T
        from tinyedm_amd import networks as N
        from tinyedm_amd.ema import FlatArena
        torch.manual_seed(0)
        self.N, self.ops = N, T.ops
        den = N.Denoiser(3, 3, ("Enc",), ("Dec",), (64,), (64,), (False,), 0.13, 0.5, 0.3, 0.3, 64, 2)
        with torch.no_grad():
            den.gain_out.fill_(0.7)
            den.decoder_blocks[-1].gain.fill_(0.9)
        self.den = den.to(DEV).train()
        self.blk = self.den.decoder_blocks[-1]
        assert self.blk._tail_last and not self.den.encoder_blocks[0]._tail_last
        self.arena = FlatArena(list(self.den.parameters()))
        self.state = {k: v.clone() for k, v in self.den.state_dict().items()}
        g = torch.Generator().manual_seed(1)
        B = 2
        self.u = torch.randn(B, 8, 8, 64, generator=g).to(torch.bfloat16).to(DEV)
        self.emb = torch.randn(B, 64, generator=g).to(DEV)
        self.noisy = torch.randn(B, 3, 8, 8, generator=g).to(DEV)
        self.sigma = (torch.rand(B, generator=g) + 0.3).to(DEV)
        self.gD = torch.randn(B, 3, 8, 8, generator=g).to(DEV)
        self.seed = 4321

    def named(self):
        out = {"blk." + k: p for k, p in self.blk.named_parameters()}
        out["conv_out.weight"] = self.den.conv_out.weight
        out["gain_out"] = self.den.gain_out
        return out

    def run(self, via=None, upto_block_output=False):
        N = self.N
        self.den.load_state_dict(self.state)
        self.arena.zero_grad()
        N.manual_seed(self.seed)
        N.reset_backward_state()
        u = N._tag(self.u.clone().requires_grad_(True))
        emb = self.emb.clone().requires_grad_(True)
        out = self.blk(u, emb)
        mid = out if via is None else N._tag(via(out))
        D = N._ConvOutFn.apply(mid, self.den.conv_out.weight, self.den.gain_out, self.noisy, self.sigma, self.den)
        if upto_block_output:
            (gmid,) = torch.autograd.grad((D * self.gD).sum(), mid)
            return gmid
        (D * self.gD).sum().backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in self.named().items()}
        grads["input"] = u.grad.detach().clone()
        grads["embedding"] = emb.grad.detach().clone()
        return grads

    def reference(self):
        """fp64 autograd of the oracle's block + the 1x1 output conv on the same inputs, the weights the forward left
        (normalised in place) and the kernel's own dropout mask"""
        blk, ops = self.blk, self.ops
        P = {"b." + k: p.detach().cpu().double().requires_grad_(True) for k, p in blk.named_parameters()}
        wout = self.den.conv_out.weight.detach().cpu().double().requires_grad_(True)
        gout = self.den.gain_out.detach().cpu().double().requires_grad_(True)
        x = self.u.float().cpu().permute(0, 3, 1, 2).double().requires_grad_(True)
        emb = self.emb.cpu().double().requires_grad_(True)
        mask = ops.dropout_mask(self.u.numel(), blk.dropout_rate, self.seed, blk.rng_sub, 0, DEV)
        mask = mask.view(self.u.shape).permute(0, 3, 1, 2).cpu().double()
        out = O.decoder_block(P, "b.", x, emb, None, False, False, 2, blk.add_factor, blk.dropout_rate, True, O._ident, mask)
        s = self.sigma.cpu().double().view(-1, 1, 1, 1)
        c_skip, c_out = 0.25 / (s * s + 0.25), s * 0.5 / (s * s + 0.25).sqrt()
        D = F.conv2d(out, O.effective_weight(wout)) * gout * c_out + self.noisy.cpu().double() * c_skip
        (D * self.gD.cpu().double()).sum().backward()
        ref = {"blk." + k[2:]: v.grad for k, v in P.items()}
        ref.update({"conv_out.weight": wout.grad, "gain_out": gout.grad, "embedding": emb.grad,
                    "input": x.grad.permute(0, 2, 3, 1)})
        return ref


@pytest.fixture(scope="module")
def net(ops):
    return _Net()


def _count_lowrank(monkeypatch, ops):
    calls = {"dgrad": 0, "wgrad": 0}
    d0, w0 = ops.lowrank_dgrad3x3_modbwd, ops.lowrank_wgrad

    def d(*a, **k):
        calls["dgrad"] += 1
        return d0(*a, **k)

    def w(dF, X, taps, **k):
        calls["wgrad"] += taps == 9
        return w0(dF, X, taps, **k)
    monkeypatch.setattr(ops, "lowrank_dgrad3x3_modbwd", d)
    monkeypatch.setattr(ops, "lowrank_wgrad", w)
    return calls


def _err(a, b):
    return ((a.cpu().double() - b).norm() / (b.norm() + 1e-300)).item()


def test_block_ab_error_not_larger(net, ops, monkeypatch):
    """last decoder block + conv_out, dropout on, r1 NaN-marked, switch on and off: every parameter gradient and the
    block's input gradients against the fp64 reference.  The factored path removes one bf16 rounding (that of g_h) and adds
    none, so its error must not be larger than today's; 10 % margin for summation-order ties."""
    from parity_log import record
    N = net.N
    assert N.U_MARKS and ops.FUSE_MOD
    calls = _count_lowrank(monkeypatch, ops)
    monkeypatch.setattr(N, "TAIL_LOWRANK", True)
    on = net.run()
    assert calls == {"dgrad": 1, "wgrad": 1} and not N._tail_slot
    monkeypatch.setattr(N, "TAIL_LOWRANK", False)
    off = net.run()
    assert calls == {"dgrad": 1, "wgrad": 1}
    ref = net.reference()
    assert set(on) == set(off) == set(ref)
    for k in sorted(ref):
        assert torch.isfinite(on[k]).all() and ref[k].abs().max() > 0, k
        e_on, e_off = _err(on[k], ref[k]), _err(off[k], ref[k])
        print(f"tail low-rank A/B {k}: error vs fp64 on {e_on:.4e}  off {e_off:.4e}")
        record(f"tail_lowrank/block_ab/{k}", e_on, 1.1 * e_off)
        assert e_on <= 1.1 * e_off, f"{k}: factored path {e_on:.4e} > 1.1 x today's {e_off:.4e}"


# gradients that no atomically-accumulated sum feeds: equal bit for bit between two runs of today's path; the modulation
# sums behind the embed / gain gradients are added with float atomics (today's path too) and agree to rounding only
_EXACT = ("input", "blk.conv_3x3_1.weight", "blk.conv_3x3_2.weight")


def _same_as_today(got, today):
    for k in today:
        if k in _EXACT:
            assert torch.equal(got[k], today[k]), k
        else:
            assert torch.allclose(got[k], today[k], rtol=1e-4, atol=1e-6 * today[k].abs().max().item()), k


def test_fallback_switch_off_and_foreign_gout(net, ops, monkeypatch):
    N = net.N
    calls = _count_lowrank(monkeypatch, ops)
    monkeypatch.setattr(N, "TAIL_LOWRANK", False)
    today = net.run()
    again = net.run()
    assert calls == {"dgrad": 0, "wgrad": 0} and not N._tail_slot            # EDM_TAIL_LOWRANK=0: none of the new launches
    _same_as_today(again, today)

    class CloneGrad(torch.autograd.Function):       # the block receives a COPY of the gradient conv_out returned
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            return g.clone()
    monkeypatch.setattr(N, "TAIL_LOWRANK", True)
    got = net.run(via=CloneGrad.apply)
    assert calls == {"dgrad": 0, "wgrad": 0} and not N._tail_slot
    _same_as_today(got, today)          # (conv_out's own gradients took the one-tap form: to rounding, like the atomic sums)


def test_slot_empty_after_truncated_backward(net, ops, monkeypatch):
    N = net.N
    monkeypatch.setattr(N, "TAIL_LOWRANK", True)
    calls = _count_lowrank(monkeypatch, ops)
    g = net.run(upto_block_output=True)            # the backward stops at the block's output: nobody takes the slot
    torch.cuda.synchronize()
    assert g.shape == net.u.shape and calls["dgrad"] == 0
    assert not N._tail_slot
    N._tail_slot[0] = ("stale",)                   # an exception inside autograd leaves the end-of-backward callback unrun
    N.reset_backward_state()
    assert not N._tail_slot


def test_fallback_fragment_major_pack(ops, monkeypatch):
    """at the shape whose 8x8 layers run on k_conv3x3_s the last block's dgrad pack is fragment-major: the block takes
    today's path, bit for bit"""
    from tinyedm_amd import networks as N
    from tinyedm_amd.ema import FlatArena
    B, C = 64, 256
    assert ops.uses_s_kernel(B, 8, 8, C, C), "no 8x8 shape on k_conv3x3_s: this test needs another shape"
    torch.manual_seed(0)
    den = N.Denoiser(3, 3, ("Enc",), ("Dec",), (C,), (C,), (False,), 0.13, 0.5, 0.3, 0.3, 64, 2)
    with torch.no_grad():
        den.gain_out.fill_(0.7)
    den = den.to(DEV).train()
    arena = FlatArena(list(den.parameters()))
    state = {k: v.clone() for k, v in den.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    noisy, sigma = torch.randn(B, 3, 8, 8, generator=g).to(DEV), (torch.rand(B, generator=g) + 0.3).to(DEV)
    emb, gD = torch.randn(B, 64, generator=g).to(DEV), torch.randn(B, 3, 8, 8, generator=g).to(DEV)
    calls = _count_lowrank(monkeypatch, ops)
    blk = den.decoder_blocks[-1]

    def run(flag):
        monkeypatch.setattr(N, "TAIL_LOWRANK", flag)
        den.load_state_dict(state)
        arena.zero_grad()
        N.manual_seed(99)
        (den(noisy, sigma, emb) * gD).sum().backward()
        torch.cuda.synchronize()
        return {k: p.grad.detach().clone() for k, p in blk.named_parameters()}
    today = run(False)
    assert getattr(blk.conv_3x3_2._cache[1], "_edm_frag", False), "the dgrad pack is not fragment-major here"
    got = run(True)
    assert calls == {"dgrad": 0, "wgrad": 0} and not N._tail_slot
    for k in ("conv_3x3_1.weight", "conv_3x3_2.weight"):
        assert torch.equal(got[k], today[k]), k


def test_supported_query_and_silent_fallback(net, ops, monkeypatch):
    """shapes whose LDS tables do not fit are refused by the host query, and a block whose shape is refused takes today's
    path without raising"""
    assert ops.lowrank_supported(256, 3, 32, 9) and ops.lowrank_supported(256, 4, 32, 9) and ops.lowrank_supported(64, 8, 8, 9)
    assert ops.lowrank_supported(256, 8, 32, 1)
    assert not ops.lowrank_supported(256, 8, 32, 9) and not ops.lowrank_supported(256, 6, 32, 9)      # 73.7 KB / > 60 KB of tables
    assert not ops.lowrank_supported(256, 9, 32, 1) and not ops.lowrank_supported(260, 3, 32, 9)
    N = net.N
    calls = _count_lowrank(monkeypatch, ops)
    monkeypatch.setattr(N, "TAIL_LOWRANK", False)
    today = net.run()
    monkeypatch.setattr(N, "TAIL_LOWRANK", True)
    monkeypatch.setattr(ops, "lowrank_supported", lambda C, Co, W, taps: taps == 1)
    got = net.run()
    assert calls == {"dgrad": 0, "wgrad": 0} and not N._tail_slot
    _same_as_today(got, today)
    monkeypatch.setattr(ops, "lowrank_supported", lambda C, Co, W, taps: False)
    got = net.run()
    assert calls == {"dgrad": 0, "wgrad": 0} and not N._tail_slot
    _same_as_today(got, today)
