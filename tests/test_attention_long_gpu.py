"""Cosine attention above 256 tokens (csrc/attention_long.hip: tiled fixed-offset softmax forward, two-kernel backward).

Kernel level: the oracle form and the limits of tests/test_kernels_gpu.py::test_attention_fwd_bwd (bf16-rounded q / k / v,
softmax rounded to bf16, autograd) on shapes that are each the smallest at which something new can go wrong; logits at both
ends of the fixed offset; a bounds check with sentinels; bit-reproducible gradients; refusals.
Network level: a small net with "A" blocks at 32x32 (1024 tokens) -- its training gradients and its evaluation forward against
the oracle, and one captured training step against the eager one.  Before these kernels that net died in its first forward
with "at most 256 tokens"."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import edm_oracle as O
from test_kernels_gpu import DEV, _qkv_perm, close_bf16, nchw, nhwc, q, rel

import attention_long_ref as R

FWD, BWD = dict(l2=6e-3, mx=3e-2), dict(l2=1.5e-2, mx=6e-2)      # test_attention_fwd_bwd's limits

SHAPES = [
    (1, 17, 17, 1, 64),     # 289 = 4*64 + 33: ragged key tile; two more query blocks after the first, the last with 33 rows
    (2, 18, 18, 2, 64),     # 324 = 5*64 + 4: a 4-row tail; more than one sample and head (grid indexing)
    (1, 24, 24, 1, 32),     # 576: whole key tiles, the last query block half full, the smallest head_dim
    (1, 17, 17, 1, 144),    # the streamed head dims; 144 carries the V zero-padding to 160
    (1, 20, 20, 1, 128),
    (1, 17, 17, 2, 192),
    (2, 32, 32, 1, 64),     # the 32x32 map
    (1, 64, 64, 1, 64),     # 4096: the largest map the convolutions allow
]
EXTREME = [(1, 32, 32, 1, 64), (1, 20, 20, 1, 192)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def _to_ref_layout(qq, kk, vv):
    """q, k, v [B, heads, N, d] -> the reference's qkv channel order [B, 3C, N] (channel = head*3d + dd*3 + which)"""
    B, heads, N, d = qq.shape
    return torch.stack((qq, kk, vv), dim=-1).permute(0, 1, 3, 4, 2).reshape(B, heads * d * 3, N)


@functools.lru_cache(maxsize=None)
def _case(B, H, W, heads, hd, extreme=False):
    """operands on the GPU and the reference of test_attention_fwd_bwd, computed once per shape and left unchanged:
    (qkv packed NHWC, gy NHWC, y_ref, gqkv_ref in packed order, fp64 log-sum-exp [B, heads, N])"""
    g = torch.Generator().manual_seed(B + H + heads + hd)
    C, N = hd * heads, H * W
    if extreme:
        raw = _to_ref_layout(*R.extreme_qkv(B, heads, N, hd, g, dtype=torch.float32)).view(B, 3 * C, H, W)
    else:
        raw = torch.randn(B, 3 * C, H, W, generator=g)
    qkv_ref_layout = q(raw)
    gy = q(torch.randn(B, C, H, W, generator=g))
    x = qkv_ref_layout.clone().requires_grad_(True)
    t = O.q_bf16(O.rms_div(x.view(B, heads, hd, 3, N), [2]))
    qq, kk, vv = t.unbind(3)
    s = torch.einsum("bhdi,bhdj->bhij", qq, kk) / math.sqrt(hd)
    p = O.q_bf16(torch.softmax(s, dim=-1))
    y_ref = torch.einsum("bhij,bhdj->bhdi", p, vv).reshape(B, C, H, W)
    y_ref.backward(gy)
    with torch.no_grad():
        s64 = torch.einsum("bhdi,bhdj->bhij", qq.double(), kk.double()) / math.sqrt(hd)
        lse = torch.logsumexp(s64, dim=-1)
    perm = _qkv_perm(C, heads)
    return nhwc(qkv_ref_layout[:, perm]), nhwc(gy), y_ref.detach(), x.grad[:, perm].clone(), lse, s64.min().item(), s64.max().item()


def _run_long(ops, qkv, gy, heads):
    y, stat = ops.attention_long_fwd(qkv, heads)
    gqkv = ops.attention_long_bwd(qkv, y, gy, stat, heads)
    return y, stat, gqkv


@pytest.mark.parametrize("B,H,W,heads,hd", SHAPES)
def test_attention_long_fwd_bwd(ops, B, H, W, heads, hd):
    qkv, gy, y_ref, gqkv_ref, lse, _, _ = _case(B, H, W, heads, hd)
    y, stat, gqkv = _run_long(ops, qkv, gy, heads)
    close_bf16(nchw(y), y_ref, **FWD)
    close_bf16(nchw(gqkv), gqkv_ref, **BWD)
    assert torch.isfinite(stat).all()
    # evaluation: no statistics wanted, same output bits
    y2, none = ops.attention_long_fwd(qkv, heads, want_stat=False)
    assert none is None and torch.equal(y2, y)


def test_attention_long_and_short_kernels_at_256_tokens(ops):
    """N = 256, the largest map of attention.hip: both kernel families within the limits of the same reference"""
    B, H, W, heads, hd = 3, 16, 16, 2, 64
    qkv, gy, y_ref, gqkv_ref, _, _, _ = _case(B, H, W, heads, hd)
    y, _, gqkv = _run_long(ops, qkv, gy, heads)
    close_bf16(nchw(y), y_ref, **FWD)
    close_bf16(nchw(gqkv), gqkv_ref, **BWD)
    y_s = ops.attention_fwd(qkv, heads)
    gqkv_s = ops.attention_bwd(qkv, y_s, gy, heads)
    close_bf16(nchw(y_s), y_ref, **FWD)
    close_bf16(nchw(gqkv_s), gqkv_ref, **BWD)


@pytest.mark.parametrize("B,H,W,heads,hd", EXTREME)
def test_attention_long_extreme_logits(ops, B, H, W, heads, hd):
    """the softmax has no running maximum: it rests on |q.k| / sqrt(d) <= sqrt(d).  k = q and the second half of the tokens
    negated puts logits at +sqrt(d) and -sqrt(d) into every row; stat is the row's log-sum-exp."""
    qkv, gy, y_ref, gqkv_ref, lse, smin, smax = _case(B, H, W, heads, hd, True)
    assert smax > 0.99 * math.sqrt(hd) and smin < -0.99 * math.sqrt(hd)
    y, stat, gqkv = _run_long(ops, qkv, gy, heads)
    close_bf16(nchw(y), y_ref, **FWD)
    close_bf16(nchw(gqkv), gqkv_ref, **BWD)
    err = (stat.double().cpu() - lse).abs().max().item()
    print(f"stat vs fp64 log-sum-exp: {err:.3e}")
    assert err <= 1e-4, err


def _guarded(n, dtype, sentinel, pad=64):
    """an n-element interior slice of a larger buffer filled with `sentinel`"""
    big = torch.full((n + 2 * pad,), sentinel, dtype=dtype, device=DEV)
    return big, big[pad:pad + n]


def test_attention_long_writes_nothing_outside_its_outputs(ops):
    """y, stat, gqkv and work as interior slices of sentinel-filled buffers at the ragged 289-token shape (valid arguments:
    a plain bounds check)"""
    B, H, W, heads, hd = 1, 17, 17, 1, 64
    C, N = hd * heads, H * W
    qkv, gy, y_ref, gqkv_ref, _, _, _ = _case(B, H, W, heads, hd)
    qkv0, gy0 = qkv.clone(), gy.clone()
    bufs = {"y": _guarded(B * N * C, torch.bfloat16, 768.0), "stat": _guarded(B * heads * N, torch.float32, 12345.0),
            "gqkv": _guarded(B * N * 3 * C, torch.bfloat16, 768.0), "work": _guarded(B * heads * N, torch.float32, 12345.0)}
    p, st = ops._p, ops._stream()
    y, stat, gqkv, work = (bufs[k][1] for k in ("y", "stat", "gqkv", "work"))
    ops._lib.call("edm_attention_long_fwd", p(qkv), p(y), p(stat), B, N, C, heads, st)
    ops._lib.call("edm_attention_long_bwd", p(qkv), p(y), p(gy), p(stat), p(gqkv), p(work), B, N, C, heads, st)
    torch.cuda.synchronize()
    for name, (big, view) in bufs.items():
        sentinel = big[0].item()
        n = view.numel()
        assert (big[:64] == sentinel).all() and (big[64 + n:] == sentinel).all(), f"{name}: write outside the output"
        assert torch.isfinite(view.float()).all() and not (view == sentinel).all(), f"{name}: output not written"
    assert torch.equal(qkv, qkv0) and torch.equal(gy, gy0)
    close_bf16(nchw(y.view(B, H, W, C)), y_ref, **FWD)
    close_bf16(nchw(gqkv.view(B, H, W, 3 * C)), gqkv_ref, **BWD)


def test_attention_long_bwd_is_bit_reproducible(ops):
    """two kernels, no atomics: every gradient element has one owner and one summation order"""
    qkv, gy, *_ = _case(2, 18, 18, 2, 64)
    y, stat = ops.attention_long_fwd(qkv, 2)
    a = ops.attention_long_bwd(qkv, y, gy, stat, 2)
    b = ops.attention_long_bwd(qkv, y, gy, stat, 2)
    assert torch.equal(a, b)


def test_attention_long_refusals(ops):
    assert ops._lib.call("edm_attention_long_supported", 1024, 48, 1) == 0
    assert not ops.attention_long_supported(1024, 96, 2)
    for hd in (64, 32, 128, 144, 192):
        assert ops._lib.call("edm_attention_long_supported", 1024, 2 * hd, 2) == 1
        assert ops.attention_long_supported(1, hd, 1)
    assert not ops.attention_long_supported(0, 64, 1)
    qkv = torch.zeros(1, 17, 17, 3 * 48, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ops._lib.HipKernelError, match="status -3.*head_dim 48 is not built"):
        ops.attention_long_fwd(qkv, 1)
    y = torch.full((1, 17, 17, 48), 768.0, dtype=torch.bfloat16, device=DEV)
    gqkv_probe = None
    with pytest.raises(ops._lib.HipKernelError, match="status -3.*head_dim 48 is not built"):
        gqkv_probe = ops.attention_long_bwd(qkv, y, y, torch.zeros(1, 1, 289, device=DEV), 1)
    assert gqkv_probe is None
    with pytest.raises(ops._lib.HipKernelError, match="bad args"):          # C not a multiple of heads
        ops.attention_long_fwd(torch.zeros(1, 17, 17, 3 * 64, dtype=torch.bfloat16, device=DEV), 3)


# ---------------------------------------------------------------------------------------------- through the network
NET_SHAPE = (2, 3, 32, 32)


def _net_cfgs(dropout=0.1, channels=3):
    """attention on both levels of the encoder and the decoder: 1024 tokens at 32x32 (64 channels, head_dim 32: the long
    kernels) and 256 tokens at 16x16 (128 channels, head_dim 64: attention.hip, as before)"""
    e = O.EmbeddingCfg(fourier_dim=32, embedding_dim=64, num_classes=10)
    d = O.DenoiserCfg(
        in_channels=channels, out_channels=channels,
        encoder_block_types=["EncA", "EncD", "EncA"],
        decoder_block_types=["DecA", "DecA", "DecU", "DecA", "DecA"],
        encoder_out_channels=[64, 128, 128],
        decoder_out_channels=[128, 128, 128, 64, 64],
        skip_connections=[True, True, False, True, True],
        dropout_rate=dropout, sigma_data=0.5, embedding_dim=64, num_heads=2)
    return e, d


def test_network_with_attention_at_32x32_gradients_vs_oracle(ops, monkeypatch):
    """every per-parameter gradient of a training step against the bf16 oracle (tests/test_gradparity_gpu.py, default
    limits); the long kernels must have run in both directions"""
    from test_gradparity_gpu import _grad_parity
    calls = []
    for name in ("attention_long_fwd", "attention_long_bwd"):
        orig = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    ecfg, dcfg = _net_cfgs()
    _grad_parity("attn_long_32x32", ecfg, dcfg, NET_SHAPE, -1.2, 1.2, 51, 83)
    assert calls.count("attention_long_fwd") == 3 and calls.count("attention_long_bwd") == 3, calls


def test_network_with_attention_at_32x32_eval_vs_oracle(ops):
    """eval mode: the bf16 path against the bf16 oracle forward, the f32 / f32x3 paths (edm_f32_attention above 256 tokens)
    against the fp32 oracle -- tests/test_configs_gpu.py's check and limits"""
    from test_configs_gpu import eval_parity
    ecfg, dcfg = _net_cfgs(dropout=0.0)
    eval_parity(ecfg, dcfg, NET_SHAPE, seed=13, tol=3e-2)


def test_attention_module_above_256_tokens_keeps_stat_only_for_a_backward(ops, monkeypatch):
    """`CosineAttention` at 32x32: a forward that a backward can follow keeps the log-sum-exp, one under torch.no_grad() does
    not ask for it, and a backward that arrives without it is an error (the rule of the fused path)"""
    from tinyedm_amd import networks as N
    g = torch.Generator().manual_seed(4)
    att = N.CosineAttention(64, 2).to(DEV).train()
    x0 = nhwc(q(torch.randn(2, 64, 32, 32, generator=g)))
    gy = nhwc(q(torch.randn(2, 64, 32, 32, generator=g)))
    calls = []
    orig = ops.attention_long_fwd
    monkeypatch.setattr(ops, "attention_long_fwd", lambda *a, **k: (calls.append(k["want_stat"]), orig(*a, **k))[1])
    x = x0.clone().requires_grad_(True)
    y = att.forward_nhwc(x)
    y.backward(gy)
    with torch.no_grad():
        y2 = att.forward_nhwc(x0)
    torch.cuda.synchronize()
    assert calls == [True, False], calls
    assert rel(y2.float(), y.detach().float()) < 4e-3        # (each training forward renormalises the weights in place)
    assert torch.isfinite(x.grad.float()).all() and x.grad.float().abs().max() > 0
    x = x0.clone().requires_grad_(True)
    out = N._AttnFn.apply(x, att.qkv_conv.weight, att.out_conv.weight, att, None, False)
    with pytest.raises(RuntimeError, match="softmax statistics"):
        out.backward(gy)


def _build_model(seed, channels):
    import tinyedm_amd as T
    from tinyedm_amd import networks as N
    ecfg, dcfg = _net_cfgs(channels=channels)
    N._rng_sub_counter[0] = 0
    T.manual_seed(seed)
    torch.manual_seed(seed)
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), dcfg.dropout_rate, dcfg.sigma_data,
                     dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    with torch.no_grad():
        den.gain_out.fill_(0.7)
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=True, use_uncertainty=False,
                  steady_steps=3, rampup_steps=3, scheduler_interval="step", lr=2e-3, ema_length=0.13)
    model = model.to(DEV).train()
    from tinyedm_amd.ema import EMAOptimizer
    base = model.configure_optimizers()["optimizer"]
    for pg in base.param_groups:
        pg["lr"] = 0.0
    return model, EMAOptimizer(base, device=DEV, gamma=T.sigma_rel_to_gamma(0.13))


def test_captured_training_step_with_attention_at_32x32(ops):
    """the same blocks through tinyedm_amd.graph.CapturedTrainStep: the captured and replayed steps give the eager steps'
    losses bit for bit.  Two things make the loss a reproducible function of the step's forward pass, so that "bit for bit"
    is a statement about the captured kernels and not about the order of fp32 atomics:
      * the learning rate is 0 (the modulation / gain gradients of a backward are summed with atomics, so two eager runs
        with a learning rate already disagree in the last bits of their weights); noise and dropout still change per step;
      * the images have one channel, 2 x 1 x 32 x 32 = 2048 elements: the loss kernel (edm_weighted_mse) adds one partial
        sum per workgroup of 1024 elements to the loss with an atomic, and two partial sums commute where three do not --
        with three channels two EAGER runs of this test differ by one ulp of the loss (1.2355262 vs 1.2355261 was seen)."""
    from tinyedm_amd.graph import CapturedTrainStep
    shape = (2, 1, 32, 32)
    g = torch.Generator().manual_seed(7)
    batches = [((0.5 * torch.randn(*shape, generator=g)).to(DEV), torch.randint(0, 10, (shape[0],), generator=g).to(DEV))
               for _ in range(4)]
    model_e, opt_e = _build_model(17, shape[1])
    opt_e.zero_grad()
    losses_e = []
    for b in batches:
        loss = model_e.training_step(b, 0)
        loss.backward()
        opt_e.step()
        opt_e.zero_grad()
        losses_e.append(float(loss.detach()))
    model_g, opt_g = _build_model(17, shape[1])
    opt_g.zero_grad()
    step = CapturedTrainStep(model_g, opt_g)
    losses_g = [float(step(b)) for b in batches]
    assert len(step._graphs) == 1                                   # the last two steps were replays of one graph
    print("captured", losses_g, "eager", losses_e)
    assert losses_g == losses_e, (losses_g, losses_e)
    assert len(set(losses_g)) == len(losses_g)
