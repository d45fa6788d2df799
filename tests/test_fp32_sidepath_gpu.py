"""The fp32 side path of every training step and sampler evaluation against fp64 on the same fp32 operands: the Linear
GEMM (csrc/linear.hip sgemm: 32 x 64 tile, 64 x 64 tile, split-K with and without the clearing memset), the noise / class
embedding, the modulation-gradient finish of all blocks (edm_mod_finish_multi), the deferred ScaleLong gate weight
gradients (edm_skip_gate_wgrad_multi) and the loss (edm_weighted_mse).

Bounds are the order-independent fp32 ones with a factor-2 margin: a sum of n products is within
gamma = 2 (n + S + 2) u of the exact result, times the sum of the magnitudes of its terms (u = 2^-24, S = partial sums added
by atomics), so they cannot flake; where that worst case is too loose to see a small fault (long sums) a relative-L2
limit of 1e-5 is required as well.  The worst ratio of error to bound of every check goes to parity_log."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import edm_oracle as O
from parity_log import record

DEV = "cuda"
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


def check_bound(name, got, ref, bound, l2=None):
    """|got - ref| <= bound elementwise (an exact zero error passes a zero bound); optionally rel L2 <= l2"""
    got, ref, bound = got.double(), ref.double(), bound.double()
    assert torch.isfinite(got).all(), f"{name}: non-finite result"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = ratio.max().item() if ratio.numel() else 0.0
    record("fp32_sidepath/" + name, worst, 1.0)
    assert worst <= 1.0, f"{name}: error / bound = {worst:.3g} (max err {err.max().item():.3e})"
    if l2 is not None:
        r = rel(got, ref)
        assert r <= l2, f"{name}: rel L2 {r:.3e} > {l2:.0e}"


def randn(g, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=g)).to(DEV)


# ------------------------------------------------------------------------------------------------ Linear GEMM
def _gemm_operands(op, A, B):
    """(left, right) of the GEMM edm_linear_<op> runs, as fp64 matrices: C = left @ right"""
    if op == "fwd":         # Y[M,N] = X[M,K] W[N,K]^T
        return A.double(), B.double().t()
    if op == "dgrad":       # dX[M,K] = dY[M,N] W[N,K]
        return A.double(), B.double()
    return A.double().t(), B.double()   # wgrad: dW[N,K] = dY[M,N]^T X[M,K]


def _operands(g, op, M, N, K):
    if op == "fwd":
        return randn(g, M, K), randn(g, N, K), (M, N)
    if op == "dgrad":
        return randn(g, M, N), randn(g, N, K), (M, K)
    return randn(g, M, N), randn(g, M, K), (N, K)


def _kshares(gk, splits):
    """K range of every split-K share (linear.hip k_sgemm_mfma: kper = ceil(ceil(K / splits) / 32) * 32)"""
    kper = ((gk + splits - 1) // splits + 31) // 32 * 32
    return [(z * kper, min(gk, z * kper + kper)) for z in range(splits)]


def run_linear(ops, name, op, M, N, K, g, c0=None, accumulate=None, expect=None):
    """one edm_linear_<op>(M, N, K) launch against fp64.  c0: C pre-filled with these values (accumulate given: called
    through _lib.call with that flag; NaN-filled C with accumulate=0 must be overwritten), else through ops.linear_<op>."""
    from tinyedm_amd import _lib
    acc_flag = {"fwd": 0, "dgrad": 1, "wgrad": 0}[op] if accumulate is None else accumulate
    rows, splits = ops.linear_plan(op, M, N, K, acc_flag)
    if expect is not None:
        assert (rows, splits) == expect, f"{name}: plan {(rows, splits)} is not the branch {expect} this case is for"
    A, B, cshape = _operands(g, op, M, N, K)
    if c0 is None and accumulate is None:
        C = {"fwd": ops.linear_fwd, "dgrad": ops.linear_dgrad, "wgrad": ops.linear_wgrad}[op](A, B)
        base = torch.zeros(cshape, dtype=torch.float64, device=DEV)
    else:
        C = c0.clone()
        assert C.shape == cshape and C.is_contiguous()
        base = torch.zeros_like(c0, dtype=torch.float64) if acc_flag == 0 else c0.double()
        if op == "fwd":
            _lib.call("edm_linear_fwd", ops._p(A), ops._p(B), ops._p(C), M, N, K, ops._stream())
        else:
            _lib.call("edm_linear_" + op, ops._p(A), ops._p(B), ops._p(C), M, N, K, acc_flag, ops._stream())
    L, R = _gemm_operands(op, A, B)
    ref = base + L @ R
    bound = 2 * (L.shape[1] + splits + 2) * U * (L.abs() @ R.abs()) + U * base.abs()
    check_bound(name, C, ref, bound, l2=1e-5)
    return rows, splits


SUM_C_CIFAR = 21 * 256           # the batched embed Linear of all 21 blocks of the CIFAR-10 net


def _sum_c_imagenet():
    from tinyedm_amd import networks
    return sum(networks.get_encoder_out_channels()) + sum(networks.get_decoder_out_channels())


# (name, op, M, N, K, expected (tile rows, splits))
LINEAR_CASES = [
    # 32 x 64 tile, no split
    ("tile32_fwd", "fwd", 5, 256, 64, (32, 1)),
    ("tile32_dgrad", "dgrad", 40, 200, 96, (32, 1)),
    ("tile32_wgrad", "wgrad", 96, 200, 40, (32, 1)),
    # 64 x 64 tile, no split (with ragged M / N / K on the big tile)
    ("tile64_fwd", "fwd", 1000, 1100, 70, (64, 1)),
    ("tile64_dgrad", "dgrad", 1024, 160, 1030, (64, 1)),
    ("tile64_wgrad", "wgrad", 77, 1030, 1000, (64, 1)),
    # split-K on the 64 x 64 tile (accumulate=0: cleared first)
    ("tile64_split_fwd", "fwd", 512, 2048, 1024, (64, 4)),
    # the real shapes: CIFAR-10 batched embed Linear (batch 128; sampler batch 512), sigma-embed Linear (64 -> 256)
    ("cifar_embed_fwd", "fwd", 128, SUM_C_CIFAR, 256, (32, 1)),
    ("cifar_embed_dgrad", "dgrad", 128, SUM_C_CIFAR, 256, (32, 21)),
    ("cifar_embed_wgrad", "wgrad", 128, SUM_C_CIFAR, 256, (64, 1)),
    ("cifar_sampler_fwd", "fwd", 512, SUM_C_CIFAR, 256, (64, 1)),
    ("cifar_sigma_fwd", "fwd", 128, 256, 64, (32, 1)),
    ("cifar_sigma_wgrad", "wgrad", 128, 256, 64, (32, 1)),
    ("sigma_wgrad_b1024", "wgrad", 1024, 256, 64, (32, 4)),          # split-K, accumulate=0: the memset form
    # split-K whose K is no multiple of 32; 32 shares of which the last three are empty
    ("split_k1025_dgrad", "dgrad", 64, 1025, 128, (32, 4)),
    ("split_k3001_dgrad", "dgrad", 33, 3001, 65, (32, 11)),
    ("split_empty_dgrad", "dgrad", 32, 8200, 64, (32, 32)),
    ("split_empty_wgrad", "wgrad", 8200, 64, 32, (32, 32)),
]


@pytest.mark.parametrize("name,op,M,N,K,expect", LINEAR_CASES, ids=[c[0] for c in LINEAR_CASES])
def test_linear_gemm_branches(ops, name, op, M, N, K, expect):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    run_linear(ops, name, op, M, N, K, g, expect=expect)
    if name.startswith("split_empty"):
        gm, gn, gk = ops._LINEAR_GEMM[op](M, N, K)
        assert _kshares(gk, expect[1])[-1][0] >= gk          # the case really has empty shares
    if name.startswith("split_k"):
        gk = ops._LINEAR_GEMM[op](M, N, K)[2]
        (lo0, hi0), (lo, hi) = _kshares(gk, expect[1])[0], _kshares(gk, expect[1])[-1]
        assert gk % 32 and 0 < hi - lo < hi0 - lo0            # a short last share that ends inside a 32-chunk


def test_linear_gemm_imagenet_shapes(ops):
    """the ImageNet config's embed Linears: sum C = 17 472 columns from its block list, E = 768, batch 176 (and 512 for a
    sampler evaluation); sigma-embed 192 -> 768"""
    S = _sum_c_imagenet()
    g = torch.Generator().manual_seed(17472)
    for name, op, M, N, K, expect in [("imnet_embed_fwd", "fwd", 176, S, 768, (64, 1)),
                                      ("imnet_embed_dgrad", "dgrad", 176, S, 768, (32, 15)),
                                      ("imnet_embed_wgrad", "wgrad", 176, S, 768, (64, 1)),
                                      ("imnet_sampler_fwd", "fwd", 512, S, 768, (64, 1)),
                                      ("imnet_sigma_fwd", "fwd", 176, 768, 192, (32, 1)),
                                      ("imnet_sigma_wgrad", "wgrad", 176, 768, 192, (32, 1))]:
        run_linear(ops, name, op, M, N, K, g, expect=expect)


def test_linear_gemm_ragged_edges(ops):
    """M in {1, 33, 65}, N in {1, 63, 65}, K in {1, 31, 33} for each of the three ops (32 x 64 tile, partial tiles and a
    partial 32-chunk everywhere)"""
    g = torch.Generator().manual_seed(3133)
    for op in ("fwd", "dgrad", "wgrad"):
        for M in (1, 33, 65):
            for N in (1, 63, 65):
                for K in (1, 31, 33):
                    run_linear(ops, f"ragged_{op}", op, M, N, K, g, expect=(32, 1))


@pytest.mark.parametrize("op,M,N,K", [("dgrad", 40, 200, 96), ("dgrad", 128, SUM_C_CIFAR, 256), ("dgrad", 32, 8200, 64),
                                      ("wgrad", 96, 200, 40), ("wgrad", 1024, 256, 64), ("wgrad", 8200, 64, 32),
                                      ("wgrad", 128, SUM_C_CIFAR, 256)])
def test_linear_accumulate_contract(ops, op, M, N, K):
    """accumulate=1 adds onto what C holds (C0 + A.B) on the split and the unsplit form; accumulate=0 overwrites C (NaN
    first: the split form must clear it before its atomics)"""
    g = torch.Generator().manual_seed(M + N + K + 5)
    cshape = {"dgrad": (M, K), "wgrad": (N, K)}[op]
    splits = ops.linear_plan(op, M, N, K, 1)[1]
    tag = f"{op}_{'split' if splits > 1 else 'nosplit'}"
    c0 = randn(g, *cshape, scale=3.0)
    run_linear(ops, f"accumulate_{tag}", op, M, N, K, g, c0=c0, accumulate=1)
    run_linear(ops, f"overwrite_{tag}", op, M, N, K, g, c0=torch.full(cshape, float("nan"), device=DEV), accumulate=0)


# ------------------------------------------------------------------------------------------------ embedding
def _fourier_params(g, Fd):
    return (2 * math.pi * torch.randn(Fd, generator=g)).float(), (2 * math.pi * torch.rand(Fd, generator=g)).float()


def _fourier_check(ops, name, sigma, freqs, phases, B):
    out = ops.fourier_fwd(sigma.to(DEV), freqs.to(DEV), phases.to(DEV), B).cpu()
    s64 = sigma.double().expand(B) if sigma.numel() == 1 else sigma.double()
    c = (s64.log() / 4).view(-1, 1)
    f, p = freqs.double().view(1, -1), phases.double().view(1, -1)
    ref = torch.cos(c * f + p) * math.sqrt(2.0)
    # error of the argument (log, scale, product, sum) and of cos, times sqrt(2); factor-2 margin
    bound = 2 * math.sqrt(2.0) * (3 * U * ((c * f).abs() + p.abs()) + 4 * U)
    check_bound(name, out, ref, bound)


def test_fourier_sigma_range_and_broadcast(ops):
    """edm_fourier_fwd over sigma in [0.002, 80] (the samplers) and ln sigma in -1.2 +- 6 * 1.2 (training tails), per
    sample (sigma_stride 1) and one scalar sigma for the batch (sigma_stride 0, B > 1)"""
    g = torch.Generator().manual_seed(138)
    for Fd in (64, 192):
        freqs, phases = _fourier_params(g, Fd)
        samp = torch.exp(torch.linspace(math.log(0.002), math.log(80.0), 509, dtype=torch.float64)).float()
        samp = torch.cat([samp, torch.tensor([0.002, 80.0, 1.0])])
        tails = torch.exp(-1.2 + 1.2 * torch.linspace(-6, 6, 257, dtype=torch.float64)).float()
        _fourier_check(ops, f"fourier_sampler_F{Fd}", samp, freqs, phases, samp.numel())
        _fourier_check(ops, f"fourier_tails_F{Fd}", tails, freqs, phases, tails.numel())
        for s in (0.002, 0.37, 80.0, math.exp(-8.4), math.exp(6.0)):
            _fourier_check(ops, f"fourier_scalar_F{Fd}", torch.tensor([s], dtype=torch.float32), freqs, phases, 37)


@pytest.mark.parametrize("K,B,t", [(10, 1, 0.5), (10, 512, 0.5), (10, 512, 0.3), (1000, 1, 0.3), (1000, 512, 0.5),
                                   (1000, 512, 0.3)])
def test_embed_combine(ops, K, B, t):
    """edm_embed_combine_fwd / _bwd against the fp64 autograd of the tail of oracle.embedding_forward (class Linear of the
    one-hot label times sqrt(K), mp_add, mp_silu) with emb_sigma and the effective class weight as the leaves; labels with
    a few classes repeated heavily (about 50 atomics on each of their gwcls addresses at B = 512)"""
    E = 256 if K == 10 else 768
    g = torch.Generator().manual_seed(K + B + int(10 * t))
    es = torch.randn(B, E, generator=g)
    wch = O.effective_weight(torch.randn(E, K, generator=g))
    hot = torch.randint(0, K, (5,), generator=g)
    labels = torch.where(torch.rand(B, generator=g) < 0.6, hot[torch.randint(0, 5, (B,), generator=g)],
                         torch.randint(0, K, (B,), generator=g))
    gout = torch.randn(B, E, generator=g)
    # fp64 oracle (networks.py:169-177 as in oracle.embedding_forward)
    es64 = es.double().requires_grad_(True)
    w64 = wch.double().requires_grad_(True)
    onehot = torch.nn.functional.one_hot(labels, K).double() * math.sqrt(K)
    pre64 = O.mp_add(es64, onehot @ w64.t(), t)
    out64 = O.mp_silu(pre64)
    out64.backward(gout.double())
    pre, out = ops.embed_combine_fwd(es.to(DEV), wch.to(DEV), labels.to(DEV), t)
    c = 1.0 / math.sqrt((1 - t) ** 2 + t ** 2)
    cls = (onehot @ w64.detach().t()).abs()
    mag = ((1 - t) * es.double().abs() + t * cls) * c                     # |terms| of the pre-activation
    e_pre = 6 * U * mag                                                    # six roundings at most
    check_bound(f"embed_pre_K{K}_B{B}", pre.cpu(), pre64.detach(), 2 * e_pre)
    p = pre64.detach()
    # mp_silu on the device: x * sigmoid(x) with a hardware exp (relative error ~ (|x| + 2) u) and two more roundings;
    # the error of pre carried through |mp_silu'| <= 1.85
    silu_b = 2 * (1.85 * e_pre + U * (p.abs() + 4) * (p * torch.sigmoid(p)).abs() / 0.596)
    check_bound(f"embed_out_K{K}_B{B}", out.cpu(), out64.detach(), silu_b)
    ges, gw = ops.embed_combine_bwd(gout.to(DEV), pre, labels.to(DEV), t, (E, K))
    # |error| of gout * mp_silu'(pre): the derivative s (1 + x (1 - s)) / 0.596 with a hardware exp, and the error of pre
    # carried through |mp_silu''| <= 0.85
    dsil = (U * (p.abs() + 4) ** 2 / 0.596 + 0.85 * e_pre) * gout.double().abs()
    check_bound(f"embed_ges_K{K}_B{B}", ges.cpu(), es64.grad, 2 * ((1 - t) * c * dsil + 3 * U * es64.grad.abs()), l2=1e-5)
    # gwcls[e, k] = sum over the n_k samples of label k, added by atomics
    n_k = torch.bincount(labels, minlength=K).double()
    term = (t * c * math.sqrt(K)) * (gout.double() * (torch.sigmoid(p) * (1 + p * (1 - torch.sigmoid(p))) / 0.596)).abs()
    per = 2 * (t * c * math.sqrt(K) * dsil + 3 * U * term) + 2 * (n_k[labels].view(-1, 1) + 2) * U * term
    bound = torch.zeros(E, K, dtype=torch.float64).index_add_(1, labels, per.t())
    check_bound(f"embed_gwcls_K{K}_B{B}", gw.cpu(), w64.grad, bound, l2=1e-5)


# ------------------------------------------------------------------------------------------------ modulation finish
def _modfin_table(gains, ggains, layout):
    """the 24-byte ModFinItem records networks._modfin_table builds: {gain ptr, ggain ptr, col0, C}"""
    rec = np.zeros(len(layout), dtype=np.dtype([("gain", "<u8"), ("ggain", "<u8"), ("col0", "<i4"), ("C", "<i4")]))
    assert rec.dtype.itemsize == 24
    for k, (col0, C) in enumerate(layout):
        rec[k] = (gains.data_ptr() + 4 * k, ggains.data_ptr() + 4 * k, col0, C)
    return torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)


NAN_SENTINEL = 0x7FC0DEAD


def _nan_sentinel(shape):
    return torch.full(shape, NAN_SENTINEL, dtype=torch.int32).view(torch.float32)


@pytest.mark.parametrize("B", [1, 5, 128, 512])
def test_mod_finish_multi(ops, B):
    """edm_mod_finish_multi over 21 items (the CIFAR-10 block count) with C in {8, 72, 256, 768}, a non-zero first column
    and gap columns between items: glin[:, col0:col0+C] += gm * gain on top of non-zero values, ggain += sum gm * lin per
    item; two items with all-zero gm (blocks that took the unfused path) must keep their glin and ggain exactly; gap
    columns (NaN in all three buffers) are neither read nor written.  The single-block edm_mod_finish (strided lin /
    glin) on the same data."""
    from tinyedm_amd import _lib
    g = torch.Generator().manual_seed(B + 21)
    Cs = ([8, 72, 256, 768] * 6)[:21]
    layout, col = [], 3
    for k, C in enumerate(Cs):
        layout.append((col, C))
        col += C + (k % 3) * 5            # gaps of 0, 5 or 10 columns
    stride = col + 7
    gap = torch.ones(stride, dtype=torch.bool)
    for col0, C in layout:
        gap[col0:col0 + C] = False
    gm = torch.randn(B, stride, generator=g) + 0.5       # biased: the ggain sums do not cancel
    lin = torch.randn(B, stride, generator=g) + 0.5
    zero_items = (4, 13)
    for k in zero_items:
        col0, C = layout[k]
        gm[:, col0:col0 + C] = 0.0
    glin0 = 2.0 * torch.randn(B, stride, generator=g)
    for t_ in (gm, lin):
        t_[:, gap] = float("nan")
    glin0[:, gap] = _nan_sentinel((B, int(gap.sum())))
    gains = torch.randn(21, generator=g)
    ggain0 = torch.randn(21, generator=g)
    gm_d, lin_d, glin_d = gm.to(DEV), lin.to(DEV), glin0.to(DEV)
    gains_d, ggains_d = gains.to(DEV), ggain0.to(DEV)
    table = _modfin_table(gains_d, ggains_d, layout)
    ops.mod_finish_multi(gm_d, lin_d, glin_d, table, 21)
    glin, ggain = glin_d.cpu(), ggains_d.cpu()
    assert torch.equal(glin[:, gap].view(torch.int32), glin0[:, gap].view(torch.int32)), "gap columns written"
    for k, (col0, C) in enumerate(layout):
        sl = slice(col0, col0 + C)
        g_k, m_k, l_k, c0_k = gains[k].double(), gm[:, sl].double(), lin[:, sl].double(), glin0[:, sl].double()
        if k in zero_items:
            assert torch.equal(glin[:, sl], glin0[:, sl]) and ggain[k] == ggain0[k], f"item {k}: unfused block changed"
            continue
        check_bound(f"modfin_multi_glin_B{B}", glin[:, sl], c0_k + m_k * g_k, 2 * (3 * U * (m_k * g_k).abs() + U * c0_k.abs()))
        terms = (m_k * l_k)
        n = B * C
        ref = ggain0[k].double() + terms.sum()
        bound = 2 * (n + 8 + 2) * U * terms.abs().sum() + U * abs(ggain0[k].item())
        check_bound(f"modfin_multi_ggain_B{B}", ggain[k:k + 1], ref.view(1), bound.view(1))
        # the worst case above grows with n; a dropped or doubled term of a long sum still shows against 1e-5
        assert abs(ggain[k].item() - ref.item()) <= 1e-5 * terms.abs().sum().item() + U * abs(ggain0[k].item()), k
    # single-block form: gm contiguous [B, C], lin rows of `stride`, glin rows of a different stride (written, not +=)
    for k in (0, 1, 2, 3, 20):
        col0, C = layout[k]
        sl = slice(col0, col0 + C)
        gm_k = gm[:, sl].contiguous().to(DEV)
        gstride = C + 13
        glin_k = _nan_sentinel((B, gstride)).to(DEV)
        gg = ggain0[k:k + 1].clone().to(DEV)
        _lib.call("edm_mod_finish", ops._p(gm_k), ctypes.c_void_p(lin_d.data_ptr() + 4 * col0), stride,
                  ctypes.c_void_p(gains_d.data_ptr() + 4 * k), ops._p(glin_k), gstride, ops._p(gg), B, C, ops._stream())
        out = glin_k.cpu()
        assert torch.equal(out[:, C:].view(torch.int32), _nan_sentinel((B, gstride - C)).view(torch.int32))
        m_k, l_k = gm[:, sl].double(), lin[:, sl].double()
        check_bound(f"modfin_single_glin_B{B}", out[:, :C], m_k * gains[k].double(), 2 * U * (m_k * gains[k].double()).abs())
        terms = m_k * l_k
        ref = ggain0[k].double() + terms.sum()
        bound = 2 * (B * C + 256 + 2) * U * terms.abs().sum() + U * abs(ggain0[k].item())    # <= 256 per-wave atomics
        check_bound(f"modfin_single_ggain_B{B}", gg.cpu(), ref.view(1), bound.view(1))
        assert abs(gg.item() - ref.item()) <= 1e-5 * terms.abs().sum().item() + U * abs(ggain0[k].item()), k


# ------------------------------------------------------------------------------------------------ ScaleLong gate weights
def _gate(ops, g, B, H, W, C, R):
    skip = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16).to(DEV)
    gcs = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16).to(DEV)
    w1h = (torch.randn(R, C + 1, generator=g) / math.sqrt(C + 1)).to(DEV)
    w2h = (torch.randn(C, R, generator=g) / math.sqrt(R)).to(DEV)
    mean, gate, z1 = ops.skip_gate_fwd(skip, w1h, w2h)
    _, ws = ops.skip_gate_bwd(gcs, 0, skip, mean, w1h, w2h, gate, z1, defer_wgrad=True)
    _, gw1_a, gw2_a = ops.skip_gate_bwd(gcs, 0, skip, mean, w1h, w2h, gate, z1, defer_wgrad=False)
    return dict(skip=skip, gcs=gcs, w1h=w1h, w2h=w2h, mean=mean, ws=ws, gw1_a=gw1_a, gw2_a=gw2_a, R=R, C=C, B=B)


def _gate_mlp64(mean, w1h, w2h):
    """oracle.scale_long_gate's MLP (networks.py:112-118) in fp64 on the given per-sample means, the effective weights
    w1h [R][C+1], w2h [C][R] as leaves"""
    m = torch.cat([mean, torch.ones_like(mean[:, :1])], 1)
    return torch.sigmoid(O.mp_silu(m @ w1h.t()) @ w2h.t())


GATE_GROUPS = {
    "one": [(128, 8, 8, 256, 16)],
    "cifar9": [(128, s, s, 256, 16) for s in (8, 8, 8, 16, 16, 16, 32, 32, 32)],
    "mixed32": [((5, 64, 128, 1, 3)[k % 5], (4, 2, 3)[k % 3], (4, 2, 5)[k % 3], (64, 192, 256, 768)[k % 4],
                 (4, 12, 16, 48, 24)[k % 5]) for k in range(32)],
    "chunked": [(1000, 2, 2, 256, 16), (3, 4, 4, 64, 4)],
}


@pytest.mark.parametrize("group", list(GATE_GROUPS))
def test_skip_gate_wgrad_multi(ops, group):
    """edm_skip_gate_wgrad_multi (every decoder gate's gw1h / gw2h in one launch) against (a) the per-tensor
    edm_skip_gate_bwd with its own weight-gradient launch: bit for bit, same body, same chunking; (b) fp64 sums of the
    same fp32 per-sample vectors (ws, mean): gW2 = sum_b dz2 h^T, gW1 = sum_b dz1 [mean; 1]^T; (c) the fp64 autograd
    of the gate MLP w.r.t. the two effective weights.  'chunked': B = 1000, R = 16 walks the batch in two LDS chunks."""
    g = torch.Generator().manual_seed(len(GATE_GROUPS[group]) * 11)
    gates = [_gate(ops, g, *shape) for shape in GATE_GROUPS[group]]
    got = ops.skip_gate_wgrad_multi([(gt["ws"], gt["mean"], gt["R"]) for gt in gates])
    for k, (gt, (gw1, gw2)) in enumerate(zip(gates, got)):
        B, C, R = gt["B"], gt["C"], gt["R"]
        for nm, a, b in (("gw1h", gw1, gt["gw1_a"]), ("gw2h", gw2, gt["gw2_a"])):
            if not torch.equal(a, b):
                d = (a - b).abs()
                pytest.fail(f"{group} gate {k} (B={B}, C={C}, R={R}): {nm} differs from the per-tensor launch in "
                            f"{int((d != 0).sum())} of {d.numel()} elements, max |diff| {d.max().item():.3e} "
                            f"(max |{nm}| {b.abs().max().item():.3e})")
        ws, mean = gt["ws"].double(), gt["mean"].double()
        dz2, dz1, h = ws[:, :C], ws[:, C:C + R], ws[:, C + R:]
        m1 = torch.cat([mean, torch.ones_like(mean[:, :1])], 1)
        check_bound(f"gate_gw2_{group}", gw2, dz2.t() @ h, 2 * (B + 2) * U * (dz2.abs().t() @ h.abs()), l2=1e-5)
        check_bound(f"gate_gw1_{group}", gw1, dz1.t() @ m1, 2 * (B + 2) * U * (dz1.abs().t() @ m1.abs()), l2=1e-5)
        # (c) autograd of the MLP; the upstream gradient d loss / d gate = sum_hw gcat * skip in fp64 on the bf16 values
        w1 = gt["w1h"].double().requires_grad_(True)
        w2 = gt["w2h"].double().requires_grad_(True)
        ggate = (gt["gcs"].double() * gt["skip"].double()).sum(dim=(1, 2))
        _gate_mlp64(mean, w1, w2).backward(ggate)
        r1, r2 = rel(gw1, w1.grad), rel(gw2, w2.grad)
        record(f"fp32_sidepath/gate_autograd_{group}", max(r1, r2), 1e-4)
        assert r1 <= 1e-4 and r2 <= 1e-4, (B, C, R, r1, r2)


@pytest.mark.parametrize("C,R", [(192, 24), (384, 24), (576, 36), (192, 48), (256, 16), (768, 48)])
def test_skip_gate_per_sample_mlp(ops, C, R):
    """the per-sample gate MLP inside edm_skip_gate_fwd / edm_skip_gate_bwd (one workgroup per sample) against fp64 on the
    kernels' own fp32 intermediates: z1 = W1 [mean; 1], gate = sigmoid(W2 mp_silu(z1)), h = mp_silu(z1),
    dz1 = (W2^T dz2) mp_silu'(z1), gmean = W1[:, :C]^T dz1; and the fp32 evaluation path's edm_f32_skip_gate against fp64.
    C = 192, 384, 576 run workgroups of 1008 threads (15 whole waves and one of 48 lanes) with more than 15 rows of W1, the
    case where the trailing partial wave used to compute rows of its own and race wave 0 for them.  Every form runs three
    times, bit for bit the same."""
    g = torch.Generator().manual_seed(C * 3 + R)
    B, H, W = 16, 4, 4
    skip = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16).to(DEV)
    gcs = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16).to(DEV)
    w1h = (torch.randn(R, C + 1, generator=g) / math.sqrt(C + 1)).to(DEV)
    w2h = (torch.randn(C, R, generator=g) / math.sqrt(R)).to(DEV)
    runs = []
    for _ in range(3):
        mean, gate, z1 = ops.skip_gate_fwd(skip, w1h, w2h)
        gmean, ws = ops.skip_gate_bwd(gcs, 0, skip, mean, w1h, w2h, gate, z1, defer_wgrad=True)
        runs.append((mean, gate, z1, gmean, ws, ops.f32_skip_gate(skip.float(), w1h, w2h)))
    names = ("mean", "gate", "z1", "gmean", "ws", "f32 gate")
    for r in runs[1:]:
        for nm, a, b in zip(names, r, runs[0]):
            assert torch.equal(a, b), f"C={C}, R={R}: {nm} differs between two identical calls"
    mean, gate, z1, gmean, ws, gate32 = (t.double() for t in runs[0])
    W1, W2 = w1h.double(), w2h.double()
    m1 = torch.cat([mean, torch.ones_like(mean[:, :1])], 1)
    check_bound(f"gate_z1_C{C}", z1, m1 @ W1.t(), 2 * (C + 1 + 8) * U * (m1.abs() @ W1.abs().t()), l2=1e-5)
    # gate from the kernel's z1: h = mp_silu(z1) with a hardware exp (relative error (|z1| + 4) u), a dot of R terms, sigmoid
    h = O.mp_silu(z1)
    x = h @ W2.t()
    sg = torch.sigmoid(x)
    dot_err = W2.abs() @ ((z1.abs() + 4) * U * h.abs()).t() + 2 * (R + 2) * U * (W2.abs() @ h.abs().t())
    gate_b = 2 * (sg * (1 - sg) * dot_err.t() + ((x.abs() + 3) * (1 - sg) + 2) * U * sg)
    check_bound(f"gate_gate_C{C}", gate, sg, gate_b, l2=1e-5)
    dz2, dz1, hw = ws[:, :C], ws[:, C:C + R], ws[:, C + R:]
    check_bound(f"gate_h_C{C}", hw, h, 2 * (z1.abs() + 4) * U * h.abs())
    s = dz2 @ W2
    sz = torch.sigmoid(z1)
    d = sz * (1 + z1 * (1 - sz)) / 0.596                                   # mp_silu'(z1)
    s_err = 2 * (C + 8) * U * (dz2.abs() @ W2.abs())
    dz1_b = 2 * (s_err * d.abs() + s.abs() * (z1.abs() + 4) ** 2 * U / 0.596 + U * (s * d).abs())
    check_bound(f"gate_dz1_C{C}", dz1, s * d, dz1_b, l2=1e-5)
    check_bound(f"gate_gmean_C{C}", gmean, dz1 @ W1[:, :C], 2 * (R + 2) * U * (dz1.abs() @ W1[:, :C].abs()), l2=1e-5)
    # fp32 evaluation path: the whole gate from the fp32 skip (the same bf16 values) in fp64
    mean64 = skip.double().mean(dim=(1, 2))
    ref32 = _gate_mlp64(mean64, W1, W2)
    r32 = rel(gate32, ref32)
    record(f"fp32_sidepath/gate_f32_C{C}", r32, 2e-6)
    assert r32 <= 2e-6, f"C={C}, R={R}: edm_f32_skip_gate rel L2 {r32:.3e}"


# ------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("shape", [(128, 3, 32, 32), (64, 4, 64, 64), (1, 1, 28, 28), (37, 3, 17, 19)])
@pytest.mark.parametrize("weighted", [False, True])
def test_weighted_mse(ops, shape, weighted):
    """edm_weighted_mse past one wave of its 256-workgroup grid: loss = sum_b mean_j w_b d^2 / B and dD = 2 w d / (CHW B)
    against fp64 (relative 1e-5 / 1e-6), with the EDM weight from sigma or a per-sample override; the metric state:
    acc_sum += sum_b mean_j w_b d^2, acc_total += B, over two calls on non-zero starting values"""
    g = torch.Generator().manual_seed(sum(shape) + weighted)
    B = shape[0]
    D, clean = torch.randn(*shape, generator=g), 0.5 * torch.randn(*shape, generator=g)
    sigma = torch.exp(-1.2 + 1.2 * torch.randn(B, generator=g))
    weight = torch.rand(B, generator=g) * 3 + 0.1 if weighted else None
    w64 = weight.double() if weighted else O.loss_weight(sigma.double(), 0.5)
    d = (D.double() - clean.double()).reshape(B, -1)
    per = (w64.view(B, 1) * d * d).mean(dim=1)
    loss_ref = per.sum() / B
    dD_ref = (2 * w64.view(B, 1) * d / d.numel()).reshape(shape)
    acc_sum = torch.tensor([0.75], device=DEV)
    acc_total = torch.tensor([7], dtype=torch.int64, device=DEV)
    for call in range(2):
        loss, dD = ops.weighted_mse(D.to(DEV), clean.to(DEV), None if weighted else sigma.to(DEV), 0.5,
                                    weight=None if weight is None else weight.to(DEV), acc_sum=acc_sum, acc_total=acc_total)
        assert abs(loss.item() - loss_ref.item()) <= 1e-5 * loss_ref.item(), (loss.item(), loss_ref.item())
        err = (dD.cpu().double() - dD_ref).abs()
        ratio = (err / (1e-6 * dD_ref.abs()).clamp_min(1e-300)).max().item()
        record(f"fp32_sidepath/loss_dD_{'w' if weighted else 'sigma'}", ratio, 1.0)
        assert ratio <= 1.0, f"dD elementwise relative error {ratio * 1e-6:.3e}"
        assert acc_total.item() == 7 + (call + 1) * B, f"acc_total {acc_total.item()} after {call + 1} calls of B = {B}"
        acc_ref = 0.75 + (call + 1) * per.sum().item()
        assert abs(acc_sum.item() - acc_ref) <= 1e-5 * acc_ref, (acc_sum.item(), acc_ref)
