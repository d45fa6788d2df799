"""Label dropout (Embedding(label_dropout=p)) and classifier-free guidance from a single network (guide="unconditional")
on the GPU:

 * the combine kernels (linear.hip) with a given mask: a dropped row is the labels=None row, a kept row the mask-free
   row, bit for bit, in pre, out and d emb_sigma; the class-weight gradient against the fp64 autograd of the per-row
   composition, within the bounds of tests/test_fp32_sidepath_gpu.py::test_embed_combine;
 * the drawn mask against a numpy restatement of philox4x32_10((b, 0x4C41424C, 0, step), (seed_lo, seed_hi)).x < thr,
   with (seed, step) as arguments and from a device step record; p = 0 is the plain call;
 * the module: p = 0 and eval() change nothing; one training step against the oracle composing the label-free and the
   conditional embedding per sample (limits of tests/test_gradparity_gpu.py); eight captured steps against eight eager
   ones (comparison of tests/test_graph_gpu.py::test_captured_step_matches_eager_step);
 * self-guided solves of all three solvers: bit-identical to a lambda guide evaluating the model without labels, eager
   and replayed, against the oracle (guided limits of tests/test_guided_solver_gpu.py); a new weight replays the cached
   graph; the cache does not keep the model alive;
 * the generate CLI with --guide_unconditional."""
import gc
import math
import os
import subprocess
import sys
import weakref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs
from parity_log import record

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
TAG = 0x4C41424C


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------ the mask stream, restated
M32 = np.uint64(0xFFFFFFFF)


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = c[0] * np.uint64(0xD2511F53)
        p1 = c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def _mask_ref(B, seed, step, p):
    """sample b is dropped iff philox((b, 0x4C41424C, 0, step), (seed_lo, seed_hi)).x < round(p * 2^32)"""
    b = np.arange(B, dtype=np.uint64)
    z = np.zeros(B, dtype=np.uint64)
    r = _philox4x32_10(b, z + TAG, z, z + step, seed & 0xFFFFFFFF, seed >> 32)
    thr = min(max(int(round(p * 2.0 ** 32)), 0), 1 << 32)
    return (r[0] < np.uint64(thr)).astype(np.int32) if thr < 1 << 32 else np.ones(B, dtype=np.int32)


def _step_record(seed, step):
    """a device edm_step_params record holding only (step, seed)"""
    rec = torch.zeros(12, dtype=torch.int32)
    u = rec.numpy().view(np.uint32)
    u[0], u[1], u[2] = step & 0xFFFFFFFF, seed & 0xFFFFFFFF, seed >> 32
    return rec.to(DEV)


# ------------------------------------------------------------------ kernels, given mask
def _check_bound(name, got, ref, bound, l2=None):
    got, ref, bound = got.double(), ref.double(), bound.double()
    assert torch.isfinite(got).all(), f"{name}: non-finite result"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = ratio.max().item() if ratio.numel() else 0.0
    record("label_dropout/" + name, worst, 1.0)
    assert worst <= 1.0, f"{name}: error / bound = {worst:.3g} (max err {err.max().item():.3e})"
    if l2 is not None:
        r = rel(got, ref)
        assert r <= l2, f"{name}: rel L2 {r:.3e} > {l2:.0e}"


@pytest.mark.parametrize("B,E,K", [(37, 64, 10), (37, 256, 1000), (130, 64, 1000), (130, 256, 10)])
@pytest.mark.parametrize("mode", ["none", "all", "mixed"])
def test_combine_given_mask(ops, B, E, K, mode):
    t = 0.5
    g = torch.Generator().manual_seed(B * E + K)
    es = torch.randn(B, E, generator=g).to(DEV)
    wch = O.effective_weight(torch.randn(E, K, generator=g))
    hot = torch.randint(0, K, (3,), generator=g)
    labels = torch.where(torch.rand(B, generator=g) < 0.6, hot[torch.randint(0, 3, (B,), generator=g)],
                         torch.randint(0, K, (B,), generator=g))
    gout = torch.randn(B, E, generator=g)
    drop = {"none": torch.zeros(B, dtype=torch.int32), "all": torch.ones(B, dtype=torch.int32),
            "mixed": (torch.rand(B, generator=g) < 0.4).to(torch.int32)}[mode]
    if mode == "mixed":
        assert 0 < int(drop.sum()) < B
    d = drop.bool().to(DEV).view(-1, 1)
    pre_n, out_n = ops.embed_combine_fwd(es, wch.to(DEV), labels.to(DEV), t)
    pre_u, out_u = ops.embed_combine_fwd(es, None, None, t)
    pre, out, mask = ops.embed_combine_fwd(es, wch.to(DEV), labels.to(DEV), t, drop=drop.to(DEV))
    assert torch.equal(mask.cpu(), drop)
    for got, n, u in ((pre, pre_n, pre_u), (out, out_n, out_u)):
        assert torch.equal(torch.where(d, got, 0.0), torch.where(d, u, 0.0))
        assert torch.equal(torch.where(d, 0.0, got), torch.where(d, 0.0, n))
    ges, gw = ops.embed_combine_bwd(gout.to(DEV), pre, labels.to(DEV), t, (E, K), drop=mask)
    ges_n, _ = ops.embed_combine_bwd(gout.to(DEV), pre_n, labels.to(DEV), t, (E, K))
    ges_u, _ = ops.embed_combine_bwd(gout.to(DEV), pre_u, None, t, None)
    assert torch.equal(torch.where(d, ges, 0.0), torch.where(d, ges_u, 0.0))
    assert torch.equal(torch.where(d, 0.0, ges), torch.where(d, 0.0, ges_n))
    # class-weight gradient: fp64 autograd of the per-row composition (mp_add for a kept row, none for a dropped one)
    es64 = es.cpu().double().requires_grad_(True)
    w64 = wch.double().requires_grad_(True)
    onehot = torch.nn.functional.one_hot(labels, K).double() * math.sqrt(K)
    kept = ~drop.bool().view(-1, 1)
    pre64 = torch.where(kept, O.mp_add(es64, onehot @ w64.t(), t), es64)
    O.mp_silu(pre64).backward(gout.double())
    if mode == "all":
        assert float(gw.abs().max()) == 0.0
        return
    # the bound of test_embed_combine over the kept samples only
    c = 1.0 / math.sqrt((1 - t) ** 2 + t ** 2)
    cls = (onehot @ w64.detach().t()).abs()
    e_pre = 6 * U * ((1 - t) * es.cpu().double().abs() + t * cls) * c
    p = pre64.detach()
    dsil = (U * (p.abs() + 4) ** 2 / 0.596 + 0.85 * e_pre) * gout.double().abs()
    kl = labels[kept.view(-1)]
    n_k = torch.bincount(kl, minlength=K).double()
    term = (t * c * math.sqrt(K)) * (gout.double() * (torch.sigmoid(p) * (1 + p * (1 - torch.sigmoid(p))) / 0.596)).abs()
    per = 2 * (t * c * math.sqrt(K) * dsil + 3 * U * term) + 2 * (n_k[labels].view(-1, 1) + 2) * U * term
    per = per * kept
    bound = torch.zeros(E, K, dtype=torch.float64).index_add_(1, labels, per.t())
    _check_bound(f"gwcls_{mode}_B{B}_E{E}_K{K}", gw.cpu(), w64.grad, bound, l2=1e-5)


# ------------------------------------------------------------------ kernels, drawn mask
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 1.0])
def test_drawn_mask_vs_restatement(ops, p):
    g = torch.Generator().manual_seed(1)
    for seed, step, B in ((0, 0, 7), (1234, 5, 130), (0x9E3779B97F4A7C15, 0xFFFFFFFF, 513), (42, 77, 2048)):
        es = torch.randn(B, 64, generator=g).to(DEV)
        wch = O.effective_weight(torch.randn(64, 10, generator=g)).to(DEV)
        labels = torch.randint(0, 10, (B,), generator=g).to(DEV)
        ref = _mask_ref(B, seed, step, p)
        if p == 0.0:
            pre0, out0 = ops.embed_combine_fwd(es, wch, labels, 0.5)
            r = ops.embed_combine_fwd(es, wch, labels, 0.5, drop_p=0.0, seed=seed, step=step)
            assert len(r) == 2 and torch.equal(r[0], pre0) and torch.equal(r[1], out0)
            assert not ref.any()
            continue
        pre, out, mask = ops.embed_combine_fwd(es, wch, labels, 0.5, drop_p=p, seed=seed, step=step)
        assert mask.dtype == torch.int32 and np.array_equal(mask.cpu().numpy(), ref)
        _, _, mask_dyn = ops.embed_combine_fwd(es, wch, labels, 0.5, drop_p=p, seed=seed ^ 1, step=step + 1,
                                               dyn=_step_record(seed, step))
        assert torch.equal(mask_dyn, mask)                        # the record overrides the by-value (seed, step)
        pre_g, out_g, _ = ops.embed_combine_fwd(es, wch, labels, 0.5, drop=mask)
        assert torch.equal(pre_g, pre) and torch.equal(out_g, out)
    if 0.0 < p < 1.0:
        big = _mask_ref(1 << 16, 7, 3, p)
        assert abs(big.mean() - p) < 5 * math.sqrt(p * (1 - p) / big.size)
        assert not np.array_equal(_mask_ref(256, 7, 3, p), _mask_ref(256, 7, 4, p))
        assert not np.array_equal(_mask_ref(256, 7, 3, p), _mask_ref(256, 8, 3, p))


# ------------------------------------------------------------------ the module
def _nets(P, ecfg, dcfg, **emb_kw):
    import tinyedm_amd as T
    from tinyedm_amd import networks as N
    N._rng_sub_counter[0] = 0
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor, **emb_kw)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), dcfg.dropout_rate,
                     dcfg.sigma_data, dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    emb.load_state_dict({k[len("embedding."):]: v for k, v in P.items() if k.startswith("embedding.")}, strict=True)
    den.load_state_dict({k[len("denoiser."):]: v for k, v in P.items() if k.startswith("denoiser.")}, strict=True)
    return emb.to(DEV), den.to(DEV)


def _batch(B, seed, H=16):
    g = torch.Generator().manual_seed(seed)
    clean = 0.5 * torch.randn(B, 3, H, H, generator=g)
    eps, noise = torch.randn(B, generator=g), torch.randn(B, 3, H, H, generator=g)
    labels = torch.randint(0, 10, (B,), generator=g)
    return clean, eps, noise, labels


def _fwd_bwd(emb, den, batch, seed):
    """one training-mode forward + backward with the oracle's noise draws -> (D, loss, {name: grad})"""
    import tinyedm_amd as T
    from tinyedm_amd import metric
    clean, eps, noise, labels = batch
    noisy, sigma = O.diffuse(clean, eps, noise, -1.2, 1.2)
    T.manual_seed(seed)
    _, e = emb(sigma.to(DEV), labels.to(DEV))
    D = den(noisy.to(DEV), sigma.to(DEV), e)
    w = (sigma ** 2 + 0.25) / (sigma * 0.5) ** 2
    loss = metric.weighted_mse_loss(w.to(DEV), D, clean.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    grads = {("embedding." + k): v.grad for k, v in emb.named_parameters()}
    grads.update({("denoiser." + k): v.grad for k, v in den.named_parameters()})
    return D.detach(), loss.detach(), grads


def test_module_zero_and_eval_change_nothing(ops):
    ecfg, dcfg = tiny_cfgs(10)
    P = O.init_params(ecfg, dcfg, torch.Generator().manual_seed(21), gains_nonzero=True)
    batch = _batch(6, 8)
    from tinyedm_amd import _lib
    D0, l0, g0 = _fwd_bwd(*[m.train() for m in _nets(P, ecfg, dcfg)], batch, 99)
    calls, real = [], _lib.call

    def spy(name, *args):
        if name.startswith("edm_embed_combine"):
            calls.append((name, args))
        return real(name, *args)
    _lib.call = spy
    try:
        D1, l1, g1 = _fwd_bwd(*[m.train() for m in _nets(P, ecfg, dcfg, label_dropout=0.0)], batch, 99)
    finally:
        _lib.call = real
    # the plain combine: threshold 0, no mask in or out, in the forward and the backward
    assert [c[0] for c in calls] == ["edm_embed_combine_fwd", "edm_embed_combine_bwd"]
    fwd, bwd = calls[0][1], calls[1][1]
    assert fwd[9] == 0 and fwd[12] is None and fwd[13] is None and fwd[14] is None and bwd[9] is None
    assert torch.equal(D0, D1)
    assert g0.keys() == g1.keys()
    # the loss and the gradients summed with float atomics (the class weight's, the modulation and split-K weight
    # gradients) differ in the last bits from run to run whatever the arguments: held to the rounding of a reordered
    # fp32 sum (scalar gains against the scale of the scalar gradients, as in tests/test_gradparity_gpu.py)
    g0, g1 = {"loss": l0, **g0}, {"loss": l1, **g1}
    scal_rms = float(np.sqrt(np.mean([float(v) ** 2 for k, v in g0.items() if v.numel() == 1 and k != "loss"])))
    for k in g0:
        assert g0[k] is not None and g1[k] is not None, k
        if k != "loss" and g0[k].numel() == 1:
            e = abs(float(g1[k]) - float(g0[k])) / max(abs(float(g0[k])), scal_rms)
        else:
            e = rel(g1[k], g0[k])
        record(f"label_dropout/p0_vs_no_argument[{k}]", e, 1e-5)
        assert e <= 1e-5, (k, e)
    # eval(): never drops (labels or not), the forward of p = 0
    clean, eps, noise, labels = batch
    noisy, sigma = O.diffuse(clean, eps, noise, -1.2, 1.2)
    outs = []
    for p in (0.0, 0.5):
        emb, den = _nets(P, ecfg, dcfg, label_dropout=p)
        emb.eval(), den.eval()
        with torch.no_grad():
            _, e = emb(sigma.to(DEV), labels.to(DEV))
            outs.append((e, den(noisy.to(DEV), sigma.to(DEV), e)))
        assert emb.last_label_drop is None
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_training_step_vs_oracle(ops):
    """one step of the tiny conditional net at label_dropout 0.3: the loss and every gradient against the oracle with
    each sample's embedding composed from oracle.embedding_forward with or without its label per the restated mask"""
    from tinyedm_amd import networks as N
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ecfg, dcfg = tiny_cfgs(10)
    P = O.init_params(ecfg, dcfg, torch.Generator().manual_seed(21), gains_nonzero=True)
    emb, den = _nets(P, ecfg, dcfg, label_dropout=0.3)
    emb.train(), den.train()
    B, seed = 8, 1234
    batch = _batch(B, 77)
    _, loss, grads = _fwd_bwd(emb, den, batch, seed)
    mask = _mask_ref(B, seed, 0, 0.3)
    assert np.array_equal(emb.last_label_drop.cpu().numpy(), mask)
    assert 0 < mask.sum() < B, mask          # (seed 1234, step 0: samples 3, 4, 7 dropped)
    assert N.rng.step == 1
    clean, eps, noise, labels = batch
    for leg, bf16 in (("bf16_oracle", True), ("fp32_autograd", False)):
        Pb = {k: v.clone() for k, v in P.items()}
        O.force_normalize_(Pb)
        keys = O.trainable_keys(Pb)
        for k in keys:
            Pb[k].requires_grad_(True)
        noisy, sigma = O.diffuse(clean, eps, noise, -1.2, 1.2)
        rows = [O.embedding_forward(Pb, ecfg, sigma[b:b + 1], None if mask[b] else labels[b:b + 1])[1] for b in range(B)]
        Dor = O.denoiser_forward(Pb, dcfg, noisy, sigma, torch.cat(rows), True, bf16, None)
        lo = O.weighted_mse(O.loss_weight(sigma, dcfg.sigma_data), Dor, clean)
        lo.backward()
        assert sorted(keys) == sorted(grads)
        lrel = abs(loss.item() - lo.item()) / abs(lo.item())
        record(f"label_dropout/step_loss_vs_{leg}", lrel, 2e-2)
        assert lrel <= 2e-2, (loss.item(), lo.item())
        scal = [Pb[k].grad.abs().item() for k in keys if Pb[k].numel() == 1]
        scal_rms = float(np.sqrt(np.mean(np.square(scal))))
        per = {}
        for k in keys:
            gr, go = grads[k], Pb[k].grad
            assert gr is not None and torch.isfinite(gr).all(), k
            per[k] = (abs(gr.item() - go.item()) / max(abs(go.item()), scal_rms)) if gr.numel() == 1 else rel(gr, go)
        worst = max(per, key=per.get)
        lim = 3e-2 if bf16 else 6e-2
        record(f"label_dropout/step_worst_tensor_vs_{leg}[{worst}]", per[worst], lim)
        assert per[worst] <= lim, f"{leg}: {worst} rel {per[worst]:.3e}"
        if bf16:
            # the class weight's gradient comes from the kept samples only: the oracle without the mask is far off
            k = "embedding.class_embed.linear.weight"
            Pn = {kk: v.clone() for kk, v in P.items()}
            O.force_normalize_(Pn)
            Pn[k].requires_grad_(True)
            O.training_loss(Pn, ecfg, dcfg, clean, eps, noise, -1.2, 1.2, labels, bf16=True).backward()
            assert rel(grads[k], Pn[k].grad) > 5 * per[k]


def _build_edm(seed, label_dropout):
    """the model of tests/test_graph_gpu.py::_build (dropout 0.1, gain_out 0.7) with label dropout"""
    import tinyedm_amd as T
    from tinyedm_amd import networks as N
    ecfg, dcfg = tiny_cfgs()
    N._rng_sub_counter[0] = 0
    T.manual_seed(seed)
    torch.manual_seed(seed)
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor,
                      label_dropout=label_dropout)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), 0.1, dcfg.sigma_data,
                     dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    with torch.no_grad():
        den.gain_out.fill_(0.7)
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=True, use_uncertainty=False,
                  steady_steps=3, rampup_steps=3, scheduler_interval="step", lr=2e-3, ema_length=0.13)
    return model.to(DEV).train()


def _opt(model):
    import tinyedm_amd as T
    from tinyedm_amd.ema import EMAOptimizer
    cfg = model.configure_optimizers()
    base, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    return EMAOptimizer(base, device=DEV, gamma=T.sigma_rel_to_gamma(0.13)), base, sched


def test_captured_steps_match_eager_steps(ops):
    from tinyedm_amd import networks as N
    from tinyedm_amd.graph import CapturedTrainStep
    g = torch.Generator().manual_seed(5)
    B = 32
    batches = [((0.5 * torch.randn(B, 3, 16, 16, generator=g)).to(DEV), torch.randint(0, 10, (B,), generator=g).to(DEV))
               for _ in range(8)]
    # ---- eager
    model_e = _build_edm(11, 0.3)
    opt_e, base_e, sched_e = _opt(model_e)
    opt_e.zero_grad()
    losses_e, masks_e = [], []
    for b in batches:
        step0 = N.rng.step
        loss = model_e.training_step(b, 0)
        loss.backward()
        opt_e.step()
        opt_e.zero_grad()
        sched_e.step()
        losses_e.append(float(loss))
        masks_e.append(model_e.embedding.last_label_drop.cpu().numpy().copy())
        assert np.array_equal(masks_e[-1], _mask_ref(B, N.rng.seed, step0, 0.3))
    counters_e = (base_e.step_count, opt_e.current_step, N.rng.step)
    for a, b in zip(masks_e, masks_e[1:]):
        assert not np.array_equal(a, b)
    # ---- captured (the first visits run eagerly, the rest replays one graph)
    model_g = _build_edm(11, 0.3)
    opt_g, base_g, sched_g = _opt(model_g)
    opt_g.zero_grad()
    step = CapturedTrainStep(model_g, opt_g)
    losses_g, masks_g = [], []
    for b in batches:
        loss = step(b)
        sched_g.step()
        losses_g.append(float(loss))
        masks_g.append(model_g.embedding.last_label_drop.cpu().numpy().copy())
    assert len(step._graphs) == 1
    assert (base_g.step_count, opt_g.current_step, N.rng.step) == counters_e
    for a, b in zip(masks_g, masks_e):
        assert np.array_equal(a, b)                 # a replay draws the mask of its step from the device record
    worst = max(abs(a - b) / abs(b) for a, b in zip(losses_g, losses_e))
    record("label_dropout/captured_loss_vs_eager", worst, 2e-3)
    assert worst <= 2e-3, (losses_g, losses_e)
    for name, a, b, lim in (("theta", base_g.arena.theta, base_e.arena.theta, 2e-3), ("adam_m", base_g.m, base_e.m, 2e-2),
                            ("adam_v", base_g.v, base_e.v, 2e-2), ("ema", opt_g.ema_arena, opt_e.ema_arena, 2e-3)):
        e = rel(a, b)
        record(f"label_dropout/captured_{name}_vs_eager", e, lim)
        assert e <= lim, f"{name}: rel {e:.3e}"


# ------------------------------------------------------------------ self-guided solves
def _edm_eval(P, ecfg, dcfg, dtype):
    import tinyedm_amd as T
    emb, den = _nets(P, ecfg, dcfg, label_dropout=0.2)
    den.set_eval_dtype(dtype)
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                  steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01)
    return model.to(DEV).eval()


SCHED = dict(num_steps=5, sigma_min=0.01, sigma_max=20.0, rho=5.0)


def _solver(kind, **kw):
    import tinyedm_amd as T
    if kind == "heun":
        return T.DeterministicSolver(**SCHED, **kw)
    if kind == "churn":
        return T.StochasticSolver(**SCHED, S_churn=20.0, seed=3, **kw)
    return T.MultistepSolver(**SCHED, order=2, **kw)


def _solve(sol, model, x0, labels, graph=False):
    if hasattr(sol, "solve_index"):
        sol.solve_index = 0         # the same churn noise on every solve
    return sol.solve(model, x0, labels, graph=graph)


def _oracle_D(P, ecfg, dcfg, w, bf16):
    def D(x, s, labels):
        sig = s.reshape(-1).expand(x.shape[0])
        Dm = O.edm_forward(P, ecfg, dcfg, x, sig, labels, bf16=bf16).float()
        Dg = O.edm_forward(P, ecfg, dcfg, x, sig, None, bf16=bf16).float()
        return Dg + w * (Dm - Dg)
    return D


def _oracle_multistep(D, x0, t, coef, labels):
    x = x0.float() * t[0]
    hist = []
    for i, (a, c0, c1, c2) in enumerate(coef.tolist()):
        m = D(x, t[i], labels)
        nxt = a * x + c0 * m
        if c1 != 0.0:
            nxt = nxt + c1 * hist[-1]
        if c2 != 0.0:
            nxt = nxt + c2 * hist[-2]
        hist.append(m)
        x = nxt
    return x


@pytest.mark.parametrize("kind", ["heun", "churn", "dpmpp"])
def test_self_guided_solve_is_the_label_free_evaluation(ops, kind):
    ecfg, dcfg = tiny_cfgs(10)
    model = _edm_eval(O.init_params(ecfg, dcfg, torch.Generator().manual_seed(7)), ecfg, dcfg, "bf16")
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(3, 3, 8, 8, generator=g).to(DEV)
    labels = torch.randint(0, 10, (3,), generator=g).to(DEV)
    sol = _solver(kind, guide="unconditional", guidance=2.0)
    eager = _solve(sol, model, x0, labels)
    lam = _solve(_solver(kind, guide=lambda x, s, c: model(x, s, None), guidance=2.0), model, x0, labels)
    assert torch.equal(eager, lam)
    assert not torch.equal(eager, _solve(_solver(kind), model, x0, labels))
    assert torch.equal(_solve(sol, model, x0, labels, graph=True), eager)
    assert torch.equal(_solve(sol, model, x0, labels, graph=True), eager)          # pure replay
    assert len(sol._graphs[model]) == 1
    key = next(iter(sol._graphs[model]))
    assert ("unconditional",) in key                 # a constant tag, not the id of a wrapper
    ent = sol._graphs[model][key]
    assert ent.guide is None                        # the entry holds no guide
    # a new guidance weight replays the cached graph
    sol.guidance = 3.5
    eager = _solve(sol, model, x0, labels)
    assert torch.equal(_solve(sol, model, x0, labels, graph=True), eager)
    assert len(sol._graphs[model]) == 1
    # the cache does not keep the model alive
    ref = weakref.ref(model)
    del model, ent, key
    gc.collect()
    assert ref() is None
    assert len(sol._graphs) == 0


@pytest.mark.parametrize("case", ["heun_bf16", "heun_f32", "dpmpp_bf16", "dpmpp_f32"])
def test_self_guided_trajectory_vs_oracle(ops, case):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    kind, dtype = case.split("_")
    bf16 = dtype == "bf16"
    ecfg, dcfg = tiny_cfgs(10)
    P = O.init_params(ecfg, dcfg, torch.Generator().manual_seed(7))
    model = _edm_eval(P, ecfg, dcfg, dtype)
    sol = _solver(kind, guide="unconditional", guidance=2.0)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 3, 8, 8, generator=g)
    labels = torch.randint(0, 10, (2,), generator=g)
    x_hip = sol.solve(model, x0.to(DEV), labels.to(DEV)).cpu()
    D = _oracle_D(P, ecfg, dcfg, 2.0, bf16)
    with torch.no_grad():
        if kind == "heun":
            x_or = O.heun_solve(D, x0, O.karras_schedule(5, 0.01, 20.0, 5.0), labels)
        else:
            x_or = _oracle_multistep(D, x0, sol.t_steps, sol.multistep_coefficients(), labels)
    e = rel(x_hip, x_or)
    lim = 3e-2 if bf16 else 6e-4
    record(f"label_dropout/self_guided_{case}_trajectory_vs_oracle", e, lim)
    assert e <= lim, e
    # the guidance must matter at this size
    x_main = _solver(kind).solve(model, x0.to(DEV), labels.to(DEV)).cpu()
    assert rel(x_main, x_or) > 5 * e


def test_self_guide_checks_before_launch(ops):
    import tinyedm_amd as T
    ecfg, dcfg = tiny_cfgs(10)
    cond = _edm_eval(O.init_params(ecfg, dcfg, torch.Generator().manual_seed(7)), ecfg, dcfg, "bf16")
    eu, du = tiny_cfgs(None)
    Pu = O.init_params(eu, du, torch.Generator().manual_seed(11))
    emb, den = _nets(Pu, eu, du)
    uncond = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                   steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01).to(DEV).eval()
    x0 = torch.randn(2, 3, 8, 8, device=DEV)
    labels = torch.zeros(2, dtype=torch.int64, device=DEV)
    for kind in ("heun", "churn", "dpmpp"):
        sol = _solver(kind, guide="unconditional", guidance=2.0)
        with pytest.raises(ValueError, match="class-conditional"):
            sol.solve(uncond, x0, labels)
        with pytest.raises(ValueError, match="class-conditional"):
            sol.solve(lambda x, s, c: cond(x, s, c), x0, labels)
        with pytest.raises(ValueError, match="class_labels"):
            sol.solve(cond, x0, None)
        assert not sol._graphs


# ------------------------------------------------------------------ generate CLI
def test_generate_cli_guide_unconditional(ops, tmp_path):
    out = tmp_path / "cfg"
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "generate.py"), "--config_name", "cifar10_cond",
           "--output_dir", str(out), "--num_samples", "4", "--batch_size", "4", "--num_steps", "3", "--num_classes",
           "10", "--image_size", "32", "--num_workers", "0", "--guide_unconditional", "--guidance", "2"]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "label_dropout 0" in r.stdout             # the config's model never saw label-free samples: one warning
    assert sorted(os.listdir(out)) == [f"{i}.png" for i in range(4)]
    from PIL import Image
    for i in range(4):
        assert Image.open(out / f"{i}.png").size == (32, 32)
