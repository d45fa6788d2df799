"""Likelihood evaluation along the probability-flow ODE on the GPU: the probe / divergence kernels against the restated
Philox stream and fp64 sums, DeterministicSolver.log_likelihood against the closed form of a diagonal Gaussian and
against the CPU oracle's exact eps . J eps on the tiny networks, the hipGraph path and the generate CLI.

Limits marked MEASURED are 3x the worst value seen on an MI355X (the figure is in the comment next to each); every test
prints its figures before asserting and records them in parity_log."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import likelihood_ref as R
from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs
from parity_log import record

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x9E3779B97F4A7C15

# MEASURED limits: 3x the worst case seen on an MI355X over the tested nets and sigmas (two runs, figures below), at the
# default delta = 1e-2.  The 3x is for box-to-box spread of the f32x3 path.
Q_KERNEL_LIMIT = 5e-15          # |q - q64| / d of the div kernels on random operands: worst 6.0e-16 (fp64 differences and
#                                 sums in the kernel, so this is a few ulp of fp64; a small multiple of it)
ANALYTIC_LIMIT = 9.5e-6         # nats/dim, log_likelihood vs the fp64 recursion, diagonal Gaussian: worst 3.17e-6 (N = 64;
#                                 1.9e-6 at N = 16 and 32): the fp32 state and the rounding of the difference quotient
Q_NET_LIMIT = {"f32": 6.9e-6, "f32x3": 1.9e-5}      # |q - q_oracle| / d per evaluation: worst 2.29e-6 / 6.35e-6 (sigma 1.04)
LOGP_NET_LIMIT = {"f32": 2.25e-5, "f32x3": 5.1e-5}  # nats/dim, whole solve vs the oracle recursion: worst 7.49e-6 / 1.69e-5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def _rand(shape, seed, offset=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    buf = torch.zeros(n + offset, device=DEV)
    buf[offset:] = (scale * torch.randn(n, generator=g)).to(DEV)
    return buf[offset:].view(shape)


def _blocks(E, B, K):
    return E[:B], [E[(1 + 2 * p) * B:(2 + 2 * p) * B] for p in range(K)], [E[(2 + 2 * p) * B:(3 + 2 * p) * B] for p in range(K)]


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape,offset", [((7, 3, 32, 32), 0), ((5, 3, 7, 9), 0), ((7, 3, 32, 32), 1)],
                         ids=["cifar-vec", "odd-scalar", "misaligned-scalar"])
def test_probe_vs_restatement(ops, shape, offset):
    solve_index, step, ev, K, h = 3, 5, 1, 3, 0.0371
    B = shape[0]
    x = _rand(shape, 1, offset)
    assert (x.data_ptr() % 16 == 0) == (offset == 0)
    rec = ops.churn_record(SEED, solve_index, DEV)
    E = ops.nll_probe(x, h, rec, step, ev, K)
    ops.check_health(DEV, "nll_probe")
    assert E.shape == ((1 + 2 * K) * B,) + shape[1:]
    eps = R.probe_signs(shape, SEED, solve_index, step, ev, K).to(DEV)
    h32 = torch.tensor(h, dtype=torch.float32, device=DEV)
    x0, plus, minus = _blocks(E, B, K)
    assert torch.equal(x0, x)
    for p in range(K):          # x +- h is one fp32 add: bit-exact
        assert torch.equal(plus[p], x + h32 * eps[p]), p
        assert torch.equal(minus[p], x - h32 * eps[p]), p
    record(f"likelihood/probe_{'x'.join(map(str, shape))}_off{offset}_mismatches", 0.0, 0.0)
    # eps read back is +-1 exactly where h is not absorbed, and the probes of other evaluations / indices differ
    back = ((plus[0] - x) / h32).round()
    assert torch.equal(back, eps[0])
    other = _blocks(ops.nll_probe(x, h, rec, step, 0, K), B, K)[1]
    assert not torch.equal(other[0], plus[0]) and not torch.equal(plus[0], plus[1]) and not torch.equal(plus[1], plus[2])
    assert not torch.equal(_blocks(ops.nll_probe(x, h, rec, step + 1, ev, 1), B, 1)[1][0], plus[0])
    assert not torch.equal(_blocks(ops.nll_probe(x, h, ops.churn_record(SEED, solve_index + 1, DEV), step, ev, 1), B, 1)[1][0],
                           plus[0])
    # the stream is neither the churn's nor the blend's of the same (seed, solve index, step): their sign patterns differ
    churn = ops.heun_churn(x * 0, 1.0, rec, step)
    blend = ops.inpaint_blend(x * 0, x * 0, torch.ones(1, int(np.prod(shape[2:])), dtype=torch.uint8, device=DEV), 1.0,
                              rec, step)
    for n in (churn, blend):
        agree = ((n > 0) == (eps[0] > 0)).float().mean().item()
        assert 0.4 < agree < 0.6, agree
    if offset:          # the scalar path of a misaligned tensor draws what the dwordx4 path draws, bit for bit
        assert torch.equal(E, ops.nll_probe(_rand(shape, 1), h, rec, step, ev, K))


def _q64(D, eps, B, K, h):
    _, plus, minus = _blocks(D.double().cpu(), B, K)
    return sum((eps[p].double() * (plus[p] - minus[p])).flatten(1).sum(1) for p in range(K)) / (2.0 * h * K)


@pytest.mark.parametrize("shape,offset,K", [((4, 3, 32, 32), 0, 2), ((5, 3, 7, 9), 0, 1), ((4, 3, 32, 32), 1, 3)],
                         ids=["cifar-vec", "odd-scalar", "misaligned-scalar"])
def test_div_kernels_vs_fp64(ops, shape, offset, K):
    B, d = shape[0], int(np.prod(shape[1:]))
    solve_index, step = 2, 9
    t0, t1 = 1.7, 2.9
    h0, h1 = float(np.float32(0.0177)), float(np.float32(0.0302))
    rec = ops.churn_record(SEED, solve_index, DEV)
    full = ((1 + 2 * K) * B,) + shape[1:]
    x = _rand(shape, 2, offset)
    E = _rand(full, 0, offset)
    E.copy_(ops.nll_probe(x, h0, rec, step, 0, K))
    D = _rand(full, 3, offset)
    L0 = torch.randn(B, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(DEV) * 100
    worst = 0.0

    def euler():
        L = L0.clone()
        dx, E1 = ops.heun_euler_div(E, D, t0, t1, h0, h1, rec, step, L, K)
        return L, dx, E1
    L, dx, E1 = euler()
    ops.check_health(DEV, "heun_euler_div")
    dx_ref, x1_ref = ops.heun_euler(E[:B].contiguous(), D[:B].contiguous(), t0, t1)
    assert torch.equal(dx, dx_ref) and torch.equal(E1[:B], x1_ref)
    eps1 = R.probe_signs(shape, SEED, solve_index, step, 1, K).to(DEV)
    h1_32 = torch.tensor(h1, dtype=torch.float32, device=DEV)
    _, plus, minus = _blocks(E1, B, K)
    for p in range(K):
        assert torch.equal(plus[p], x1_ref + h1_32 * eps1[p]) and torch.equal(minus[p], x1_ref - h1_32 * eps1[p])
    c = (np.float64(np.float32(t1)) - np.float64(np.float32(t0))) * 0.5 / np.float64(np.float32(t0))
    q = d - (L - L0).cpu() / c
    q64 = _q64(D, R.probe_signs(shape, SEED, solve_index, step, 0, K), B, K, h0)
    e = ((q - q64).abs() / d).max().item()
    print(f"heun_euler_div {shape} off {offset} K {K}: |q - q64| / d {e:.3e}, |q| / d up to {(q64.abs() / d).max():.3e}")
    worst = max(worst, e)
    L2, dx2, E12 = euler()
    assert torch.equal(L, L2) and torch.equal(dx, dx2) and torch.equal(E1, E12)          # run == run, bit for bit

    # the correction, with and without the next step's probes
    D1 = _rand(full, 5, offset)
    for nxt in (True, False):
        L = L0.clone()
        out = ops.heun_correct_div(E, dx, E1, D1, t0, t1, h1, rec, step, L, K, h_next=h0 if nxt else None)
        ops.check_health(DEV, "heun_correct_div")
        ref = ops.heun_correct(E[:B].contiguous(), dx, E1[:B].contiguous(), D1[:B].contiguous(), t0, t1)
        assert torch.equal(out[:B], ref) and out.shape[0] == ((1 + 2 * K) * B if nxt else B)
        if nxt:
            epsn = R.probe_signs(shape, SEED, solve_index, step - 1, 0, K).to(DEV)
            h0_32 = torch.tensor(h0, dtype=torch.float32, device=DEV)
            _, plus, minus = _blocks(out, B, K)
            for p in range(K):
                assert torch.equal(plus[p], ref + h0_32 * epsn[p]) and torch.equal(minus[p], ref - h0_32 * epsn[p])
        c1 = (np.float64(np.float32(t1)) - np.float64(np.float32(t0))) * 0.5 / np.float64(np.float32(t1))
        q = d - (L - L0).cpu() / c1
        q64 = _q64(D1, eps1.cpu(), B, K, h1)
        e = ((q - q64).abs() / d).max().item()
        print(f"heun_correct_div {shape} off {offset} K {K} next {nxt}: |q - q64| / d {e:.3e}")
        worst = max(worst, e)
        La = L0.clone()
        assert torch.equal(ops.heun_correct_div(E, dx, E1, D1, t0, t1, h1, rec, step, La, K, h_next=h0 if nxt else None), out)
        assert torch.equal(La, L)
    record(f"likelihood/div_kernels_{'x'.join(map(str, shape))}_off{offset}_q_over_d", worst, Q_KERNEL_LIMIT)
    assert worst <= Q_KERNEL_LIMIT, worst

    # the prior term
    L = torch.zeros(B, dtype=torch.float64, device=DEV)
    ops.nll_prior(x, 2.5, L)
    ref = R.log_normal(x.cpu(), 2.5 ** 2)
    e = ((L.cpu() - ref).abs() / ref.abs()).max().item()
    print(f"nll_prior {shape}: |L - L64| / |L64| {e:.3e}")
    record(f"likelihood/prior_{'x'.join(map(str, shape))}_off{offset}_rel", e, 1e-13)
    assert e <= 1e-13, e          # fp64 throughout, a few thousand terms of one sign: a few ulp of 1.1e-16


def test_nonfinite_sets_health(ops):
    shape, K, B = (2, 3, 8, 8), 1, 2
    rec = ops.churn_record(1, 0, DEV)
    x = _rand(shape, 7)
    E = ops.nll_probe(x, 0.01, rec, 3, 0, K)
    ops.check_health(DEV, "before")
    for row in (0, B):              # a NaN in D(x) poisons the state, one in D(x + h eps) only L: both leave the bit
        D = _rand(tuple(E.shape), 8)
        D[row, 1, 2, 3] = float("nan")          # a plain tensor write
        L = torch.zeros(B, dtype=torch.float64, device=DEV)
        _, E1 = ops.heun_euler_div(E, D, 1.0, 2.0, 0.01, 0.02, rec, 3, L, K)
        nan_state, nan_L = bool(torch.isnan(E1[0]).any()), bool(torch.isnan(L[0]))
        with pytest.raises(ops.GraphCorruptionError):
            ops.check_health(DEV, "planted NaN")
        assert (nan_state, nan_L) == ((True, False) if row == 0 else (False, True))
        assert not torch.isnan(E1[1]).any() and not torch.isnan(L[1])
    ops.check_health(DEV, "cleared")
    bad = x.clone()
    bad[1, 0, 0, 0] = float("inf")
    ops.nll_probe(bad, 0.01, rec, 3, 0, K)
    with pytest.raises(ops.GraphCorruptionError):
        ops.check_health(DEV, "planted inf")


def test_ops_reject_bad_operands(ops):
    rec = ops.churn_record(1, 0, DEV)
    x = _rand((2, 3, 4, 4), 1)
    L = torch.zeros(2, dtype=torch.float64, device=DEV)
    E = ops.nll_probe(x, 0.1, rec, 1, 0, 1)
    for fn in (lambda: ops.nll_probe(x, 0.1, rec, 1 << 16), lambda: ops.nll_probe(x, 0.0, rec, 1),
               lambda: ops.nll_probe(x, 0.1, rec, 1, 2), lambda: ops.nll_probe(x, 0.1, rec, 1, 0, 33),
               lambda: ops.nll_probe(x, 0.1, rec[:3], 1), lambda: ops.nll_probe(x.double(), 0.1, rec, 1),
               lambda: ops.heun_euler_div(E, E[:4], 1.0, 2.0, 0.1, 0.1, rec, 1, L),
               lambda: ops.heun_euler_div(E, E, 1.0, 2.0, 0.1, 0.1, rec, 1 << 16, L),
               lambda: ops.heun_euler_div(E, E, 1.0, 2.0, 0.1, 0.1, rec, 1, L.float()),
               lambda: ops.heun_euler_div(E, E, 1.0, 2.0, 0.1, 0.1, rec, 1, L, 2),
               lambda: ops.heun_euler_div(E, E, 0.0, 2.0, 0.1, 0.1, rec, 1, L),
               lambda: ops.heun_correct_div(E, x, E, E, 1.0, 2.0, 0.1, rec, 0, L, h_next=0.1),
               lambda: ops.heun_correct_div(E, E, E, E, 1.0, 2.0, 0.1, rec, 1, L),
               lambda: ops.heun_correct_div(E, x, E, E, 1.0, 2.0, 0.1, rec, 1 << 16, L),
               lambda: ops.nll_prior(x, 0.0, L), lambda: ops.nll_prior(x, 1.0, L[:1])):
        with pytest.raises((ValueError, TypeError)):
            fn()


# ------------------------------------------------------------------ analytic: a diagonal Gaussian
MU = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64).view(1, 3, 1, 1)
SV = torch.tensor([0.25, 0.5, 1.0], dtype=torch.float64).view(1, 3, 1, 1)


def _gaussian(x, s, labels=None):
    """D(x; t) = mu + S / (S + t^2) (x - mu), diagonal S distinct per channel: linear, diagonal Jacobian"""
    s = s.double()
    mu, sv = MU.to(x.device), SV.to(x.device)
    return (mu + sv / (sv + s * s) * (x.double() - mu)).float()


def _analytic_image():
    g = torch.Generator().manual_seed(1)
    return (MU + SV.sqrt() * torch.randn(16, 3, 8, 8, generator=g, dtype=torch.float64)).float()


def _closed_form(img, t_last):
    var = (SV + t_last ** 2).expand(img.shape)
    return (-0.5 * torch.log(2 * math.pi * var) - (img.double() - MU) ** 2 / (2 * var)).flatten(1).sum(1)


def _recursion64(img, t, end=0):
    return R.nll_recursion(lambda x, i: MU + SV / (SV + t[i] ** 2) * (x - MU),
                           lambda x, i, step, ev: (SV / (SV + t[i] ** 2)).expand(x.shape).flatten(1).sum(1),
                           img.double(), t, end)


def test_analytic_log_likelihood(ops):
    import tinyedm_amd as T
    img = _analytic_image()
    d = img[0].numel()
    err, worst_a, worst_c = {}, 0.0, 0.0
    for N in (16, 32, 64):      # (the fp64 restatement itself falls by >= 3.8x at both doublings: test_likelihood_cpu.py)
        sol = T.DeterministicSolver(num_steps=N, seed=11)
        t = sol.t_steps.double()
        lp, lat = sol.log_likelihood(_gaussian, img.to(DEV), return_latent=True)
        assert lp.dtype == torch.float64 and lp.shape == (16,) and sol.solve_index == 1
        ref, _ = _recursion64(img, t)
        a = ((lp.cpu() - ref).abs() / d).max().item()                   # (a) the same discrete recursion in fp64
        err[N] = ((lp.cpu() - _closed_form(img, t[N - 1])).abs() / d).max().item()
        sol2 = T.DeterministicSolver(num_steps=N, seed=12345)
        c = ((sol2.log_likelihood(_gaussian, img.to(DEV)) - lp).abs() / d).max().item()       # (c) another seed
        print(f"analytic N {N}: vs fp64 recursion {a:.3e} nats/dim, vs closed form {err[N]:.3e}, seed to seed {c:.3e}")
        worst_a, worst_c = max(worst_a, a), max(worst_c, c)
        assert torch.equal(lat, T.DeterministicSolver(num_steps=N).invert(_gaussian, img.to(DEV)))      # (d)
    ops.check_health(DEV, "analytic log_likelihood")
    record("likelihood/analytic_vs_fp64_recursion_nats_per_dim", worst_a, ANALYTIC_LIMIT)
    record("likelihood/analytic_seed_to_seed_nats_per_dim", worst_c, ANALYTIC_LIMIT)
    assert worst_a <= ANALYTIC_LIMIT, worst_a
    # a diagonal Jacobian is estimated exactly by any Rademacher probe: what is left between two seeds is the rounding
    # of the difference quotient, the same rounding that separates the GPU from the fp64 recursion
    assert worst_c <= ANALYTIC_LIMIT, worst_c
    assert err[16] / err[32] >= 3.5 and err[32] / err[64] >= 3.5, err             # (b) second order


def test_analytic_end_step_and_probes(ops):
    import tinyedm_amd as T
    img = _analytic_image()
    d = img[0].numel()
    sol = T.DeterministicSolver(num_steps=32, seed=5)
    t = sol.t_steps.double()
    worst = 0.0
    for end, K in ((6, 1), (6, 4), (16, 2), (31, 1)):
        lp, lat = sol.log_likelihood(_gaussian, img.to(DEV), end_step=end, num_probes=K, return_latent=True)
        ref, _ = _recursion64(img, t, end)
        assert torch.equal(lat, sol.invert(_gaussian, img.to(DEV), end_step=end))
        if end == 31:           # no step: the fp64 prior of the fp32 image at t_{N-1}, O(1e5) nats/dim
            assert ((lp.cpu() - ref).abs() / ref.abs()).max().item() <= 1e-13
            continue
        worst = max(worst, ((lp.cpu() - ref).abs() / d).max().item())
    print(f"analytic end_step / num_probes: vs fp64 recursion {worst:.3e} nats/dim")
    record("likelihood/analytic_end_probes_vs_fp64_recursion_nats_per_dim", worst, ANALYTIC_LIMIT)
    assert worst <= ANALYTIC_LIMIT, worst
    assert sol.solve_index == 4


# ------------------------------------------------------------------ the tiny networks vs the CPU oracle
SCHED = dict(num_steps=8, sigma_min=0.01, sigma_max=20.0, rho=5.0)


def _edm(P, ecfg, dcfg, dtype):
    """an eval-mode EDM on the GPU with the oracle's parameters (the pattern of tests/test_image_conditioned_gpu.py)"""
    import tinyedm_amd as T
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), dcfg.dropout_rate,
                     dcfg.sigma_data, dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    emb.load_state_dict({k[len("embedding."):]: v for k, v in P.items() if k.startswith("embedding.")}, strict=True)
    den.load_state_dict({k[len("denoiser."):]: v for k, v in P.items() if k.startswith("denoiser.")}, strict=True)
    den.set_eval_dtype(dtype)
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                  steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01)
    return model.to(DEV).eval()


def _net(num_classes, dtype):
    em, dm = tiny_cfgs(num_classes)
    P = O.init_params(em, dm, torch.Generator().manual_seed(7))
    return P, em, dm, _edm(P, em, dm, dtype)


def _net_inputs(num_classes):
    g = torch.Generator().manual_seed(4)
    image = 0.5 * torch.randn(3, 3, 8, 8, generator=g)
    labels = torch.randint(0, 10, (3,), generator=g) if num_classes else None
    return image, labels


def kernel_q(ops, model, x, sigma, labels, h, rec, step, K):
    """the estimator's q of one evaluation, through the kernels: the probes, one network call on the (1 + 2K) B batch, and
    the divergence sum read back from L; also the eps the probe kernel drew, read back as (x+ - x) / h, and D"""
    B, d = x.shape[0], x[0].numel()
    E = ops.nll_probe(x, h, rec, step, 0, K)
    lab = None if labels is None else labels.repeat(1 + 2 * K)
    with torch.no_grad():
        D = model(E, torch.tensor(sigma, device=DEV), lab).float().contiguous()
    L = torch.zeros(B, dtype=torch.float64, device=DEV)
    t0 = float(np.float32(sigma))
    ops.heun_euler_div(E, D, t0, 2 * t0, h, h, rec, step, L, K)
    q = d - L.cpu() / 0.5           # c = (2 t0 - t0) / 2 / t0
    _, plus, _ = _blocks(E, B, K)
    eps = torch.stack([((p - x) / torch.tensor(h, dtype=torch.float32, device=DEV)).round() for p in plus]).cpu()
    return q, eps, D


@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
@pytest.mark.parametrize("num_classes", [None, 10], ids=["uncond", "cond"])
def test_q_per_evaluation_vs_oracle(ops, dtype, num_classes):
    import tinyedm_amd as T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    P, em, dm, model = _net(num_classes, dtype)
    image, labels = _net_inputs(num_classes)
    sol = T.DeterministicSolver(**SCHED)
    rec = ops.churn_record(SEED, 0, DEV)
    d = image[0].numel()
    worst = 0.0
    g = torch.Generator().manual_seed(9)
    for i in (0, 2, 4, 6, 7):               # across the table: sigma 20 ... 0.01
        sigma = sol.t_steps[i].item()
        h = sol.probe_widths(dm.sigma_data)[i]
        x = image + sigma * torch.randn(image.shape, generator=g)
        for K in (1, 3):
            q, eps, D = kernel_q(ops, model, x.to(DEV), sigma, None if labels is None else labels.to(DEV), h, rec, i, K)
            assert torch.equal(eps, R.probe_signs(tuple(x.shape), SEED, 0, i, 0, K))
            q_or = R.oracle_q(O, P, em, dm, x, sigma, labels, eps)
            e = ((q - q_or).abs() / d).max().item()
            print(f"q {dtype} classes {num_classes} sigma {sigma:.4g} K {K}: |q - q_oracle| / d {e:.3e}  (q / d "
                  f"{(q_or / d).mean():.4f})")
            worst = max(worst, e)
            if K == 3:          # the mean of the three single-probe quotients, to rounding
                q1 = _q64(D, eps, x.shape[0], K, h)
                assert ((q - q1).abs() / d).max().item() <= 1e-12
    record(f"likelihood/q_per_evaluation_{dtype}_{'cond' if num_classes else 'uncond'}_over_d", worst, Q_NET_LIMIT[dtype])
    assert worst <= Q_NET_LIMIT[dtype], worst


@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
@pytest.mark.parametrize("num_classes,end,K", [(None, 0, 1), (10, 5, 3), (10, 0, 1)], ids=["uncond-0-1", "cond-5-3", "cond-0-1"])
def test_log_likelihood_vs_oracle(ops, dtype, num_classes, end, K):
    import tinyedm_amd as T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    P, em, dm, model = _net(num_classes, dtype)
    image, labels = _net_inputs(num_classes)
    sol = T.DeterministicSolver(seed=SEED, **SCHED)
    sol.solve_index = 2
    d = image[0].numel()
    lp, lat = sol.log_likelihood(model, image.to(DEV), None if labels is None else labels.to(DEV), end_step=end,
                                 num_probes=K, return_latent=True)
    ops.check_health(DEV, "log_likelihood")
    assert sol.solve_index == 3
    assert torch.equal(lat, sol.invert(model, image.to(DEV), None if labels is None else labels.to(DEV), end_step=end))
    t = sol.t_steps

    def D(x, i):
        with torch.no_grad():
            return O.edm_forward(P, em, dm, x, t[i].expand(x.shape[0]), labels).float()

    def q(x, i, step, ev):      # the oracle's exact eps . J eps under the probes the kernels drew
        return R.oracle_q(O, P, em, dm, x, t[i].item(), labels, R.probe_signs(tuple(x.shape), SEED, 2, step, ev, K))
    ref, lat_ref = R.nll_recursion(D, q, image.float(), t.double(), end)
    e = ((lp.cpu() - ref).abs() / d).max().item()
    print(f"log_likelihood {dtype} classes {num_classes} end {end} K {K}: {e:.3e} nats/dim vs the oracle recursion "
          f"(logp / d {(ref / d).tolist()})")
    record(f"likelihood/logp_{dtype}_{'cond' if num_classes else 'uncond'}_end{end}_K{K}_nats_per_dim", e, LOGP_NET_LIMIT[dtype])
    assert e <= LOGP_NET_LIMIT[dtype], e
    # the change-of-variables term is not a rounding matter: without it the value is off by O(1) nats/dim
    assert ((R.log_normal(lat_ref * t[end].item(), t[end].item() ** 2) - ref).abs() / d).min().item() > 100 * e


def test_bf16_evaluation_is_refused(ops):
    import tinyedm_amd as T
    _, _, _, model = _net(10, "bf16")
    image, labels = _net_inputs(10)
    with pytest.raises(ValueError, match="bf16"):
        T.DeterministicSolver(**SCHED).log_likelihood(model, image.to(DEV), labels.to(DEV))


@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
def test_hipgraph_equals_eager_and_replays(ops, dtype):
    import tinyedm_amd as T
    _, _, _, model = _net(10, dtype)
    image, labels = _net_inputs(10)
    image, labels = image.to(DEV), labels.to(DEV)
    eager, graph = T.DeterministicSolver(seed=3, **SCHED), T.DeterministicSolver(seed=3, **SCHED)
    for k, img in enumerate((image, image.flip(0).contiguous(), image)):          # capture, then two replays
        a = eager.log_likelihood(model, img, labels, end_step=2, num_probes=2, return_latent=True)
        b = graph.log_likelihood(model, img, labels, graph=True, end_step=2, num_probes=2, return_latent=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), k
        assert eager.solve_index == graph.solve_index == k + 1 and len(graph._graphs[model]) == 1
    # same image, another solve index: other probes, another estimate; setting the index back reproduces the first
    first = graph.log_likelihood(model, image, labels, graph=True, end_step=2, num_probes=2)
    assert not torch.equal(first, b[0])
    graph.solve_index = 0
    again = graph.log_likelihood(model, image, labels, graph=True, end_step=2, num_probes=2)
    eager.solve_index = 0
    assert torch.equal(again, eager.log_likelihood(model, image, labels, end_step=2, num_probes=2))
    # its own cache entries: per (end_step, num_probes, delta), and apart from invert's
    graph.invert(model, image, labels, graph=True, end_step=2)
    assert len(graph._graphs[model]) == 2
    graph.log_likelihood(model, image, labels, graph=True, end_step=2, num_probes=1)
    assert len(graph._graphs[model]) == 3
    graph.delta = 2e-2
    graph.log_likelihood(model, image, labels, graph=True, end_step=2, num_probes=1)
    assert len(graph._graphs[model]) == 4
    assert any("nll" in key for key in graph._graphs[model]) and any("invert" in key for key in graph._graphs[model])
    ops.check_health(DEV, "log_likelihood(graph=True)")


# ------------------------------------------------------------------ generate CLI
CLI = ["--config_name", "cifar10_cond", "--num_samples", "4", "--batch_size", "4", "--num_steps", "4", "--num_classes",
       "10", "--image_size", "32", "--num_workers", "0"]


def _generate(out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "generate.py"), "--output_dir", str(out), *CLI, *extra]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_generate_cli_likelihood(ops, tmp_path):
    from tinyedm_amd import generate as G
    from tinyedm_amd.solvers import NLL_DELTA, bits_per_dim
    _generate(tmp_path / "plain")
    out = tmp_path / "nll.json"
    _generate(tmp_path / "unused", "--init_dir", str(tmp_path / "plain"), "--likelihood_to", str(out), "--num_probes", "2",
              "--dequantize", "--seed", "3")
    assert not os.path.exists(tmp_path / "unused" / "0.png")
    with open(out) as f:
        res = json.load(f)
    assert {"logp", "bpd", "logp_mean", "bpd_mean", "num_steps", "num_probes", "delta", "seed", "network_dtype"} <= set(res)
    assert res["num_steps"] == 4 and res["num_probes"] == 2 and res["seed"] == 3 and res["network_dtype"] == "f32x3"
    assert res["delta"] == NLL_DELTA and len(res["logp"]) == len(res["bpd"]) == 4
    logp, bpd = torch.tensor(res["logp"], dtype=torch.float64), torch.tensor(res["bpd"], dtype=torch.float64)
    assert bool(torch.isfinite(logp).all()) and bool(torch.isfinite(bpd).all())
    want = bits_per_dim(logp, 3 * 32 * 32, [2.0 * s for s in G.CIFAR_STD])       # load_images: x = (pixel - mean) / (2 std)
    assert torch.allclose(bpd, want, rtol=0, atol=1e-12)
    assert abs(res["logp_mean"] - logp.mean().item()) <= 1e-9 and abs(res["bpd_mean"] - bpd.mean().item()) <= 1e-12
