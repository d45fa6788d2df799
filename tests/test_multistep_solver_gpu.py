"""DPM-Solver++ multistep sampling on the GPU (MultistepSolver, ops.dpm_multistep):

 * the update kernel (solver_steps.hip) against an fp64 restatement, for each order, guided and unguided, on the dwordx4 path,
   its scalar tail and the scalar path of a misaligned operand; w = 0 is bit-identical to the unguided kernel fed
   D_guide; the final row (0, 1, 0, 0) returns the mixed D itself; a NaN raises the health bit; bad operands raise;
 * convergence on two analytic denoisers (a Gaussian with its exact solution, a 4-component Gaussian mixture against an
   fp64 Heun solve of 2048 steps) on the default Karras table, with the means and x0 drawn from torch.manual_seed(0): 2M is second order and within 1.2x of Heun at the same
   N, the first-order solve is first order, 3M is at least 3x more accurate than 2M at N = 24 and 32;
 * trajectories of tiny nets against a CPU restatement of the recursion around the oracle's forward, bf16 and "f32",
   unguided and CFG at w = 2.  Limits: the Heun ones (bf16 1e-2, tests/test_network_gpu.py; f32 2e-4,
   tests/test_evalf32_gpu.py), 3x when guided as in tests/test_guided_solver_gpu.py;
 * identities: the final x is the last mixed D bit for bit, order 1 is EDM's Euler solve, guidance 1 never evaluates
   the guide and is the unguided solve, guidance 0 is the guide's solve;
 * the hipGraph path: replays bit-identical to eager, a replay with a new x0 is right (no stale history), a new
   guidance weight replays the same graph, a new order or interval captures a new one, Heun and multistep solves of one
   model keep separate entries;
 * the generate CLI and EDM.predict_step end to end."""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs
from parity_log import record

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------ kernel
def _operands(n, offset, seed):
    g = torch.Generator().manual_seed(seed)
    # offset 1: every operand starts one float past a 16-byte boundary -> the kernel's scalar path
    return [torch.randn(n + 1, generator=g).to(DEV)[offset:offset + n] for _ in range(5)]


def _row(order):
    """a real row of effective order `order` (step 5 of the default 18-step table)"""
    import tinyedm_amd as T
    return T.MultistepSolver(num_steps=18, order=order).multistep_coefficients()[5].tolist()


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("n,offset", [(3 * 32 * 32 * 7, 0), (4099, 0), (4099, 1)],
                         ids=["n21504", "n4099-tail", "n4099-misaligned"])
def test_dpm_multistep_vs_fp64(ops, n, offset, order, guided):
    x, Dm, Dg, m1, m2 = _operands(n, offset, n + offset + 10 * order)
    assert x.is_contiguous() and (x.data_ptr() % 16 == 0) == (offset == 0)
    a, c0, c1, c2 = _row(order)
    assert (c1 != 0) == (order >= 2) and (c2 != 0) == (order == 3)
    w = 2.0
    w_dev = torch.full((1,), w, device=DEV)
    h1, h2 = (m1 if order >= 2 else None), (m2 if order == 3 else None)
    m_out = torch.empty(n + 1, device=DEV)[offset:offset + n]
    kw = dict(Dg=Dg, w_dev=w_dev) if guided else {}
    out = ops.dpm_multistep(x, Dm, a, c0, c1, c2, m1=h1, m2=h2, m_out=m_out, **kw)
    ops.check_health(x.device, "dpm_multistep")
    X, M, G, H1, H2 = (v.double() for v in (x, Dm, Dg, m1, m2))
    m_ref = G + w * (M - G) if guided else M
    m_mag = (G.abs() + w * (M - G).abs()) if guided else M.abs()
    ref = a * X + c0 * m_ref
    mag = abs(a) * X.abs() + abs(c0) * m_mag
    if order >= 2:
        ref, mag = ref + c1 * H1, mag + abs(c1) * H1.abs()
    if order == 3:
        ref, mag = ref + c2 * H2, mag + abs(c2) * H2.abs()
    # fp32 evaluation: the mix (2 roundings of m, scaled by |c0|) and at most 4 roundings of partial sums <= mag
    assert ((out.double() - ref).abs() <= 8 * EPS32 * mag + 1e-30).all()
    assert ((m_out.double() - m_ref).abs() <= 2 * EPS32 * m_mag + 1e-30).all()
    if not guided:
        assert torch.equal(m_out, Dm)

    # w = 0: bit-identical to the unguided kernel fed D_guide
    w0 = torch.zeros(1, device=DEV)
    mo0, mou = torch.empty_like(x), torch.empty_like(x)
    o0 = ops.dpm_multistep(x, Dm, a, c0, c1, c2, Dg=Dg, w_dev=w0, m1=h1, m2=h2, m_out=mo0)
    ou = ops.dpm_multistep(x, Dg, a, c0, c1, c2, m1=h1, m2=h2, m_out=mou)
    assert torch.equal(o0, ou) and torch.equal(mo0, mou) and torch.equal(mou, Dg)
    # the final row returns the mixed D itself
    last = ops.dpm_multistep(x, Dm, 0.0, 1.0, **kw)
    if guided:
        mix = torch.empty_like(x)
        ops.dpm_multistep(x, Dm, a, c0, Dg=Dg, w_dev=w_dev, m_out=mix)
        assert torch.equal(last, mix)
    else:
        assert torch.equal(last, Dm)
    ops.check_health(x.device, "dpm_multistep, w = 0")


def test_dpm_multistep_nonfinite_sets_health(ops):
    n = 4099
    x, Dm, Dg, m1, m2 = _operands(n, 0, 5)
    a, c0, c1, c2 = _row(3)
    w_dev = torch.full((1,), 2.0, device=DEV)
    ops.check_health(x.device, "before")
    Dg[4097] = float("nan")                  # in the scalar tail
    ops.dpm_multistep(x, Dm, a, c0, c1, c2, Dg=Dg, w_dev=w_dev, m1=m1, m2=m2)
    with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
        ops.check_health(x.device, "dpm_multistep")
    m2[17] = float("inf")                    # in the dwordx4 body
    ops.dpm_multistep(x, Dm, a, c0, c1, c2, m1=m1, m2=m2)
    with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
        ops.check_health(x.device, "dpm_multistep")
    ops.check_health(x.device, "after")      # the read cleared the word


def test_dpm_multistep_rejects_bad_operands(ops):
    x, Dm, Dg, m1, m2 = _operands(64, 0, 3)
    w_dev = torch.full((1,), 2.0, device=DEV)
    with pytest.raises(ValueError):
        ops.dpm_multistep(x, Dm[:32], 0.5, 0.5)
    with pytest.raises(TypeError):
        ops.dpm_multistep(x, Dm, 0.5, 0.5, Dg=Dg.double(), w_dev=w_dev)
    with pytest.raises(ValueError, match="w_dev"):
        ops.dpm_multistep(x, Dm, 0.5, 0.5, Dg=Dg, w_dev=torch.full((2,), 2.0, device=DEV))
    with pytest.raises(RuntimeError):
        ops.dpm_multistep(x, Dm, 0.5, 0.5, Dg=Dg, w_dev=torch.full((1,), 2.0))
    with pytest.raises(ValueError, match="together"):
        ops.dpm_multistep(x, Dm, 0.5, 0.5, Dg=Dg)
    with pytest.raises(ValueError, match="m1"):
        ops.dpm_multistep(x, Dm, 0.5, 0.5, 0.1)
    with pytest.raises(ValueError, match="m2"):
        ops.dpm_multistep(x, Dm, 0.5, 0.5, 0.1, 0.1, m2=m2)
    with pytest.raises(ValueError, match="contiguous"):
        ops.dpm_multistep(x, Dm, 0.5, 0.5, 0.1, m1=torch.randn(128, device=DEV)[::2])
    with pytest.raises(ValueError, match="m1"):
        ops.dpm_multistep(x, Dm, 0.5, 0.5, 0.1, m1=m1[:32])
    with pytest.raises(ValueError, match="alias"):
        ops.dpm_multistep(x, Dm, 0.5, 0.5, 0.1, m1=m1, m_out=m1)
    with pytest.raises(ValueError, match="finite"):
        ops.dpm_multistep(x, Dm, math.nan, 0.5)


# ------------------------------------------------------------------ convergence on analytic denoisers
MU, SD = 0.3, 0.5


def _gaussian(x, s, labels=None):
    s = s.double()
    return (MU + SD ** 2 / (SD ** 2 + s * s) * (x.double() - MU)).float()


def _mixture(means):
    means = means.to(DEV)
    stds = torch.tensor([0.1, 0.2, 0.3, 0.15], dtype=torch.float64, device=DEV)
    logw = torch.tensor([0.1, 0.2, 0.3, 0.4], dtype=torch.float64, device=DEV).log()

    def D(x, s, labels=None):
        """the posterior mean E[y | y + s n = x] of the mixture, in fp64"""
        xs = x.double().reshape(x.shape[0], 1, -1)
        v = stds ** 2 + s.double() ** 2
        logp = logw - 0.5 * ((xs - means) ** 2).sum(-1) / v - 0.5 * means.shape[1] * v.log()
        p = torch.softmax(logp, dim=1)
        post = means + (stds ** 2 / v)[:, None] * (xs - means)
        return (p[:, :, None] * post).sum(1).reshape(x.shape).to(x.dtype)
    return D


def _heun64(D, x0, N):
    """EDM's Heun solve in fp64 (the mixture's reference)"""
    import tinyedm_amd as T
    t = T.DeterministicSolver(num_steps=N).t_steps.double().to(DEV)
    x1 = x0.double() * t[0]
    for i in range(N):
        x, t0, t1 = x1, t[i], t[i + 1]
        dx = (x - D(x, t0)) / t0
        x1 = x + (t1 - t0) * dx
        if i < N - 1:
            x1 = x + (t1 - t0) * (0.5 * dx + 0.5 * (x1 - D(x1, t1)) / t1)
    return x1


@pytest.fixture(scope="module")
def denoisers(ops):
    import tinyedm_amd as T
    # torch.manual_seed(0)'s stream: the mixture's means, then 64 samples x0 ~ N(0, I) of d = 192, both fp64
    g = torch.Generator().manual_seed(0)
    means = 0.5 * torch.randn(4, 192, generator=g, dtype=torch.float64)
    x0 = torch.randn(64, 192, generator=g, dtype=torch.float64).float().reshape(64, 3, 8, 8).to(DEV)
    s0 = T.DeterministicSolver().t_steps[0].item()
    exact = MU + SD * (x0.double() * s0 - MU) / math.sqrt(SD ** 2 + s0 ** 2)
    mix = _mixture(means)
    return x0, {"gaussian": (_gaussian, exact), "mixture": (mix, _heun64(mix, x0, 2048))}


@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_convergence_on_analytic_denoisers(denoisers, name):
    import tinyedm_amd as T
    x0, dens = denoisers
    D, ref = dens[name]

    def err(solver):
        return rel(solver.solve(D, x0), ref)
    heun = {N: err(T.DeterministicSolver(num_steps=N)) for N in (16, 32, 64)}
    e = {(o, N): err(T.MultistepSolver(num_steps=N, order=o)) for o, Ns in ((1, (32, 64)), (2, (16, 24, 32, 64)),
                                                                            (3, (24, 32))) for N in Ns}
    assert e[2, 32] / e[2, 64] >= 3.5, e                         # second order
    assert 1.6 <= e[1, 32] / e[1, 64] <= 2.4, e                  # first order
    for N in (16, 32, 64):
        assert e[2, N] <= 1.2 * heun[N], (N, e[2, N], heun[N])   # half the evaluations, about Heun's error
    for N in (24, 32):
        assert e[3, N] <= e[2, N] / 3, (N, e[3, N], e[2, N])


# ------------------------------------------------------------------ trajectories vs the CPU oracle
def _edm(P, ecfg, dcfg, dtype):
    """an eval-mode EDM on the GPU with the oracle's parameters (the _cifar pattern of tests/test_evalf32_gpu.py)"""
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


def _oracle_D(Pm, em, dm, bf16, guide=None):
    def D(x, s, labels):
        sig = s.reshape(-1).expand(x.shape[0])
        Dm = O.edm_forward(Pm, em, dm, x, sig, labels, bf16=bf16).float()
        if guide is None:
            return Dm
        Pg, eg, dg, w = guide
        gl = labels if eg.num_classes is not None else None     # an unconditional EDM drops the labels
        Dg = O.edm_forward(Pg, eg, dg, x, sig, gl, bf16=bf16).float()
        return Dg + w * (Dm - Dg)
    return D


def _oracle_multistep(D, x0, t, coef, labels):
    """the multistep recursion on the CPU: x_{i+1} = a x + c0 m_i + c1 m_{i-1} + c2 m_{i-2}, from the solver's table"""
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


SCHED = dict(num_steps=6, sigma_min=0.01, sigma_max=20.0, rho=5.0)


@pytest.mark.parametrize("case", ["o2_bf16", "o2_f32", "o3_bf16", "o3_f32", "o2_cfg_bf16", "o3_cfg_f32"])
def test_multistep_trajectory_vs_oracle(ops, case):
    import tinyedm_amd as T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    order = int(case[1])
    bf16 = case.endswith("bf16")
    dtype = "bf16" if bf16 else "f32"
    em, dm = tiny_cfgs(10)
    Pm = O.init_params(em, dm, torch.Generator().manual_seed(7))
    main = _edm(Pm, em, dm, dtype)
    kw, guide_or = {}, None
    if "cfg" in case:
        eg, dg = tiny_cfgs(None)
        Pg = O.init_params(eg, dg, torch.Generator().manual_seed(11))
        kw = dict(guide=_edm(Pg, eg, dg, dtype), guidance=2.0)
        guide_or = (Pg, eg, dg, 2.0)
    sol = T.MultistepSolver(**SCHED, order=order, **kw)
    coef = sol.multistep_coefficients()
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 3, 8, 8, generator=g)
    labels = torch.randint(0, 10, (2,), generator=g)
    x_hip = sol.solve(main, x0.to(DEV), labels.to(DEV)).cpu()
    with torch.no_grad():
        x_or = _oracle_multistep(_oracle_D(Pm, em, dm, bf16, guide_or), x0, sol.t_steps, coef, labels)
    e = rel(x_hip, x_or)
    lim = (1e-2 if bf16 else 2e-4) * (3 if guide_or is not None else 1)
    record(f"multistep/{case}_trajectory_vs_{'bf16' if bf16 else 'fp32'}_oracle", e, lim)
    assert e <= lim, e
    if guide_or is not None:
        # the guidance must matter at this size: the unguided solve is far from the guided oracle
        x_main = T.MultistepSolver(**SCHED, order=order).solve(main, x0.to(DEV), labels.to(DEV)).cpu()
        assert rel(x_main, x_or) > 5 * e
    if not bf16:
        # and so must the order: the solve of the other order is far from this one's oracle
        x_alt = T.MultistepSolver(**SCHED, order=5 - order, **kw).solve(main, x0.to(DEV), labels.to(DEV)).cpu()
        assert rel(x_alt, x_or) > 5 * e


# ------------------------------------------------------------------ identities and the hipGraph path
@pytest.fixture(scope="module")
def pair(ops):
    em, dm = tiny_cfgs(10)
    eg, dg = tiny_cfgs(None)
    main = _edm(O.init_params(em, dm, torch.Generator().manual_seed(7)), em, dm, "bf16")
    guide = _edm(O.init_params(eg, dg, torch.Generator().manual_seed(11)), eg, dg, "bf16")
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(3, 3, 8, 8, generator=g).to(DEV)
    labels = torch.randint(0, 10, (3,), generator=g).to(DEV)
    return main, guide, x0, labels


def _solver(**kw):
    import tinyedm_amd as T
    return T.MultistepSolver(**SCHED, **kw)


@pytest.mark.parametrize("order", [1, 2, 3])
def test_final_x_is_the_last_mixed_d(pair, order):
    main, _, x0, labels = pair
    outs = []

    def spy(x, s, c):
        D = main(x, s, c).float().contiguous()
        outs.append(D.clone())
        return D
    x = _solver(order=order).solve(spy, x0, labels)
    assert len(outs) == SCHED["num_steps"]                       # one evaluation per step
    assert torch.equal(x, outs[-1])


def test_order_one_is_edm_euler(pair):
    import tinyedm_amd as T
    main, _, x0, labels = pair
    main.denoiser.set_eval_dtype("f32")
    try:
        x = _solver(order=1).solve(main, x0, labels)
        t = T.DeterministicSolver(**SCHED).t_steps.tolist()
        y = x0 * t[0]
        with torch.no_grad():
            for i in range(SCHED["num_steps"]):                 # EDM's Euler step: x + (t1 - t0) * (x - D) / t0
                D = main(y, torch.tensor(t[i], device=DEV), labels).float()
                y = y + (t[i + 1] - t[i]) * (y - D) / t[i]
    finally:
        main.denoiser.set_eval_dtype("bf16")
    assert rel(x, y) <= 1e-5, rel(x, y)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_guidance_one_is_the_unguided_solve(pair, graph):
    main, guide, x0, labels = pair
    calls = []
    spy = lambda x, s, c: calls.append(1) or guide(x, s, c)        # noqa: E731
    x_g = _solver(order=3, guide=spy, guidance=1.0, guidance_interval=(0.1, 5.0)).solve(main, x0, labels, graph=graph)
    x_u = _solver(order=3).solve(main, x0, labels, graph=graph)
    assert torch.equal(x_g, x_u)
    assert not calls


@pytest.mark.parametrize("order", [2, 3])
def test_guidance_zero_is_the_guide_solve(pair, order):
    main, guide, x0, labels = pair
    x_0 = _solver(order=order, guide=guide, guidance=0.0).solve(main, x0, labels)
    assert torch.equal(x_0, _solver(order=order).solve(guide, x0, labels))


@pytest.mark.parametrize("order", [2, 3])
def test_multistep_hipgraph_replay_and_cache_key(pair, order):
    main, guide, x0, labels = pair
    x0b = torch.randn(x0.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    sol = _solver(order=order, guide=guide, guidance=2.0)
    eager = sol.solve(main, x0, labels)
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager)           # capture
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager)           # pure replay
    # a new x0 through the same graph: the history buffers are rewritten before they are read
    eager_b = sol.solve(main, x0b, labels)
    assert not torch.equal(eager_b, eager)
    assert torch.equal(sol.solve(main, x0b, labels, graph=True), eager_b)
    assert len(sol._graphs[main]) == 1
    # a new guidance weight is a device value: same graph, new result
    sol.guidance = 3.5
    eager = sol.solve(main, x0, labels)
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager)
    assert len(sol._graphs[main]) == 1
    # a new interval changes which evaluations run the guide: a new capture
    sol.guidance_interval = (0.1, 5.0)
    eager = sol.solve(main, x0, labels)
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager)
    assert len(sol._graphs[main]) == 2
    # a new order changes the coefficients baked into the graph: a new capture
    sol.order = 5 - order
    eager = sol.solve(main, x0, labels)
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager)
    assert len(sol._graphs[main]) == 3


def test_heun_and_multistep_keep_separate_entries(pair):
    import tinyedm_amd as T
    main, _, x0, labels = pair
    heun, ms = T.DeterministicSolver(**SCHED), _solver(order=2)
    e_h, e_m = heun.solve(main, x0, labels), ms.solve(main, x0, labels)
    assert not torch.equal(e_h, e_m)
    for _ in range(2):                                  # interleaved captures and replays on one model
        assert torch.equal(heun.solve(main, x0, labels, graph=True), e_h)
        assert torch.equal(ms.solve(main, x0, labels, graph=True), e_m)
    assert len(heun._graphs[main]) == 1 and len(ms._graphs[main]) == 1
    assert set(heun._graphs[main]).isdisjoint(ms._graphs[main])


def test_predict_step_with_multistep_solver(pair):
    main, _, x0, labels = pair
    sol = _solver(order=2)
    main.solver = sol
    try:
        with torch.no_grad():
            out = main.predict_step((x0, labels), 0)
    finally:
        del main.solver
    assert torch.equal(out, sol.solve(main, x0, labels))


# ------------------------------------------------------------------ generate CLI
def _generate(out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "generate.py"), "--config_name", "cifar10_cond",
           "--output_dir", str(out), "--num_samples", "4", "--batch_size", "4", "--num_steps", "3", "--num_classes",
           "10", "--image_size", "32", "--num_workers", "0", *extra]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def _pngs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_generate_cli_dpmpp(ops, tmp_path):
    from PIL import Image
    _generate(tmp_path / "plain")
    plain = _pngs(tmp_path / "plain")
    assert sorted(plain) == [f"{i}.png" for i in range(4)]
    _generate(tmp_path / "heun", "--solver", "heun", "--solver_order", "3")
    assert _pngs(tmp_path / "heun") == plain
    _generate(tmp_path / "o2", "--solver", "dpmpp", "--solver_order", "2")
    o2 = _pngs(tmp_path / "o2")
    assert sorted(o2) == sorted(plain)
    for f in o2:
        assert Image.open(tmp_path / "o2" / f).size == (32, 32)
    assert any(o2[f] != plain[f] for f in o2)
    _generate(tmp_path / "o2b", "--solver", "dpmpp", "--no_graph")         # the eager loop: the same images
    assert _pngs(tmp_path / "o2b") == o2
