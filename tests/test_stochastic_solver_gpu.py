"""Stochastic Heun sampling on the GPU (StochasticSolver, Algorithm 2 of Karras et al. 2022):

 * the churn kernel (ops.heun_churn, solver_steps.hip) against a numpy restatement of Philox4x32-10 + Box-Muller in uint64 /
   fp64, on the dwordx4 path, the scalar path (CHW % 4 != 0) and the scalar path of a misaligned tensor; x + c*n on a
   non-zero x; the noise of a sample does not depend on the batch size or the memory path; different step, solve index
   or seed give uncorrelated N(0, 1) noise; a NaN raises the health bit;
 * stochastic trajectories of tiny nets against the CPU oracle composing Algorithm 2 with the exact GPU noise (drawn by
   ops.heun_churn on zeros), bf16 and "f32", with a window and with CFG guidance.  Limits: the unguided trajectory
   limits (bf16 1e-2, tests/test_network_gpu.py; f32 2e-4, tests/test_evalf32_gpu.py), 3x for the guided case as in
   tests/test_guided_solver_gpu.py;
 * S_churn = 0 is the deterministic solve bit for bit; S_noise = 0 ignores the seed; the seed and solve index
   reproduce a solve;
 * the hipGraph path: replays bit-identical to eager, a new seed or solve index replays the same graph, a new churn
   schedule captures a new one;
 * the generate CLI end to end."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs
from parity_log import record

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------ the noise stream, restated
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


def _box_muller(a, b):
    u1 = ((a >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    u2 = ((b >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)


def _noise_ref(shape, seed, solve_index, step):
    """element j of sample b: normal j % 4 of philox((j / 4, b, 0x43480000 ^ step, solve_index), (seed_lo, seed_hi))"""
    B, CHW = shape[0], int(np.prod(shape[1:]))
    j = np.arange(CHW, dtype=np.uint64)
    b = np.arange(B, dtype=np.uint64)[:, None]
    r = _philox4x32_10(j[None, :] // np.uint64(4) + 0 * b, b + 0 * j[None, :], 0x43480000 ^ step, solve_index,
                       seed & 0xFFFFFFFF, seed >> 32)
    n0, n1 = _box_muller(r[0], r[1])
    n2, n3 = _box_muller(r[2], r[3])
    n = np.stack([n0, n1, n2, n3])                   # [4, B, CHW]
    k = (j % np.uint64(4)).astype(np.int64)
    return np.take_along_axis(n.transpose(1, 2, 0), k[None, :, None], axis=2)[..., 0].reshape(shape)


def _zeros(shape, offset=0):
    n = int(np.prod(shape))
    return torch.zeros(n + offset, device=DEV)[offset:].view(shape)


@pytest.mark.parametrize("shape,offset", [((7, 3, 32, 32), 0), ((5, 3, 7, 9), 0), ((7, 3, 32, 32), 1)],
                         ids=["cifar-vec", "odd-scalar", "misaligned-scalar"])
def test_churn_noise_vs_restatement(ops, shape, offset):
    seed, solve_index, step = 0x9E3779B97F4A7C15, 3, 5
    rec = ops.churn_record(seed, solve_index, DEV)
    x = _zeros(shape, offset)
    assert (x.data_ptr() % 16 == 0) == (offset == 0)
    n = ops.heun_churn(x, 1.0, rec, step)
    ops.check_health(x.device, "heun_churn")
    ref = _noise_ref(shape, seed, solve_index, step)
    err = float(np.abs(n.double().cpu().numpy() - ref).max())
    record(f"stochastic/churn_noise_{'x'.join(map(str, shape))}_off{offset}_maxabs", err, 1e-5)
    assert err <= 1e-5, err      # measured 2.1e-6 (__logf, __sincosf); a wrong counter is O(1)
    if offset:          # the scalar path of a misaligned tensor draws what the dwordx4 path draws, bit for bit
        assert torch.equal(n, ops.heun_churn(_zeros(shape), 1.0, rec, step))


def test_churn_affine_on_nonzero_x(ops):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(6, 3, 16, 16, generator=g).to(DEV)
    rec = ops.churn_record(42, 0, DEV)
    c = 2.75
    n = ops.heun_churn(torch.zeros_like(x), 1.0, rec, 2)
    x_hat = ops.heun_churn(x, c, rec, 2)
    ref = x.double() + c * n.double()
    assert rel(x_hat, ref) <= 1e-7
    assert (x_hat.double() - ref).abs().max().item() <= 4e-7 * ref.abs().max().item()
    # c = 0: x itself, bit for bit
    assert torch.equal(ops.heun_churn(x, 0.0, rec, 2), x)
    ops.check_health(x.device, "heun_churn affine")


def test_churn_noise_independent_of_batch_size(ops):
    rec = ops.churn_record(123, 9, DEV)
    for shape in ((4, 3, 32, 32), (4, 3, 7, 9)):
        n4 = ops.heun_churn(_zeros(shape), 1.0, rec, 1)
        n2 = ops.heun_churn(_zeros((2,) + shape[1:]), 1.0, rec, 1)
        assert torch.equal(n4[:2], n2)


def test_churn_streams_uncorrelated(ops):
    shape = (8, 3, 64, 64)                      # 98 304 elements: corr / mean standard error 0.0032
    draws = {
        "base": (5, 0, 0), "step": (5, 0, 1), "index": (5, 1, 0), "seed": (6, 0, 0), "seed_hi": (5 + (1 << 32), 0, 0),
    }
    ns = {k: ops.heun_churn(_zeros(shape), 1.0, ops.churn_record(s, i, DEV), st).double().flatten()
          for k, (s, i, st) in draws.items()}
    m = ns["base"].numel()
    for k, v in ns.items():
        assert abs(v.mean().item()) < 5 / math.sqrt(m), k
        assert abs(v.std().item() - 1.0) < 5 / math.sqrt(2 * m), k
        if k != "base":
            corr = torch.corrcoef(torch.stack([ns["base"], v]))[0, 1].item()
            assert abs(corr) < 0.02, (k, corr)
    # the samples of one batch are uncorrelated with each other too
    per = ns["base"].view(8, -1)
    assert abs(torch.corrcoef(per[:2])[0, 1].item()) < 0.05


def test_churn_nonfinite_sets_health(ops):
    rec = ops.churn_record(1, 0, DEV)
    ops.check_health(DEV, "before")
    x = torch.zeros(7, 3, 32, 32, device=DEV)
    x[3, 1, 5, 17] = float("nan")           # the dwordx4 body
    ops.heun_churn(x, 1.0, rec, 0)
    with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
        ops.check_health(x.device, "heun_churn vec")
    x = torch.zeros(5, 3, 7, 9, device=DEV)
    x[4, 2, 6, 8] = float("nan")             # the last element of the scalar path's partial quad
    ops.heun_churn(x, 1.0, rec, 0)
    with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
        ops.check_health(x.device, "heun_churn scalar")
    ops.check_health(DEV, "after")


def test_churn_rejects_bad_operands(ops):
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    rec = ops.churn_record(0, 0, DEV)
    with pytest.raises(TypeError):
        ops.heun_churn(x.double(), 1.0, rec, 0)
    with pytest.raises(ValueError, match="contiguous"):
        ops.heun_churn(x.transpose(2, 3), 1.0, rec, 0)
    with pytest.raises(ValueError, match="rec"):
        ops.heun_churn(x, 1.0, torch.zeros(3, dtype=torch.int32, device=DEV), 0)
    with pytest.raises(TypeError):
        ops.heun_churn(x, 1.0, torch.zeros(4, dtype=torch.int64, device=DEV), 0)
    with pytest.raises(RuntimeError):
        ops.heun_churn(x, 1.0, torch.zeros(4, dtype=torch.int32), 0)
    with pytest.raises(ValueError, match="finite"):
        ops.heun_churn(x, math.inf, rec, 0)
    with pytest.raises(ValueError, match="step"):
        ops.heun_churn(x, 1.0, rec, -1)
    with pytest.raises(ValueError):
        ops.heun_churn(torch.zeros(4, device=DEV), 1.0, rec, 0)
    with pytest.raises(RuntimeError):
        ops.churn_record(0, 0, out=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="rec"):
        ops.churn_record(0, 0, out=torch.zeros(2, dtype=torch.int32, device=DEV))


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
        Pg, eg, dg, w, (lo, hi) = guide
        if not lo < float(s) <= hi:
            return Dm
        gl = labels if eg.num_classes is not None else None
        Dg = O.edm_forward(Pg, eg, dg, x, sig, gl, bf16=bf16).float()
        return Dg + w * (Dm - Dg)
    return D


def _oracle_stochastic(ops, sol, D, x0, labels, solve_index):
    """Algorithm 2 on the CPU, with the noise the GPU kernel draws for (sol.seed, solve_index, step)"""
    t = sol.t_steps
    s = sol.churn_schedule()
    rec = ops.churn_record(sol.seed, solve_index, DEV)
    N = sol.num_steps
    x1 = x0.float() * t[0]
    for i in range(N):
        x = x1
        t0, t1 = t[i], t[i + 1]
        if s.gamma[i] > 0:
            n = ops.heun_churn(torch.zeros(x0.shape, device=DEV), 1.0, rec, i).cpu()
            x = x + s.c[i] * n
            t0 = s.t_hat[i]
        dx = (x - D(x, t0, labels)) / t0
        x1 = x + (t1 - t0) * dx
        if i < N - 1:
            dxp = (x1 - D(x1, t1, labels)) / t1
            x1 = x + (t1 - t0) * (0.5 * dx + 0.5 * dxp)
    return x1


@pytest.mark.parametrize("case", ["all_bf16", "all_f32", "window_bf16", "cfg_interval_bf16"])
def test_stochastic_trajectory_vs_oracle(ops, case):
    import tinyedm_amd as T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    em, dm = tiny_cfgs(10)
    Pm = O.init_params(em, dm, torch.Generator().manual_seed(7))
    bf16 = not case.endswith("f32")
    dtype = "bf16" if bf16 else "f32"
    main = _edm(Pm, em, dm, dtype)
    kw = dict(num_steps=6, sigma_min=0.01, sigma_max=20.0, rho=5.0)
    churn = dict(S_churn=30.0, seed=1234)
    guide_or = None
    if case == "window_bf16":
        churn.update(S_min=0.5, S_max=8.0)
    if case.startswith("cfg"):
        eg, dg = tiny_cfgs(None)
        Pg = O.init_params(eg, dg, torch.Generator().manual_seed(11))
        interval = (0.2, 7.0)
        kw.update(guide=_edm(Pg, eg, dg, dtype), guidance=2.0, guidance_interval=interval)
        guide_or = (Pg, eg, dg, 2.0, interval)
    sol = T.StochasticSolver(**kw, **churn)
    churned = int((sol.churn_schedule().gamma > 0).sum())
    if case == "window_bf16":
        assert 0 < churned < 6
    else:
        assert churned == 6
    if guide_or is not None:
        flags = sol.guided_evaluations()
        assert any(flags) and not all(flags)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 3, 8, 8, generator=g)
    labels = torch.randint(0, 10, (2,), generator=g)
    sol.solve_index = 5
    x_hip = sol.solve(main, x0.to(DEV), labels.to(DEV)).cpu()
    assert sol.solve_index == 6
    with torch.no_grad():
        x_or = _oracle_stochastic(ops, sol, _oracle_D(Pm, em, dm, bf16, guide_or), x0, labels, 5)
    e = rel(x_hip, x_or)
    lim = (1e-2 if bf16 else 2e-4) * (3 if guide_or is not None else 1)
    record(f"stochastic/{case}_trajectory_vs_{'bf16' if bf16 else 'fp32'}_oracle", e, lim)
    assert e <= lim, e
    # the churn must matter at this size: the deterministic solve is far from the stochastic oracle
    det_kw = {k: v for k, v in kw.items()}
    x_det = T.DeterministicSolver(**det_kw).solve(main, x0.to(DEV), labels.to(DEV)).cpu()
    assert rel(x_det, x_or) > 5 * e


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


SCHED = dict(num_steps=6, sigma_min=0.01, sigma_max=20.0, rho=5.0)


def _solver(**kw):
    import tinyedm_amd as T
    return T.StochasticSolver(**SCHED, **kw)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_zero_churn_is_the_deterministic_solve(pair, graph):
    import tinyedm_amd as T
    main, _, x0, labels = pair
    sol = _solver(S_churn=0.0, S_min=0.5, S_max=8.0, S_noise=1.003, seed=99)
    x_s = sol.solve(main, x0, labels, graph=graph)
    det = T.DeterministicSolver(**SCHED)
    assert torch.equal(x_s, det.solve(main, x0, labels, graph=graph))
    if graph:
        assert len(sol._graphs[main]) == 1
        # the same cache key as the deterministic solver's
        assert list(sol._graphs[main]) == list(det._graphs[main])


def test_zero_noise_ignores_the_seed(ops, pair):
    main, _, x0, labels = pair
    x = torch.randn(3, 3, 8, 8, generator=torch.Generator().manual_seed(8)).to(DEV)
    assert torch.equal(ops.heun_churn(x, 0.0, ops.churn_record(7, 0, DEV), 3), x)
    a = _solver(S_churn=30.0, S_noise=0.0, seed=1).solve(main, x0, labels)
    b = _solver(S_churn=30.0, S_noise=0.0, seed=2).solve(main, x0, labels)
    assert torch.equal(a, b)


def test_seed_and_solve_index_reproduce(pair):
    main, _, x0, labels = pair
    s1, s2 = _solver(S_churn=30.0, seed=17), _solver(S_churn=30.0, seed=17)
    a = [s1.solve(main, x0, labels) for _ in range(3)]
    b = [s2.solve(main, x0, labels) for _ in range(3)]
    assert s1.solve_index == s2.solve_index == 3
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2])
    s1.solve_index = 1
    assert torch.equal(s1.solve(main, x0, labels), a[1])
    other = _solver(S_churn=30.0, seed=18).solve(main, x0, labels)
    assert rel(other, a[0]) > 1e-3


def test_stochastic_hipgraph_replay_and_cache_key(pair):
    main, _, x0, labels = pair
    sol = _solver(S_churn=30.0, seed=3)
    eager = [sol.solve(main, x0, labels) for _ in range(2)]
    sol.solve_index = 0
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager[0])       # capture
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager[1])       # pure replay, next index
    assert len(sol._graphs[main]) == 1
    # a new seed is a device value: the same graph, new noise
    sol.seed, sol.solve_index = 4, 0
    e4 = sol.solve(main, x0, labels)
    sol.solve_index = 0
    r4 = sol.solve(main, x0, labels, graph=True)
    assert torch.equal(r4, e4) and not torch.equal(r4, eager[0])
    assert len(sol._graphs[main]) == 1
    # a new S_churn, then a window: new schedules, new captures
    sol.S_churn = 1.2                   # gamma 0.2: below the sqrt(2) - 1 cap that S_churn = 30 hits at N = 6
    sol.solve_index = 0
    e = sol.solve(main, x0, labels)
    sol.solve_index = 0
    assert torch.equal(sol.solve(main, x0, labels, graph=True), e)
    assert len(sol._graphs[main]) == 2
    sol.S_min, sol.S_max = 0.5, 8.0
    sol.solve_index = 0
    e = sol.solve(main, x0, labels)
    sol.solve_index = 0
    assert torch.equal(sol.solve(main, x0, labels, graph=True), e)
    assert len(sol._graphs[main]) == 3


def test_guided_stochastic_hipgraph_replay(pair):
    main, guide, x0, labels = pair
    sol = _solver(guide=guide, guidance=2.0, guidance_interval=(0.2, 7.0), S_churn=30.0, seed=5)
    eager = [sol.solve(main, x0, labels) for _ in range(2)]
    sol.solve_index = 0
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager[0])
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager[1])
    assert len(sol._graphs[main]) == 1


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


def test_generate_cli_churn(ops, tmp_path):
    from PIL import Image
    _generate(tmp_path / "plain")
    plain = _pngs(tmp_path / "plain")
    assert sorted(plain) == [f"{i}.png" for i in range(4)]
    _generate(tmp_path / "zero", "--S_churn", "0")
    assert _pngs(tmp_path / "zero") == plain
    churn = ("--S_churn", "40", "--S_min", "0.05", "--S_max", "50")
    _generate(tmp_path / "c0", *churn)
    c0 = _pngs(tmp_path / "c0")
    assert sorted(c0) == sorted(plain)
    for f in c0:
        assert Image.open(tmp_path / "c0" / f).size == (32, 32)
    assert all(c0[f] != plain[f] for f in c0)
    _generate(tmp_path / "c0b", *churn)
    assert _pngs(tmp_path / "c0b") == c0
    _generate(tmp_path / "c1", *churn, "--seed", "1")
    c1 = _pngs(tmp_path / "c1")
    assert all(c1[f] != c0[f] for f in c1)
