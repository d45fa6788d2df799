"""Optimised sampling schedules on the GPU (csrc/schedule.hip, ops.pair_step_errors, DeterministicSolver.trace, the
sigmas= argument of the table solvers, tinyedm_amd/schedule.py and the two command lines):

 * pair_step_errors on exact operands, bit for bit; on random fp32 operands against the fp64 reference under a bound from
   the rounding count; its invariances (the batch, a sub-grid, the load path), bit for bit; the edges of G;
 * trace against solve, scale_f32 and heun_euler, bit for bit, on an analytic callable and on a tiny net, one guided;
 * a caller's Karras table reproduces the default constructor for all four table solvers, eager and captured;
 * Heun on a table that is no Karras table against the reference's Heun;
 * optimize_schedule end to end on the analytic Gaussian denoiser; the command lines on a tiny checkpoint."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import schedule_ref as R
from parity_log import record
from test_adaptive_solver_gpu import _gaussian_gpu, _tiny_case
from test_multistep_solver_gpu import _edm

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
EPS32 = 2.0 ** -24
SCHED = dict(num_steps=6, sigma_min=0.01, sigma_max=20.0, rho=5.0)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _give_the_block_counter_back():
    """Every residual block takes its dropout sub-stream from a process-wide counter (networks._rng_sub_counter), so the
    masks of a network built later in the session depend on how many blocks were built before it.  The tiny nets of this
    file are evaluation-only: put the counter back, and the tests that follow see the streams they see without this file."""
    from tinyedm_amd import networks
    before = networks._rng_sub_counter[0]
    yield
    networks._rng_sub_counter[0] = before


def _dev(a, offset=0):
    """a host array as a contiguous fp32 device tensor whose first element lies ``offset`` floats past a 16-byte boundary"""
    a = torch.as_tensor(np.asarray(a, dtype=np.float32))
    buf = torch.empty(a.numel() + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + a.numel()].view(a.shape)
    view.copy_(a)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * offset
    return view


def _tau(t):
    return torch.as_tensor(np.asarray(t, dtype=np.float64)).to(DEV)


def _bound(X, S, tau, order, K):
    """|d2 - ref| <= 2 (K + 8) 2^-53 sum_k m_k^2, m_k = |x_i| + |c h| (|s_i| [+ |s_j|]) + |x_j| (c = 1/2 for the trapezoid).
    The kernel forms e = fma(c h, s_i + s_j, x_i - x_j) in fp64: the two differences of fp32 values (exact, or one rounding
    when their exponents lie more than 29 bits apart), h (one rounding, shared with the reference) and the fma: <= 3 u m.
    The reference forms x_i + h s_i - x_j, or x_i + (h/2)(s_i + s_j) - x_j: <= 4 roundings, each <= u m.  So the two e
    differ by <= 7 u m and, |e| <= m, their squares by <= 14 u m^2 (to first order); each side rounds the square once
    (u m^2) and adds K terms in some order (<= (K - 1) u sum m^2 each): (14 + 2 + 2 (K - 1)) u sum m^2 = 2 (K + 7) u sum m^2,
    taken as 2 (K + 8) for the second-order terms."""
    return 2.0 * (K + 8) * U64 * R.pair_step_magnitudes(X, S, tau, order)


def _lower_is_plus_zero(d2):
    G = d2.shape[1]
    low = d2[:, np.tril_indices(G, 0, G + 1)[0], np.tril_indices(G, 0, G + 1)[1]]
    return bool((low == 0.0).all()) and not bool(np.signbit(low).any())


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("K", [1, 5, 192, 1024, 4099])
def test_pair_step_errors_exact(ops, K, order, offset):
    """integers in [-8, 8] and tau = (8, 4, 2, 1, 1/2, 0): e is a multiple of 1/4 with |e| <= 80 and 4099 * 6400 * 16 < 2^53,
    so every product and sum is exact in fp64 and d2 is one defined number whatever the order of the sum"""
    rng = np.random.default_rng(1000 * K + 10 * order + offset)
    tau = np.array([8.0, 4.0, 2.0, 1.0, 0.5, 0.0])
    G, B = 5, 3
    X = rng.integers(-8, 9, (G + 1, B, K)).astype(np.float32)
    S = rng.integers(-8, 9, (G, B, K)).astype(np.float32)
    got = ops.pair_step_errors(_dev(X, offset), _dev(S, offset), _tau(tau), order)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, G, G + 1) and got.is_contiguous()
    got = got.cpu().numpy()
    assert np.array_equal(got, R.pair_step_errors(X, S, tau, order))
    assert _lower_is_plus_zero(got)


def _trajectory_like(G, B, K, seed, table=None):
    """operands scaled as a real trajectory: node i is about tau_i in size, slopes about 1"""
    import tinyedm_amd as T
    g = torch.Generator().manual_seed(seed)
    tau = (T.DeterministicSolver(num_steps=G).t_steps if table is None else table).double().numpy()
    scale = torch.from_numpy(np.sqrt(tau ** 2 + 0.25)).float()[:, None, None]
    X = (torch.randn(G + 1, B, K, generator=g) * scale).numpy()
    S = torch.randn(G, B, K, generator=g).numpy()
    return X, S, tau


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("G,B,K,offset", [(3, 2, 5, 0), (9, 3, 4099, 0), (12, 2, 3072, 0), (12, 2, 3072, 1), (18, 1, 772, 0)],
                         ids=["G3-K5", "G9-K4099-tail", "G12-K3072", "G12-K3072-misaligned", "G18-K772"])
def test_pair_step_errors_vs_fp64(ops, G, B, K, offset, order):
    X, S, tau = _trajectory_like(G, B, K, 7 * G + K + order)
    got = ops.pair_step_errors(_dev(X, offset), _dev(S, offset), _tau(tau), order).cpu().numpy()
    ref, bound = R.pair_step_errors(X, S, tau, order), _bound(X, S, tau, order, K)
    up = np.triu_indices(G, 1, G + 1)
    err, room = np.abs(got - ref)[:, up[0], up[1]], bound[:, up[0], up[1]]
    worst = float((err / room).max())
    print(f"G {G} K {K} order {order}: worst |d2 - ref| / bound = {worst:.3g}; smallest d2 / largest = "
          f"{ref[:, up[0], up[1]].min() / ref.max():.3g}")
    record(f"schedule/pair_errors_G{G}_K{K}_o{order}_off{offset}", worst, 1.0)
    assert (err <= room).all(), worst
    assert _lower_is_plus_zero(got)


@pytest.mark.parametrize("order", [1, 2])
def test_pair_step_errors_invariances(ops, order):
    G, B, K = 8, 5, 2052            # (513 quads: the threads hold one to three each)
    X, S, tau = _trajectory_like(G, B, K, 31 + order)
    Xd, Sd, td = _dev(X), _dev(S), _tau(tau)
    full = ops.pair_step_errors(Xd, Sd, td, order)
    # the batch: row b of the B = 5 call is the B = 1 call on that sample
    for b in range(B):
        alone = ops.pair_step_errors(Xd[:, b:b + 1].contiguous(), Sd[:, b:b + 1].contiguous(), td, order)
        assert torch.equal(alone[0], full[b])
    # the grid: the nodes 0, 2, 4, .. as a grid of their own (other tiles, other places in a tile, another end row)
    sub = ops.pair_step_errors(Xd[::2].contiguous(), Sd[::2].contiguous(), td[::2].contiguous(), order)
    assert tuple(sub.shape) == (B, G // 2, G // 2 + 1)
    # (the step onto the end is Euler in both calls; a trapezoid step reads the slope of its target, a node of both)
    assert torch.equal(sub, full[:, ::2, ::2])
    # the load path
    assert torch.equal(ops.pair_step_errors(_dev(X, 1), _dev(S, 1), td, order), full)
    assert torch.equal(ops.pair_step_errors(_dev(X, 3), _dev(S, 2), td, order), full)
    # the other order differs (the test would notice an ignored argument)
    assert not torch.equal(ops.pair_step_errors(Xd, Sd, td, 3 - order), full)


@pytest.mark.parametrize("G,K", [(1, 7), (2, 4), (256, 4)], ids=["G1", "G2", "G256-K4"])
def test_pair_step_errors_edges(ops, G, K):
    import tinyedm_amd as T
    assert ops.SCHEDULE_MAX_GRID == 256
    B = 2
    table = torch.cat([torch.tensor([3.0]), torch.zeros(1)]) if G == 1 else T.DeterministicSolver(num_steps=G).t_steps
    X, S, tau = _trajectory_like(G, B, K, G, table)
    for order in (1, 2):
        got = ops.pair_step_errors(_dev(X), _dev(S), _tau(tau), order).cpu().numpy()
        assert got.shape == (B, G, G + 1) and _lower_is_plus_zero(got)
        assert (np.abs(got - R.pair_step_errors(X, S, tau, order)) <= _bound(X, S, tau, order, K)).all()
    if G == 1:      # one node and the end: the one entry is the Euler jump to 0, in both orders
        assert got[0, 0, 1] > 0.0 and np.array_equal(got, ops.pair_step_errors(_dev(X), _dev(S), _tau(tau), 1).cpu().numpy())


def test_pair_step_errors_misuse(ops):
    from tinyedm_amd import _lib
    X, S, tau = _trajectory_like(3, 2, 8, 5)
    Xd, Sd, td = _dev(X), _dev(S), _tau(tau)
    for args, match in (((Xd, Sd, td, 3), "order"), ((Xd, Sd[:2].contiguous(), td, 2), "S"), ((Xd, Sd, td[:3].contiguous(), 2), "tau"),
                        ((Xd, Sd, td.float(), 2), "tau"), ((Xd.double(), Sd, td, 2), "X"), ((Xd[:1], Sd, td, 2), "X")):
        with pytest.raises(ValueError, match=match):
            ops.pair_step_errors(*args)
    big = torch.zeros(258, 1, 1, device=DEV)
    with pytest.raises(ValueError, match="at most 256"):
        ops.pair_step_errors(big, big[:257], torch.zeros(258, dtype=torch.float64, device=DEV), 1)
    # the entry point itself: a negative status before any launch
    d2 = torch.zeros(2, 3, 4, dtype=torch.float64, device=DEV)
    fn = _lib.lib().edm_pair_step_errors
    good = (Xd.data_ptr(), Sd.data_ptr(), td.data_ptr(), 2, 3, 8, 2, d2.data_ptr(), None)
    for k, v in ((6, 3), (6, 0), (4, 0), (4, 257), (3, 0), (5, 0), (0, None), (7, None)):
        bad = list(good)
        bad[k] = v
        assert fn(*bad) < 0
    torch.cuda.synchronize()
    assert bool((d2 == 0).all())


# ------------------------------------------------------------------ the recorder
@torch.no_grad()
def _check_trace(ops, sol, model, x0, labels, guide=None):
    tr = sol.trace(model, x0, labels)
    N = sol.num_steps
    assert tr.x.shape == (N + 1, *x0.shape) and tr.slope.shape == (N, *x0.shape)
    assert tr.x.dtype == tr.slope.dtype == torch.float32 and tr.x.is_contiguous() and tr.slope.is_contiguous()
    assert torch.equal(tr.sigmas, sol.t_steps) and not tr.sigmas.is_cuda
    assert torch.equal(tr.x[N], sol.solve(model, x0, labels))
    assert torch.equal(tr.x[0], ops.scale_f32(x0.float().contiguous(), sol.t_steps[0].item()))
    ts, t_dev = sol.t_steps.tolist(), sol.t_steps.to(DEV)
    flags = sol.guided_evaluations()
    w_dev = torch.full((1,), float(sol.guidance), device=DEV)
    for i in range(N):
        D = model(tr.x[i], t_dev[i], labels).float().contiguous()
        if flags[2 * i]:
            Dg = guide(tr.x[i], t_dev[i], labels).float().contiguous()
            dx = ops.heun_euler_guided(tr.x[i], D, Dg, w_dev, ts[i], ts[i + 1])[0]
        else:
            dx = ops.heun_euler(tr.x[i], D, ts[i], ts[i + 1])[0]
        assert torch.equal(tr.slope[i], dx), i
    return tr


def test_trace_on_the_gaussian_callable(ops):
    import tinyedm_amd as T
    _, x0 = R.setting()
    x0 = torch.from_numpy(x0).float().to(DEV)
    _check_trace(ops, T.DeterministicSolver(num_steps=7), _gaussian_gpu, x0, None)
    # an unchurned StochasticSolver is the same solve
    tr = T.StochasticSolver(num_steps=7).trace(_gaussian_gpu, x0)
    assert torch.equal(tr.x, T.DeterministicSolver(num_steps=7).trace(_gaussian_gpu, x0).x)


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "cfg-w2"])
def test_trace_on_a_tiny_net(ops, guided):
    import tinyedm_amd as T
    (Pm, em, dm), guide, x0, labels = _tiny_case(guided)
    main = _edm(Pm, em, dm, "f32")
    g_net = _edm(guide[0], guide[1], guide[2], "f32") if guided else None
    x0, labels = x0.to(DEV), labels.to(DEV)
    kw = dict(guide=g_net, guidance=2.0, guidance_interval=(0.05, 5.0)) if guided else {}
    sol = T.DeterministicSolver(**SCHED, **kw)
    if guided:
        assert 0 < sum(sol.guided_evaluations()) < 11        # the interval is honoured: both kinds of step are checked
    _check_trace(ops, sol, main, x0, labels, g_net)
    ops.check_health(DEV, "trace")


# ------------------------------------------------------------------ a caller's table
@pytest.mark.parametrize("name", ["heun", "churn", "dpmpp", "picard"])
def test_explicit_karras_table_reproduces_the_default(ops, name):
    import tinyedm_amd as T
    (Pm, em, dm), _, x0, labels = _tiny_case(False)
    main = _edm(Pm, em, dm, "f32")
    x0, labels = x0.to(DEV), labels.to(DEV)
    cls, kw = {"heun": (T.DeterministicSolver, {}), "churn": (T.StochasticSolver, dict(S_churn=3.0, seed=5)),
               "dpmpp": (T.MultistepSolver, dict(order=2)),
               "picard": (T.ParallelSolver, dict(window=3, rtol=1e-2, atol=1e-3))}[name]
    table = cls(**SCHED, **kw).t_steps[:-1]
    for graph in (False, True):
        a, b = cls(**SCHED, **kw), cls(sigmas=table, **kw)      # (fresh: a churned solve draws from its solve index)
        assert torch.equal(a.t_steps, b.t_steps) and b.rho is None
        out_a, out_b = a.solve(main, x0, labels, graph=graph), b.solve(main, x0, labels, graph=graph)
        assert torch.equal(out_a, out_b) and bool(torch.isfinite(out_a).all())
    ops.check_health(DEV, "sigmas=")


def test_heun_on_a_table_that_is_no_karras_table(ops):
    """a geometric table, 80 -> 0.002 in 12 levels, on the analytic Gaussian denoiser against the reference's fp64 Heun on
    the same fp32 levels.  The denoiser is linear in x, so a relative perturbation of the state is carried through every
    later step unchanged; a step perturbs the state by the roundings of its two evaluations (1 each, the fp64 value cast
    to fp32), of the Euler stage (x - D, / t0, t1 - t0, the fma: 4) and of the correction (x1 - D1, / t1, the two halves
    and their sum, the fma: 6), the slopes weighted by |dt| / t1 = (1 - r) / r = 1.6 at most for the ratio r = 0.38 of this
    table: under 12 * 1.6 < 24 roundings of eps32 / 2 relative to the state, taken as 24 eps32 per step."""
    import tinyedm_amd as T
    N = 12
    table = torch.tensor(np.geomspace(80.0, 0.002, N), dtype=torch.float32)
    _, x0 = R.setting()
    sol = T.DeterministicSolver(sigmas=table)
    out = sol.solve(_gaussian_gpu, torch.from_numpy(x0).float().to(DEV)).double().cpu().numpy()
    ref = R.heun_solve(R.gaussian, x0.astype(np.float32).astype(np.float64), table.double().numpy())
    err = np.linalg.norm(out - ref, axis=1) / np.linalg.norm(ref, axis=1)
    print(f"geometric table: worst relative error {err.max():.3g}, bound {24 * N * EPS32:.3g}")
    record("schedule/heun_geometric_table", float(err.max()), 24 * N * EPS32)
    assert (err <= 24 * N * EPS32).all(), err.max()
    # and the table matters: the Karras table of the same ends gives another image
    assert not np.allclose(out, T.DeterministicSolver(num_steps=N).solve(
        _gaussian_gpu, torch.from_numpy(x0).float().to(DEV)).double().cpu().numpy(), rtol=1e-3, atol=0)


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("grid", [32, 33], ids=["grid32", "grid33-has-even-paths"])
def test_optimize_schedule_on_the_gaussian_callable(ops, grid):
    import tinyedm_amd as T
    from tinyedm_amd import schedule
    kw = dict(shape=(R.D_,), grid=grid, warmup=8, order=2, seed=4, device=torch.device(DEV), return_costs=True)
    found, cost = schedule.optimize_schedule(_gaussian_gpu, [5, 9], batch_size=3, **kw)
    teacher = T.DeterministicSolver(num_steps=grid)
    assert cost.shape == (grid, grid + 1) and cost.dtype == np.float64
    assert np.isinf(cost[np.tril_indices(grid, 0, grid + 1)]).all() and np.isfinite(cost[np.triu_indices(grid, 1, grid + 1)]).all()
    for s, N in zip(found, (5, 9)):
        idx, total = R.best_path(cost, N)
        assert s.indices == list(idx) and s.cost == total and s.num_steps == N
        assert s.sigmas == teacher.t_steps[idx].tolist() and (s.order, s.grid, s.warmup, s.seed) == (2, grid, 8, 4)
        even = R.even_path(grid, N)
        if even is None:        # (31 is prime: a 32-node grid holds no evenly spaced 5- or 9-step path)
            assert s.karras_cost is None
        else:
            assert s.karras_cost == R.path_cost(cost, even) and s.cost <= s.karras_cost
        T.DeterministicSolver(sigmas=s.sigmas)
    assert (grid == 33) == all(s.karras_cost is not None for s in found)
    # one chunk of 8 gives the bits of chunks of 3
    once, cost8 = schedule.optimize_schedule(_gaussian_gpu, 5, batch_size=8, **kw)
    assert np.array_equal(cost8, cost) and once == found[0]
    # step_costs on the recorded trajectory, chunked or not, and the kernel against the reference on that trajectory
    x0 = torch.randn((8, R.D_), generator=torch.Generator().manual_seed(4), dtype=torch.float32).to(DEV)
    tr = teacher.trace(_gaussian_gpu, x0)
    assert np.array_equal(schedule.step_costs(tr), cost) and np.array_equal(schedule.step_costs(tr, batch_size=3), cost)
    X, S, tau = tr.x.cpu().numpy(), tr.slope.cpu().numpy(), tr.sigmas.double().numpy()
    for order in (1, 2):
        d2 = ops.pair_step_errors(tr.x, tr.slope, tr.sigmas.double().to(DEV), order).cpu().numpy()
        assert (np.abs(d2 - R.pair_step_errors(X, S, tau, order)) <= _bound(X, S, tau, order, R.D_)).all()
        assert np.array_equal(schedule.step_costs(tr, order), R.step_costs(d2))


def test_the_command_lines(ops, tmp_path):
    """python -m tinyedm.schedule on a tiny checkpoint writes the file python -m tinyedm.generate --sigma_table samples with;
    the images are those of a direct solve with sigmas= of that file"""
    from PIL import Image
    import tinyedm_amd as T
    from tinyedm_amd import schedule
    from tinyedm_amd.callbacks import PreditionWriter
    from tinyedm_amd.datamodules import RandomNoiseDataModule
    from tinyedm_amd.generate import CIFAR_MEAN, CIFAR_STD
    (Pm, em, dm), _, _, _ = _tiny_case(False)
    model = _edm(Pm, em, dm, "f32")
    ckpt, table = str(tmp_path / "tiny.ckpt"), str(tmp_path / "schedule.json")
    torch.save({"hyper_parameters": dict(model.hparams), "state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, ckpt)
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "-m", "tinyedm.schedule", "--ckpt_path", ckpt, "--num_steps", "4", "6", "--grid", "11",
                        "--warmup", "4", "--batch_size", "3", "--image_size", "8", "--network_dtype", "f32", "--seed", "2",
                        "--out", table], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    found = schedule.load_schedules(table)
    assert sorted(found) == [4, 6] and all(s.grid == 11 and s.warmup == 4 and s.order == 2 for s in found.values())
    assert found[6].karras_cost is not None and found[6].cost <= found[6].karras_cost and found[4].karras_cost is None
    for N in (4, 6):
        assert f"N = {N}: cost" in r.stdout and "Karras cost" in r.stdout
    out = tmp_path / "out"
    common = ["--output_dir", str(out), "--num_samples", "4", "--image_size", "8", "--num_classes", "10", "--batch_size", "4",
              "--num_workers", "0", "--network_dtype", "f32", "--seed", "3", "--sigma_table", table]
    r = subprocess.run([sys.executable, "-m", "tinyedm.generate", "--ckpt_path", ckpt, "--num_steps", "6", *common],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    # the same images from a direct solve on the file's table
    model.solver = T.DeterministicSolver(sigmas=found[6].sigmas, seed=3)
    batch = next(iter(RandomNoiseDataModule(4, 0, 8, 4, 10, in_channels=3, seed=3).predict_dataloader()))
    direct = tmp_path / "direct"
    PreditionWriter(str(direct), "batch", CIFAR_MEAN, CIFAR_STD).write_on_batch_end(
        None, model, model.predict_step(batch, 0), None, None, 0, 0)
    for i in range(4):
        a, b = np.asarray(Image.open(out / f"{i}.png")), np.asarray(Image.open(direct / f"{i}.png"))
        assert a.shape == (8, 8, 3) and np.array_equal(a, b), i
    json.loads(open(table).read())
