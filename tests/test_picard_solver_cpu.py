"""The parallel-in-time solver, host side (no GPU): the numpy restatement tests/picard_ref.py is put to the test on the
analytic denoisers of tests/test_adaptive_solver_cpu.py (d = 48, B = 8, the 18-step table), so that every condition
tests/test_picard_solver_gpu.py leans on is checked here; then the stride rule on hand-made rows, the host validation of
ParallelSolver and of the generate flags, and the C ABI declarations."""
import math
import os
import re

import numpy as np
import pytest
import torch

import picard_ref as R
from test_adaptive_solver_cpu import gaussian, mixture, setting
from tinyedm_amd import DeterministicSolver, ParallelSolver, ParallelStats, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ = 18
TS = DeterministicSolver(num_steps=N_).t_steps.double().numpy()         # the fp32 table values, t_N = 0
WINDOWS = (1, 3, N_ - 1, 64)


@pytest.fixture(scope="module")
def world():
    means, x0 = setting()
    return x0, {"gaussian": gaussian, "mixture": mixture(means)}


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_zero_tolerance_is_the_sequential_solve_exactly(world, name, order):
    x0, dens = world
    seq, seq_min = R.sequential(dens[name], x0, TS, order=order)
    for P in WINDOWS:
        r = R.solve(dens[name], x0, TS, P, order=order, rtol=0.0, atol=0.0)
        assert np.array_equal(r.x_min, seq_min) and np.array_equal(r.x, seq), P
        assert r.iterations <= N_ - 1 and r.iterations == r.per_sample_iterations.max()
        assert r.evaluations == order * r.iterations + 1
        print(f"{name} order {order} window {P}: {r.iterations} iterations to the fixed point")


@pytest.mark.parametrize("order", [1, 2])
def test_window_one_is_the_sequential_loop(world, order):
    x0, dens = world
    for rtol in (0.0, 1e-2):
        r = R.solve(dens["mixture"], x0, TS, 1, order=order, rtol=rtol, atol=rtol / 10)
        assert r.iterations == N_ - 1 and all((s == 1).all() for s in r.strides)
        assert (r.per_sample_iterations == N_ - 1).all()
        assert np.array_equal(r.x, R.sequential(dens["mixture"], x0, TS, order=order)[0])


@pytest.mark.parametrize("P", WINDOWS)
@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_iterations_are_bounded_and_fall_with_the_tolerance(world, name, P):
    x0, dens = world
    its = []
    for rtol in (0.0, 1e-4, 1e-3, 1e-2):
        r = R.solve(dens[name], x0, TS, P, rtol=rtol, atol=rtol / 10)
        assert r.iterations <= N_ - 1
        its.append(r.iterations)
    print(f"{name} window {P}: iterations at rtol 0, 1e-4, 1e-3, 1e-2 = {its}")
    assert its[0] >= its[1] >= its[2] >= its[3], its


def test_every_active_sample_advances(world):
    x0, dens = world
    r = R.solve(dens["mixture"], x0, TS, 5, rtol=1e-3, atol=1e-4)
    s = np.zeros(len(x0), np.int64)
    for stride in r.strides:
        active = s < N_ - 1
        assert (stride[active] >= 1).all() and (stride[~active] == 0).all()
        s += stride
    assert (s == N_ - 1).all()


def test_a_sample_alone_gives_the_bits_of_the_batch(world):
    x0, dens = world
    batch = R.solve(dens["mixture"], x0, TS, 5, rtol=1e-2, atol=1e-3)
    for b in (0, 5):
        alone = R.solve(dens["mixture"], x0[b:b + 1], TS, 5, rtol=1e-2, atol=1e-3)
        assert np.array_equal(alone.x[0], batch.x[b]) and alone.per_sample_iterations[0] == batch.per_sample_iterations[b]


def test_float32_fixed_point_is_the_float32_sequential_solve(world):
    x0, dens = world
    D = lambda x, t: dens["gaussian"](x.astype(np.float64), t).astype(np.float32)       # noqa: E731
    for order in (1, 2):
        seq = R.sequential(D, x0, TS, order=order, dtype=np.float32)[0]
        r = R.solve(D, x0, TS, 5, order=order, rtol=0.0, atol=0.0, dtype=np.float32)
        assert r.x.dtype == np.float32 and np.array_equal(r.x, seq)


# ------------------------------------------------------------------ the stride rule, the slide, the error norm
def test_stride_rule():
    assert R.stride_rule([0.1, 0.5, 1.0, 0.9], 4) == 4             # all converged: the whole live window (m + 1 clamped)
    assert R.stride_rule([0.1, 0.5, 1.0, 0.9, 3.0], 5) == 5         # four converged and the one after them
    assert R.stride_rule([2.0, 0.1, 0.1], 3) == 1                   # none converged: position 1 is still exact
    assert R.stride_rule([0.1, float("nan"), 0.1, 0.1], 4) == 2     # a NaN is not converged
    assert R.stride_rule([0.0, 0.0, 0.0, 0.0, 0.0], 2) == 2         # clamped at the table end: only L live positions
    assert R.stride_rule([float("inf")], 1) == 1
    assert R.stride_rule([], 0) == 0
    # control: start, status and the iteration count
    CHW = 4
    S = np.array([[0.0, 0.0, 0.0], [4.0 * 9, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    stride, s, status, iters, still = R.control(S, CHW, [0, 2, 3, 8, 9], [0, 0, 0, 0, 1], [0, 1, 2, 3, 4], 10, 3)
    assert stride.tolist() == [3, 1, 2, 1, 0] and s.tolist() == [3, 3, 5, 9, 9]
    assert status.tolist() == [0, 0, 0, 1, 1] and iters.tolist() == [1, 2, 3, 4, 4] and still == 3


def test_error_norm_zero_scale():
    old = np.array([[0.0, 1.0, -2.0]], np.float32)
    assert R.error_norm(old, old, 0.0, 0.0)[0] == 0.0
    new = old.copy()
    new[0, 1] = np.nextafter(np.float32(1.0), np.float32(2.0))
    assert R.error_norm(new, old, 0.0, 0.0)[0] == np.inf
    assert R.error_norm(new, old, 1e-4, 1e-3)[0] < 1e-3
    assert R.error_norm(old, old, 0.0, 1e-3)[0] == 0.0              # (the zero element: scale 0, unchanged)


def test_slide_shifts_extrapolates_and_copies():
    N, P, B, d = 6, 3, 3, 4
    ts = np.array([8.0, 4.0, 2.0, 1.0, 0.5, 0.25, 0.0])
    g = np.random.default_rng(0)
    Xnew, D = g.standard_normal((P + 1, B, d)), g.standard_normal((P, B, d))
    s_old, stride = np.array([0, 2, 4]), np.array([2, 3, 1])        # L = 3, 3, 1
    X = R.slide(Xnew, D, stride, s_old, ts, N, P, np.float64)
    assert np.array_equal(X[0, 0], Xnew[2, 0]) and np.array_equal(X[1, 0], Xnew[3, 0])
    for j, i in ((2, 4), (3, 5)):                                   # sample 0: entering at table indices 4 and 5
        assert np.allclose(X[j, 0], D[2, 0] + (Xnew[3, 0] - D[2, 0]) * ts[i] / ts[3])
    assert np.array_equal(X[0, 1], Xnew[3, 1])                      # sample 1: s = 5 = N - 1, everything else is a copy
    assert all(np.array_equal(X[j, 1], Xnew[3, 1]) for j in (1, 2, 3))
    assert all(np.array_equal(X[j, 2], Xnew[1, 2]) for j in range(P + 1))       # sample 2 arrives at N - 1
    T = R.times(s_old + stride, ts, N, P)
    assert T[:, 0].tolist() == [2.0, 1.0, 0.5, 0.25] and T[:, 1].tolist() == [0.25] * 4
    X0 = R.begin(np.ones((2, d)), ts, N, 7, np.float64)
    assert [X0[j, 0, 0] for j in range(8)] == [8.0, 4.0, 2.0, 1.0, 0.5, 0.25, 8.0, 8.0]


# ------------------------------------------------------------------ host validation
def _never(*a, **k):
    raise AssertionError("nothing may be evaluated")


@pytest.mark.parametrize("kw,match", [
    ({"window": 0}, "window"), ({"window": 65}, "window"), ({"window": 2.0}, "window"), ({"window": True}, "window"),
    ({"order": 3}, "order"), ({"order": 0}, "order"), ({"order": True}, "order"),
    ({"rtol": -1e-3}, "rtol"), ({"rtol": math.nan}, "rtol"), ({"atol": math.inf}, "atol"), ({"atol": -1.0}, "atol"),
    ({"rtol": "1e-3"}, "rtol"), ({"num_steps": 1}, "num_steps"), ({"num_steps": 2.0}, "num_steps"),
    ({"guidance": 2.0}, "needs a guide"), ({"guidance": 2.0, "guide": _never, "guidance_interval": (0.1, 5.0)}, "guidance_interval"),
    ({"guidance_interval": (0.1, 5.0)}, "guidance_interval"), ({"dtype": "float64"}, "float32"),
])
def test_invalid_settings_rejected(kw, match):
    with pytest.raises(ValueError, match=match):
        ParallelSolver(**kw)


def test_constructor_and_defaults():
    from tinyedm_amd import AdaptiveSolver
    s = ParallelSolver()
    assert isinstance(s, DeterministicSolver)
    assert (s.window, s.order, s.rtol, s.atol) == (16, 2, AdaptiveSolver().rtol, AdaptiveSolver().atol) == (16, 2, 1e-3, 1e-4)
    assert s.last_stats is None and torch.equal(s.t_steps, DeterministicSolver().t_steps)
    assert ParallelSolver(rtol=0.0, atol=0.0).guided_evaluations() == (False,)         # zero tolerance is legal
    assert ParallelSolver(num_steps=2, window=64).num_steps == 2
    with pytest.raises(TypeError):
        ParallelSolver(18, 0.002, 80.0, 7.0, None, 16)          # window and the rest are keyword-only
    import tinyedm
    assert tinyedm.ParallelSolver is ParallelSolver and tinyedm.solvers.ParallelSolver is ParallelSolver
    assert tinyedm.ParallelStats is ParallelStats and tinyedm.solvers.ParallelStats is ParallelStats
    assert ParallelStats._fields == ("iterations", "evaluations", "guide_evaluations", "rows", "sequential_evaluations",
                                     "per_sample_iterations")
    s.window = 100                                              # plain attributes, checked again at every solve
    with pytest.raises(ValueError, match="window"):
        s.solve(_never, torch.zeros(1, 3, 4, 4))


@pytest.mark.parametrize("kw", [
    {"start_step": 3}, {"image": torch.zeros(1, 3, 4, 4)}, {"mask": torch.ones(4, 4)}, {"degradation": object()},
    {"measurement": torch.zeros(1, 3, 2, 2)}, {"operator": object()}, {"dps_scale": 1.0},
])
def test_solve_refuses_on_the_host(kw):
    # x0 is a host tensor: the refusal comes before the "no CPU path" error, so before any launch
    with pytest.raises(ValueError, match="not implemented for the parallel solver"):
        ParallelSolver().solve(_never, torch.zeros(1, 3, 4, 4), **kw)


def test_invert_likelihood_and_cpu_tensors_refused():
    s = ParallelSolver()
    with pytest.raises(ValueError, match="inversion is not implemented"):
        s.invert(_never, torch.zeros(1, 3, 4, 4))
    with pytest.raises(ValueError, match="likelihood"):
        s.log_likelihood(_never, torch.zeros(1, 3, 4, 4))
    for graph in (False, True):
        with pytest.raises(ValueError, match="no CPU path"):
            s.solve(_never, torch.zeros(1, 3, 4, 4), graph=graph)
    with pytest.raises(ValueError, match="floating-point"):
        s.solve(_never, torch.zeros(1, 3, 4, 4, dtype=torch.int32))


def test_ops_have_no_cpu_path():
    x = torch.zeros(3, 2, 8)
    t = torch.ones(3, 2)
    state = torch.zeros(ops.PICARD_ROWS, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="CPU"):
        ops.picard_begin(x[0], torch.ones(5), 4, 2)
    with pytest.raises(ValueError, match="CPU"):
        ops.picard_scan(x, x[:2], None, None, t, state, 1e-4, 1e-3, N=4)
    with pytest.raises(ValueError, match="CPU"):
        ops.picard_control(torch.zeros(2, 2, 1, dtype=torch.float64), 8, state, 4, 2, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="CPU"):
        ops.picard_slide(x, x[:2], torch.zeros(2, dtype=torch.int32), state, torch.ones(5), N=4)
    with pytest.raises(ValueError, match="window"):
        ops.picard_begin(x[0], torch.ones(5), 4, 65)
    with pytest.raises(ValueError, match="atol"):
        ops.picard_tol(-1.0, 0.0, "cpu")
    assert [ops.picard_chunks(n) for n in (1, 1024, 1025, 3072, 4099, 10 ** 6)] == [1, 1, 2, 3, 5, 64]
    assert ops.PICARD_MAX_WINDOW == 64


GEN = dict(ckpt_path="missing.ckpt", load_ema=False, num_samples=4, image_size=32, num_classes=10, batch_size=4)


@pytest.mark.parametrize("kw,match", [
    ({"guidance_interval": (0.1, 5.0)}, "--guidance_interval"), ({"S_churn": 5.0}, "S_churn"),
    ({"init_dir": "d"}, "--init_dir"), ({"init_dir": "d", "mask_box": (1, 1, 5, 5)}, "--mask_box"),
    ({"init_dir": "d", "restore_scale": 4}, "--restore_scale"), ({"init_dir": "d", "restore_gray": True}, "--restore_scale"),
    ({"init_dir": "d", "dps_scale": 1.0, "blur_std": 1.0}, "--dps_scale"),
    ({"init_dir": "d", "likelihood_to": "o.json"}, "--likelihood_to"), ({"init_dir": "d", "invert_to": "o.pt"}, "--invert_to"),
    ({"init_dir": "d", "start_step": 2}, "--start_step"),
    ({"rtol": -1.0}, "--rtol"), ({"atol": math.nan}, "--atol"), ({"max_iterations": 10}, "--max_iterations"),
    ({"window": 0}, "--window"), ({"window": 65}, "--window"), ({"window": 2.5}, "--window"),
    ({"solver_order": 3}, "--solver_order"),
])
def test_generate_refuses_before_anything_is_loaded(tmp_path, kw, match):
    from tinyedm_amd.generate import generate
    with pytest.raises(ValueError, match=match):
        generate(output_dir=str(tmp_path / "out"), solver="picard", **{**GEN, **kw})
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("solver", ["heun", "dpmpp", "adaptive"])
def test_generate_window_needs_the_picard_solver(tmp_path, solver):
    from tinyedm_amd.generate import generate
    with pytest.raises(ValueError, match="--window needs --solver picard"):
        generate(output_dir=str(tmp_path / "out"), solver=solver, window=4, **GEN)


def test_generate_cli_flags(capsys, tmp_path):
    from tinyedm_amd.generate import _check_picard, _validate, main
    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--window", "--rtol", "--atol", "--solver_report", "--solver_order"):
        assert re.search(rf"(^|\s){flag}(\s|$)", out, re.M), flag
    assert "picard" in out
    args = ["--ckpt_path", "missing.ckpt", "--output_dir", str(tmp_path / "out"), "--num_samples", "4", "--image_size", "32",
            "--num_classes", "10", "--batch_size", "4", "--solver", "picard"]
    with pytest.raises(ValueError, match="S_churn"):
        main(args + ["--S_churn", "5"])
    for extra in (["--solver_order", "3"], ["--window", "0"], ["--guidance_interval", "0.1", "5"]):
        with pytest.raises(SystemExit):
            main(args + extra)
    assert not (tmp_path / "out").exists()
    assert callable(_check_picard)
    # what it accepts: plain and guided, both orders, zero tolerance, the report
    base = dict(solver="picard", S_churn=0.0, init_dir=None, start_step=0, num_steps=18, mask_box=None, invert_to=None,
                likelihood_to=None, network_dtype="f32x3", num_probes=1, dequantize=False, image_size=32, dps_scale=None,
                blur_std=None, blur_radius=2, measurement_noise=0.0, restore_scale=1, restore_gray=False, save_degraded=None,
                restore_report=None, labels_to=None, guided=False)
    assert _validate(**base, rtol=0.0, atol=0.0, window=64, solver_order=1, solver_report="r.json") == (False, False)
    assert _validate(**{**base, "guided": True, "labels_to": "l.json"}, window=1) == (False, False)


def test_picard_declared_in_header_and_lib():
    from tinyedm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    declared = set(re.findall(r"\b(edm_[a-z0-9_]+)\s*\(", hdr))
    for name in ("edm_picard_scan", "edm_picard_control", "edm_picard_slide"):
        assert name in declared and name in _lib.SIGNATURES
    assert int(re.search(r"#define EDM_PICARD_ROWS (\d+)", hdr).group(1)) == ops.PICARD_ROWS
    assert int(re.search(r"#define EDM_PICARD_MAX_WINDOW (\d+)", hdr).group(1)) == ops.PICARD_MAX_WINDOW
