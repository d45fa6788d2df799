"""Optimised sampling schedules on the host (tinyedm_amd/schedule.py, the sigmas= argument of the table solvers, the
--sigma_table flag of generate): the dynamic programme against brute force, its ties and edges, caller's tables and their
refusals, the method itself on the two analytic denoisers through the fp64 reference (tests/schedule_ref.py), the
validator, the C ABI and the JSON file.

The method, measured by test_optimised_table_beats_karras_on_analytic_denoisers (ratio = rms error of the N-step Heun
solve on the optimised table / on the Karras table, truth = Heun on the 257-point Karras table, 64-step grid, order 2):
gaussian N = 9: 0.252, gaussian N = 17: 0.275, mixture N = 9: 0.747.  Mixture N = 5 is WORSE (1.57) and is not asserted:
a sum of local errors is not the global error."""
import math
import os
import re

import numpy as np
import pytest
import torch

import schedule_ref as R
from tinyedm_amd import (AdaptiveSolver, DeterministicSolver, MultistepSolver, ParallelSolver, StochasticSolver, schedule)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 64


def _random_costs(G, seed):
    cost = np.random.default_rng(seed).uniform(0.1, 1.0, (G, G + 1))
    cost[np.tril_indices(G, 0, G + 1)] = np.inf
    return cost


# ------------------------------------------------------------------ the path
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("N", range(2, 10))
def test_best_path_is_optimal(N, seed):
    cost = _random_costs(9, seed)
    best, paths = R.brute_force(cost, N)
    for fn in (schedule.best_path, R.best_path):
        idx, total = fn(cost, N)
        assert len(idx) == N and idx[0] == 0 and idx[-1] == 8 and all(a < b for a, b in zip(idx[:-1], idx[1:]))
        assert total == best and list(idx) in paths and total == R.path_cost(cost, idx)
    assert list(schedule.best_path(cost, N)[0]) == list(R.best_path(cost, N)[0])


def test_best_path_ties_go_to_the_smaller_index():
    G = 5
    cost = np.full((G, G + 1), 4.0)
    cost[np.tril_indices(G, 0, G + 1)] = np.inf
    # 0 -> k -> 4 costs 2 for k = 1, 2, 3 alike (exact in fp64): the smaller predecessor wins
    for k in (1, 2, 3):
        cost[0, k] = cost[k, 4] = 1.0
    for fn in (schedule.best_path, R.best_path):
        idx, total = fn(cost, 3)
        assert list(idx) == [0, 1, 4] and total == 2.0 + cost[4, 5]
    # ... at every stage: with all costs equal the path hugs the start
    flat = np.where(np.isfinite(cost), 1.0, np.inf)
    for fn in (schedule.best_path, R.best_path):
        assert list(fn(flat, 3)[0]) == [0, 1, 4] and list(fn(flat, 4)[0]) == [0, 1, 2, 4]


def test_best_path_edges():
    cost = _random_costs(7, 5)
    for fn in (schedule.best_path, R.best_path):
        idx, total = fn(cost, 7)
        assert list(idx) == list(range(7)) and total == R.path_cost(cost, list(range(7)))
        idx, total = fn(cost, 2)
        assert list(idx) == [0, 6] and total == cost[0, 6] + cost[6, 7]
        for bad in (8, 1, 0):
            with pytest.raises(ValueError):
                fn(cost, bad)
    with pytest.raises(ValueError, match=r"\[G, G \+ 1\]"):
        schedule.best_path(np.zeros((4, 4)), 2)
    with pytest.raises(ValueError, match="num_steps"):
        schedule.best_path(cost, 2.5)


# ------------------------------------------------------------------ caller's tables
def test_sigmas_reproduce_the_default_table():
    ref = DeterministicSolver(num_steps=18)
    for given in (ref.t_steps[:-1], ref.t_steps[:-1].tolist(), ref.t_steps[:-1].numpy(), ref.t_steps[:-1].double()):
        sol = DeterministicSolver(sigmas=given)
        assert sol.t_steps.dtype == torch.float32 and torch.equal(sol.t_steps, ref.t_steps)
        assert sol.num_steps == 18 and sol.rho is None
        assert (sol.sigma_max, sol.sigma_min) == (ref.t_steps[0].item(), ref.t_steps[17].item())
        assert sol.guided_evaluations() == ref.guided_evaluations() == (False,) * 35
    # the default constructor is untouched
    assert (ref.num_steps, ref.sigma_min, ref.sigma_max, ref.rho) == (18, 0.002, 80.0, 7.0)


@pytest.mark.parametrize("cls,kw", [(StochasticSolver, {"S_churn": 10.0}), (MultistepSolver, {"order": 3}),
                                    (ParallelSolver, {"window": 4})], ids=["stochastic", "multistep", "parallel"])
def test_sigmas_on_the_other_table_solvers(cls, kw):
    table = [10.0, 3.0, 1.0, 0.25, 0.01]
    sol = cls(sigmas=table, **kw)
    assert sol.num_steps == 5 and sol.t_steps.tolist() == torch.tensor(table + [0.0]).tolist() and sol.rho is None
    assert (sol.sigma_max, sol.sigma_min) == (10.0, torch.tensor(0.01).item())
    sol.guided_evaluations()
    ref = cls(num_steps=7, **kw)
    assert torch.equal(cls(sigmas=ref.t_steps[:-1], **kw).t_steps, ref.t_steps)
    if cls is MultistepSolver:
        assert torch.equal(cls(sigmas=ref.t_steps[:-1], **kw).multistep_coefficients(), ref.multistep_coefficients())
    if cls is StochasticSolver:
        s = sol.churn_schedule()
        assert s.t_hat.shape == (5,) and bool((s.t_hat >= sol.t_steps[:-1]).all())


@pytest.mark.parametrize("bad,match", [
    ([1.0], "at least 2"), ([], "at least 2"), ([[2.0, 1.0]], "one-dimensional"), ([2.0, float("nan")], "finite"),
    ([float("inf"), 1.0], "finite"), ([2.0, 0.0], "> 0"), ([2.0, -1.0], "> 0"), ([1.0, 1.0], "strictly decreasing"),
    ([1.0, 2.0], "strictly decreasing"), ([1.0 + 1e-10, 1.0], "strictly decreasing"),      # equal after rounding to fp32
    ([1.0, 1e-60], "strictly decreasing"),                                                  # 0 after rounding to fp32
    ("abc", "sigmas"),
], ids=["one", "none", "2d", "nan", "inf", "zero", "negative", "equal", "increasing", "equal-in-fp32", "zero-in-fp32", "str"])
def test_sigmas_refusals(bad, match):
    for cls in (DeterministicSolver, StochasticSolver, MultistepSolver, ParallelSolver):
        with pytest.raises(ValueError, match=match):
            cls(sigmas=bad)


def test_adaptive_solver_refuses_a_table():
    with pytest.raises(ValueError, match="sigmas is not implemented for the adaptive solver"):
        AdaptiveSolver(sigmas=[2.0, 1.0])
    AdaptiveSolver()


def test_trace_refuses_on_the_host():
    x0 = torch.zeros(2, 4)
    D = lambda x, s, labels=None: x     # noqa: E731
    sol = DeterministicSolver(num_steps=4)
    for kw in ({"graph": True}, {"start_step": 1}, {"image": x0}, {"mask": x0}, {"degradation": 1}, {"measurement": x0},
               {"operator": 1}, {"dps_scale": 1.0}):
        with pytest.raises(ValueError, match="not implemented for the recorder"):
            sol.trace(D, x0, **kw)
    with pytest.raises(ValueError, match="takes another step"):
        MultistepSolver(num_steps=4).trace(D, x0)
    with pytest.raises(ValueError, match="churned"):
        StochasticSolver(num_steps=4, S_churn=10.0).trace(D, x0)
    for cls in (AdaptiveSolver, ParallelSolver):
        with pytest.raises(ValueError, match="recorder is not implemented"):
            cls(num_steps=4).trace(D, x0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sol.trace(D, x0)


# ------------------------------------------------------------------ the method, on the analytic denoisers
@pytest.fixture(scope="module")
def analytic():
    means, x0 = R.setting()
    grid = R.karras_table(GRID)
    out = {}
    for name, D in (("gaussian", R.gaussian), ("mixture", R.mixture(means))):
        X, S, tau = R.heun_trace(D, x0, grid)
        cost = R.step_costs(R.pair_step_errors(X, S, tau, 2))
        out[name] = (D, cost, R.heun_solve(D, x0, R.karras_table(257)))
    return x0, grid, out


def _rms(a, b):
    return float(np.sqrt(((a - b) ** 2).mean()))


@pytest.mark.parametrize("name,N", [("gaussian", 9), ("gaussian", 17), ("mixture", 9)])
def test_optimised_table_beats_karras_on_analytic_denoisers(analytic, name, N):
    x0, grid, dens = analytic
    D, cost, truth = dens[name]
    idx, _ = schedule.best_path(cost, N)
    assert list(idx) == list(R.best_path(cost, N)[0])
    e_karras = _rms(R.heun_solve(D, x0, R.karras_table(N)), truth)
    e_opt = _rms(R.heun_solve(D, x0, grid[idx]), truth)
    print(f"{name} N = {N}: Karras {e_karras:.4g}, optimised {e_opt:.4g}, ratio {e_opt / e_karras:.3f}")
    assert e_opt < e_karras, (e_opt, e_karras)


@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_dp_cost_is_at_most_the_even_paths(analytic, name):
    cost = analytic[2][name][1]
    seen = 0
    for N in range(2, GRID + 1):
        even = R.even_path(GRID, N)
        idx, total = schedule.best_path(cost, N)
        assert total == R.path_cost(cost, idx)
        if even is not None:
            seen += 1
            assert total <= R.path_cost(cost, even), N
    assert seen == 6        # N - 1 a divisor of 63: N = 2, 4, 8, 10, 22, 64
    found = schedule.schedules_from_costs(cost, np.append(R.karras_table(GRID), 0.0), [8, 9, 64], order=2, warmup=8, seed=0)
    assert [s.num_steps for s in found] == [8, 9, 64] and found[1].karras_cost is None
    assert found[0].karras_cost == R.path_cost(cost, R.even_path(GRID, 8)) >= found[0].cost
    assert found[2].indices == list(range(GRID)) and found[2].cost == found[2].karras_cost
    assert found[0].sigmas == torch.tensor(R.karras_table(GRID))[found[0].indices].tolist()


def test_ref_pair_errors_and_costs():
    """the reference's own pieces against hand arithmetic"""
    X = np.array([[[4.0, 0.0]], [[2.0, 1.0]], [[1.0, 1.0]]])     # [G + 1 = 3, B = 1, K = 2]
    S = np.array([[[1.0, -1.0]], [[2.0, 0.0]]])
    tau = np.array([2.0, 1.0, 0.0])
    d1, d2 = R.pair_step_errors(X, S, tau, 1), R.pair_step_errors(X, S, tau, 2)
    # 0 -> 1, h = -1: Euler e = (4 - 1 - 2, 0 + 1 - 1) = (1, 0); trapezoid e = (4 - 1.5 - 2, 0 + .5 - 1) = (.5, -.5)
    assert d1[0, 0, 1] == 1.0 and d2[0, 0, 1] == 0.5
    # 0 -> 2 (the end: Euler in both), h = -2: e = (4 - 2 - 1, 0 + 2 - 1) = (1, 1);  1 -> 2, h = -1: e = (2 - 2 - 1, 1 - 1) = (-1, 0)
    assert d1[0, 0, 2] == d2[0, 0, 2] == 2.0 and d1[0, 1, 2] == d2[0, 1, 2] == 1.0
    assert d1[0, 1, 0] == d1[0, 1, 1] == d1[0, 0, 0] == 0.0
    cost = R.step_costs(np.concatenate([d1, 4 * d1]))
    assert cost[0, 1] == 1.5 and np.isinf(cost[0, 0]) and np.isinf(cost[1, 1]) and np.isinf(cost[1, 0])
    assert R.pair_step_magnitudes(X, S, tau, 2)[0, 0, 1] == (4 + 1.5 + 2) ** 2 + (0.5 + 1) ** 2


# ------------------------------------------------------------------ the file, the validator, the C ABI
def test_schedule_json_round_trip(tmp_path):
    a = schedule.Schedule([80.0, torch.tensor(0.3).item(), torch.tensor(0.002).item()], [0, 5, 9], 1.25, None, 2, 10, 8, 3)
    b = schedule.Schedule([80.0, 0.5], [0, 9], 2.5, 2.5, 1, 10, 8, 3)
    one = tmp_path / "one.json"
    a.save(one)
    assert schedule.Schedule.load(one) == a == schedule.Schedule.load(one, 3) and a.num_steps == 3
    both = tmp_path / "both.json"
    schedule.save_schedules([a, b], both)
    assert schedule.load_schedules(both) == {3: a, 2: b}
    assert schedule.Schedule.load(both, 2) == b
    with pytest.raises(ValueError, match=r"no schedule for num_steps = 5; it has N = \[2, 3\]"):
        schedule.Schedule.load(both, 5)
    with pytest.raises(ValueError, match="it has N"):
        schedule.Schedule.load(both)
    bad = tmp_path / "bad.json"
    bad.write_text("{}")
    with pytest.raises(ValueError, match="not a schedule file"):
        schedule.load_schedules(bad)
    # the table of a file goes straight into a solver
    assert DeterministicSolver(sigmas=schedule.Schedule.load(one).sigmas).t_steps.tolist()[:3] == a.sigmas
    import tinyedm
    import tinyedm.schedule as alias
    assert alias.optimize_schedule is schedule.optimize_schedule is tinyedm.optimize_schedule and alias.main is schedule.main


def _validate_kw(**kw):
    import inspect
    from tinyedm_amd import generate as G
    defaults = {k: p.default for k, p in inspect.signature(G.generate).parameters.items()}
    return {**{k: defaults.get(k, False) for k in inspect.signature(G._validate).parameters}, "image_size": 32,
            "num_steps": 8, **kw}


def test_validate_sigma_table(tmp_path):
    from tinyedm_amd import generate as G
    assert _validate_kw()["sigma_table"] is None
    with pytest.raises(ValueError, match="--solver adaptive does not take --sigma_table"):
        G._validate(**_validate_kw(sigma_table="s.json", solver="adaptive"))
    for kw in ({}, {"solver": "dpmpp"}, {"solver": "picard"}, {"S_churn": 10.0}, {"guided": True}):
        assert G._validate(**_validate_kw(sigma_table="s.json", **kw)) == (False, False)
    # generate() reads the file before anything is loaded: a file without the N is refused, naming the N it has
    path = tmp_path / "s.json"
    schedule.Schedule([80.0, 1.0, 0.002], [0, 4, 9], 1.0, None, 2, 10, 8, 0).save(path)
    with pytest.raises(ValueError, match=r"no schedule for num_steps = 8; it has N = \[3\]"):
        G.generate("missing.ckpt", False, str(tmp_path / "out"), 4, 32, 10, 2, num_steps=8, sigma_table=str(path))
    with pytest.raises(SystemExit):
        G.main(["--output_dir", "o", "--num_samples", "1", "--image_size", "32", "--num_classes", "10", "--batch_size", "1",
                "--solver", "adaptive", "--sigma_table", str(path)])


def test_optimize_schedule_refuses_on_the_host():
    D = lambda x, s, labels=None: x     # noqa: E731
    for kw, match in (({"order": 3}, "order"), ({"grid": 1}, "grid"), ({"grid": 257}, "grid"), ({"warmup": 0}, "warmup"),
                      ({"batch_size": 0}, "batch_size")):
        with pytest.raises(ValueError, match=match):
            schedule.optimize_schedule(D, 4, shape=(8,), **kw)
    for n in (1, 65, [4, 70]):
        with pytest.raises(ValueError, match="num_steps"):
            schedule.optimize_schedule(D, n, shape=(8,))


def test_pair_step_errors_declared_in_header_and_lib():
    from tinyedm_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    m = re.search(r"int edm_pair_step_errors\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["edm_pair_step_errors"]) == 9
    assert int(re.search(r"#define EDM_SCHEDULE_MAX_GRID (\d+)", hdr).group(1)) == ops.SCHEDULE_MAX_GRID >= 256
    assert os.path.exists(os.path.join(ROOT, "tinyedm_amd", "csrc", "schedule.hip"))
    with pytest.raises(ValueError, match="CUDA/HIP tensor"):
        ops.pair_step_errors(torch.zeros(3, 1, 4), torch.zeros(2, 1, 4), torch.zeros(3, dtype=torch.float64))
    assert math.isfinite(ops.SCHEDULE_MAX_GRID)
