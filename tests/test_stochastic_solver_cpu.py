"""Stochastic Heun sampling, host side (no GPU): the churn schedule of StochasticSolver against a restatement of
Algorithm 2 of Karras et al. 2022, the validation of the churn settings, which evaluations a guided stochastic solve
guides, instantiation from a config node, the churn record layout, the generate CLI flags and the C ABI declaration."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tinyedm_amd import DeterministicSolver, StochasticSolver, ops
from tinyedm_amd.config import instantiate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _guide(x, sigma, labels):
    raise AssertionError("the guide must not be evaluated on the host")


def _restated(t_steps, N, S_churn, S_min, S_max, S_noise):
    """Algorithm 2, lines 4-6, per step in fp64 on the fp32 table values; t_hat and c rounded to fp32"""
    gamma, t_hat, c = [], [], []
    for t in t_steps[:-1].tolist():
        g = min(S_churn / N, math.sqrt(2) - 1) if S_min <= t <= S_max else 0.0
        th = float(np.float32(t + g * t))
        gamma.append(np.float32(g))
        t_hat.append(th)
        c.append(np.float32(S_noise * math.sqrt(th * th - t * t)))
    return np.array(gamma, np.float32), np.array(t_hat, np.float32), np.array(c, np.float32)


@pytest.mark.parametrize("S_churn,S_min,S_max,S_noise", [(40.0, 0.05, 50.0, 1.003), (80.0, 0.0, math.inf, 1.0),
                                                          (3.2, 0.0, math.inf, 1.0), (40.0, 0.5, 2.0, 0.5)],
                         ids=["edm_imagenet", "capped", "uncapped", "narrow_window"])
def test_churn_schedule_matches_algorithm_2(S_churn, S_min, S_max, S_noise):
    N = 32
    sol = StochasticSolver(num_steps=N, S_churn=S_churn, S_min=S_min, S_max=S_max, S_noise=S_noise)
    s = sol.churn_schedule()
    assert all(v.dtype == torch.float32 and v.shape == (N,) for v in s)
    gamma, t_hat, c = _restated(sol.t_steps, N, S_churn, S_min, S_max, S_noise)
    assert np.array_equal(s.gamma.numpy(), gamma)
    assert np.array_equal(s.t_hat.numpy(), t_hat)
    assert np.array_equal(s.c.numpy(), c)
    t = sol.t_steps[:-1]
    inside = (t >= S_min) & (t <= S_max)
    assert torch.equal(s.gamma > 0, inside)
    assert torch.equal(s.t_hat[~inside], t[~inside]) and not s.c[~inside].any()
    assert (s.t_hat[inside] > t[inside]).all() and (s.c[inside] > 0).all()
    g = s.gamma[inside]
    assert torch.equal(g, torch.full_like(g, np.float32(min(S_churn / N, math.sqrt(2) - 1))))


def test_edm_imagenet_window_and_cap():
    sol = StochasticSolver(num_steps=32, S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)
    s = sol.churn_schedule()
    t = sol.t_steps[:-1]
    churned = (s.gamma > 0).nonzero().flatten().tolist()
    assert churned == [i for i, v in enumerate(t.tolist()) if 0.05 <= v <= 50]
    assert 0 < len(churned) < 32 and 0 not in churned and 31 not in churned    # t_0 = 80 > S_max, t_31 < S_min
    assert s.gamma.max().item() == pytest.approx(40 / 32 if 40 / 32 < math.sqrt(2) - 1 else math.sqrt(2) - 1)


def test_zero_churn_is_the_deterministic_table():
    sol = StochasticSolver(num_steps=18)
    s = sol.churn_schedule()
    assert torch.equal(s.t_hat, sol.t_steps[:-1]) and not s.c.any() and not s.gamma.any()
    assert torch.equal(sol.t_steps, DeterministicSolver(num_steps=18).t_steps)
    assert sol._evaluation_sigmas() == DeterministicSolver(num_steps=18)._evaluation_sigmas()
    assert sol._graph_key_extra() == ()


@pytest.mark.parametrize("kw,match", [
    ({"S_churn": -1.0}, "S_churn"), ({"S_churn": math.inf}, "S_churn"), ({"S_churn": math.nan}, "S_churn"),
    ({"S_noise": -0.1}, "S_noise"), ({"S_noise": math.inf}, "S_noise"), ({"S_noise": math.nan}, "S_noise"),
    ({"S_min": -0.01}, "S_min"), ({"S_min": 2.0, "S_max": 1.0}, "S_min"), ({"S_min": math.nan}, "S_min"),
    ({"seed": -1}, "seed"), ({"seed": 2 ** 64}, "seed"), ({"seed": 1.5}, "seed"), ({"seed": "7"}, "seed"),
])
def test_invalid_churn_settings_rejected(kw, match):
    with pytest.raises(ValueError, match=match):
        StochasticSolver(num_steps=8, S_churn=kw.pop("S_churn", 10.0), **kw)


def test_every_query_validates():
    sol = StochasticSolver(num_steps=8, S_churn=10.0, seed=2 ** 64 - 1)        # the largest seed is valid
    sol.churn_schedule()
    for attr, bad in (("S_churn", -1.0), ("S_noise", math.nan), ("S_min", -1.0), ("S_max", -1.0), ("seed", 2 ** 64),
                      ("solve_index", -1), ("solve_index", 2 ** 32)):
        old = getattr(sol, attr)
        setattr(sol, attr, bad)
        with pytest.raises(ValueError):
            sol.churn_schedule()
        with pytest.raises(ValueError):
            sol.guided_evaluations()
        setattr(sol, attr, old)
    sol.guided_evaluations()


def test_constructor_signature():
    a = StochasticSolver(18, 0.002, 80.0, 7.0, None)
    assert torch.equal(a.t_steps, DeterministicSolver(18, 0.002, 80.0, 7.0, None).t_steps)
    assert (a.S_churn, a.S_min, a.S_max, a.S_noise, a.seed, a.solve_index) == (0.0, 0.0, math.inf, 1.0, 0, 0)
    with pytest.raises(TypeError):
        StochasticSolver(18, 0.002, 80.0, 7.0, None, 40.0)       # the churn arguments are keyword-only
    assert isinstance(a, DeterministicSolver)


def test_guided_evaluations_use_t_hat():
    lo, hi = 0.28, 5.42
    N = 32
    sol = StochasticSolver(num_steps=N, guide=_guide, guidance=2.0, guidance_interval=(lo, hi), S_churn=40,
                           S_min=0.05, S_max=50)
    t = sol.t_steps.tolist()
    t_hat = sol.churn_schedule().t_hat.tolist()
    expected = []
    for i in range(N):          # Euler at t_hat_i, then (but for the last step) the correction at t_{i+1}
        expected.append(lo < t_hat[i] <= hi)
        if i < N - 1:
            expected.append(lo < t[i + 1] <= hi)
    flags = sol.guided_evaluations()
    assert list(flags) == expected
    # the churn moves some Euler evaluations across the interval's edge: the flags differ from the deterministic ones
    det = DeterministicSolver(num_steps=N, guide=_guide, guidance=2.0, guidance_interval=(lo, hi)).guided_evaluations()
    assert flags != det
    assert StochasticSolver(num_steps=N, guide=_guide, guidance=2.0, S_churn=40).guided_evaluations() == (True,) * 63


def test_instantiate_from_config_node():
    node = {"_target_": "tinyedm.StochasticSolver", "num_steps": 32, "sigma_min": 0.002, "sigma_max": 80.0,
            "rho": 7.0, "S_churn": 40, "S_min": 0.05, "S_max": 50, "S_noise": 1.003, "seed": 11}
    sol = instantiate(node)
    assert isinstance(sol, StochasticSolver)
    assert (sol.num_steps, sol.S_churn, sol.S_min, sol.S_max, sol.S_noise, sol.seed) == (32, 40, 0.05, 50, 1.003, 11)
    import tinyedm
    assert tinyedm.StochasticSolver is StochasticSolver
    assert tinyedm.solvers.StochasticSolver is StochasticSolver


def test_churn_record_layout():
    seed = 0x0123456789ABCDEF
    rec = ops.churn_record(seed, 7, "cpu")
    assert rec.dtype == torch.int32 and rec.shape == (4,)
    words = [v & 0xFFFFFFFF for v in rec.tolist()]
    assert words == [0x89ABCDEF, 0x01234567, 7, 0]
    assert [v & 0xFFFFFFFF for v in ops.churn_record(2 ** 64 - 1, 2 ** 32 - 1, "cpu").tolist()] == \
        [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    with pytest.raises(ValueError, match="seed"):
        ops.churn_record(2 ** 64, 0, "cpu")
    with pytest.raises(ValueError, match="solve_index"):
        ops.churn_record(0, 2 ** 32, "cpu")


def test_heun_churn_has_no_cpu_path():
    with pytest.raises(RuntimeError, match="CPU"):
        ops.heun_churn(torch.zeros(2, 3, 4, 4), 1.0, torch.zeros(4, dtype=torch.int32), 0)


def test_generate_help_lists_churn_flags(capsys):
    from tinyedm_amd.generate import main
    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--S_churn", "--S_min", "--S_max", "--S_noise"):
        assert re.search(rf"(^|\s){flag}(\s|$)", out, re.M), flag


def test_churn_declared_in_header_and_lib():
    from tinyedm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    assert "edm_heun_churn" in set(re.findall(r"\b(edm_[a-z0-9_]+)\s*\(", hdr))
    assert "edm_heun_churn" in _lib.SIGNATURES
