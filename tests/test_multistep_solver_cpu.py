"""DPM-Solver++ multistep sampling, host side (no GPU): the coefficient table of MultistepSolver against an independent
fp64 restatement of the update in its D1/D2 form, the warm-up and final-step rows, order 1 against EDM's Euler step,
the validation rules, which evaluations a guided solve guides, instantiation from a config node, the generate CLI flags
and the C ABI declaration."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tinyedm_amd import DeterministicSolver, MultistepSolver, StochasticSolver, ops
from tinyedm_amd.config import instantiate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _guide(x, sigma, labels):
    raise AssertionError("the guide must not be evaluated on the host")


def _restated(t_steps, N, order):
    """fp64 rows (a, c0, c1, c2): the update of step i applied to x = 0 and unit m_i, m_{i-1}, m_{i-2}"""
    sig = t_steps.double().tolist()

    def lam(j):
        return -math.log(sig[j]) if sig[j] > 0 else math.inf

    rows = []
    for i in range(N):
        h = lam(i + 1) - lam(i)
        e = math.expm1(-h)
        k = 1 if i == N - 1 else min(order, i + 1)

        def update(m0, m1, m2):
            if k == 1:
                return -e * m0
            if k == 2:
                r = (lam(i) - lam(i - 1)) / h
                return -e * ((1 + 1 / (2 * r)) * m0 - (1 / (2 * r)) * m1)
            r0 = (lam(i) - lam(i - 1)) / h
            r1 = (lam(i - 1) - lam(i - 2)) / h
            D1_0 = (m0 - m1) / r0
            D1_1 = (m1 - m2) / r1
            D1 = D1_0 + r0 / (r0 + r1) * (D1_0 - D1_1)
            D2 = (D1_0 - D1_1) / (r0 + r1)
            return -e * m0 + (e / h + 1) * D1 - ((e + h) / h ** 2 - 0.5) * D2

        rows.append([sig[i + 1] / sig[i], update(1.0, 0.0, 0.0), update(0.0, 1.0, 0.0), update(0.0, 0.0, 1.0)])
    return np.array(rows, dtype=np.float64)


SCHEDULES = {"default": {}, "custom": {"sigma_min": 0.01, "sigma_max": 20.0, "rho": 5.0}}


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("N", [2, 5, 18, 32])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_coefficients_match_restatement(order, N, sched):
    sol = MultistepSolver(num_steps=N, order=order, **SCHEDULES[sched])
    assert torch.equal(sol.t_steps, DeterministicSolver(num_steps=N, **SCHEDULES[sched]).t_steps)
    c = sol.multistep_coefficients()
    assert c.dtype == torch.float32 and c.shape == (N, 4)
    ref = _restated(sol.t_steps, N, order)
    got = c.double().numpy()
    # fp32 rounding of the fp64 value, plus fp64 round-off amplified by the cancellation in the order-3 sums
    tol = 2.0 ** -24 * np.abs(ref) + 1e-12 * np.abs(ref).max(axis=1, keepdims=True)
    assert np.all(np.abs(got - ref) <= tol), np.abs(got - ref).max()
    # consistency: a + c0 + c1 + c2 = 1 (a constant denoiser D = x keeps x), to the fp32 rounding of the four terms
    s = got.sum(axis=1)
    assert np.all(np.abs(s - 1.0) <= 4 * 2.0 ** -24 * np.abs(got).sum(axis=1)), s


@pytest.mark.parametrize("order", [1, 2, 3])
def test_warmup_and_final_rows(order):
    N = 18
    c = MultistepSolver(num_steps=N, order=order).multistep_coefficients()
    assert c[-1].tolist() == [0.0, 1.0, 0.0, 0.0]
    first = MultistepSolver(num_steps=N, order=1).multistep_coefficients()
    assert torch.equal(c[0], first[0])                          # k = 1 at step 0
    assert c[0, 2] == 0 and c[0, 3] == 0
    if order >= 2:
        assert c[1, 2] != 0 and c[1, 3] == 0                    # k = 2 at step 1
        assert (c[1:N - 1, 2] != 0).all()
        assert torch.equal(c[1], MultistepSolver(num_steps=N, order=2).multistep_coefficients()[1])
    if order == 3:
        assert (c[2:N - 1, 3] != 0).all()                       # k = 3 from step 2 to N - 2
    else:
        assert not c[:, 3].any()
    if order == 1:
        assert not c[:, 2:].any()
    k = [s[0] for s in MultistepSolver(num_steps=N, order=order)._steps()]
    assert k == [1] + [min(order, i + 1) for i in range(1, N - 1)] + [1]


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_order_one_is_edm_euler(sched):
    N = 32
    sol = MultistepSolver(num_steps=N, order=1, **SCHEDULES[sched])
    c = sol.multistep_coefficients().double()
    t = sol.t_steps.double()
    # EDM's Euler step x + (t1 - t0) * (x - D) / t0 = (t1 / t0) x + (1 - t1 / t0) D
    a = t[1:] / t[:-1]
    assert torch.allclose(c[:, 0], a, rtol=2.0 ** -23, atol=0)
    assert torch.allclose(c[:, 1], 1 - a, rtol=2.0 ** -23, atol=2.0 ** -24)
    assert not c[:, 2:].any()


@pytest.mark.parametrize("kw,match", [
    ({"order": 0}, "order"), ({"order": 4}, "order"), ({"order": True}, "order"), ({"order": "2"}, "order"),
    ({"num_steps": 1}, "num_steps"), ({"num_steps": 0}, "num_steps"), ({"num_steps": -3}, "num_steps"),
    ({"guidance": 2.0}, "needs a guide"), ({"guidance": math.nan, "guide": _guide}, "finite"),
    ({"guidance": math.inf, "guide": _guide}, "finite"),
    ({"guidance": 2.0, "guide": _guide, "guidance_interval": (3.0, 1.0)}, "0 <= lo < hi"),
    ({"guidance": 2.0, "guide": _guide, "guidance_interval": (-1.0, 1.0)}, "0 <= lo < hi"),
    ({"dtype": "float64"}, "float32"),
])
def test_invalid_settings_rejected(kw, match):
    with pytest.raises(ValueError, match=match):
        MultistepSolver(**{"num_steps": 8, **kw})


def test_every_query_validates():
    sol = MultistepSolver(num_steps=8, order=3, guide=_guide, guidance=2.0)
    for attr, bad in (("order", 4), ("order", 0), ("guidance", math.nan), ("guidance_interval", (2.0, 1.0))):
        old = getattr(sol, attr)
        setattr(sol, attr, bad)
        with pytest.raises(ValueError):
            sol.guided_evaluations()
        if attr == "order":
            with pytest.raises(ValueError, match="order"):
                sol.multistep_coefficients()
        setattr(sol, attr, old)
    sol.guided_evaluations()


def test_constructor_signature():
    a = MultistepSolver(18, 0.002, 80.0, 7.0, None)
    assert torch.equal(a.t_steps, DeterministicSolver(18, 0.002, 80.0, 7.0, None).t_steps)
    assert a.order == 2 and a.guidance == 1.0 and a.guide is None and a.guidance_interval is None
    with pytest.raises(TypeError):
        MultistepSolver(18, 0.002, 80.0, 7.0, None, 3)          # order is keyword-only
    assert isinstance(a, DeterministicSolver)


def test_guided_evaluations_one_per_step():
    N, lo, hi = 32, 0.28, 5.42
    sol = MultistepSolver(num_steps=N, guide=_guide, guidance=2.0, guidance_interval=(lo, hi))
    t = sol.t_steps.tolist()
    flags = sol.guided_evaluations()
    assert list(flags) == [lo < t[i] <= hi for i in range(N)]
    assert any(flags) and not all(flags)
    assert MultistepSolver(num_steps=N, guide=_guide, guidance=2.0).guided_evaluations() == (True,) * N
    assert MultistepSolver(num_steps=N, guide=_guide, guidance=1.0,
                           guidance_interval=(lo, hi)).guided_evaluations() == (False,) * N
    assert MultistepSolver(num_steps=N).guided_evaluations() == (False,) * N


def test_heun_solvers_keep_their_key():
    assert DeterministicSolver(num_steps=18)._graph_key_extra() == ()
    assert StochasticSolver(num_steps=18)._graph_key_extra() == ()
    keys = {o: MultistepSolver(num_steps=18, order=o)._graph_key_extra() for o in (1, 2, 3)}
    assert all(k and k[0] == "multistep" for k in keys.values())
    assert len(set(keys.values())) == 3


def test_instantiate_from_config_node():
    node = {"_target_": "tinyedm.MultistepSolver", "num_steps": 18, "order": 3}
    sol = instantiate(node)
    assert isinstance(sol, MultistepSolver)
    assert (sol.num_steps, sol.order) == (18, 3)
    import tinyedm
    assert tinyedm.MultistepSolver is MultistepSolver
    assert tinyedm.solvers.MultistepSolver is MultistepSolver


def test_dpm_multistep_has_no_cpu_path():
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.dpm_multistep(x, x, 0.5, 0.5)


def test_generate_rejects_churn_with_dpmpp(tmp_path):
    from tinyedm_amd.generate import generate, main
    missing = str(tmp_path / "missing.ckpt")                 # never opened: the check runs first
    args = ["--ckpt_path", missing, "--output_dir", str(tmp_path / "out"), "--num_samples", "4", "--image_size", "32",
            "--num_classes", "10", "--batch_size", "4"]
    with pytest.raises(ValueError, match="S_churn"):
        main(args + ["--solver", "dpmpp", "--S_churn", "5"])
    with pytest.raises(ValueError, match="S_churn"):
        main(["--config_name", "cifar10"] + args[2:] + ["--solver", "dpmpp", "--S_churn", "5"])
    with pytest.raises(ValueError, match="S_churn"):
        generate(missing, False, str(tmp_path / "out"), 4, 32, 10, 4, solver="dpmpp", S_churn=5.0)
    with pytest.raises(ValueError, match="solver"):
        generate(missing, False, str(tmp_path / "out"), 4, 32, 10, 4, solver="euler")
    assert not (tmp_path / "out").exists()


def test_generate_help_lists_solver_flags(capsys):
    from tinyedm_amd.generate import main
    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--solver", "--solver_order"):
        assert re.search(rf"(^|\s){flag}(\s|$)", out, re.M), flag
    assert "dpmpp" in out


def test_multistep_declared_in_header_and_lib():
    from tinyedm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    assert "edm_dpm_multistep" in set(re.findall(r"\b(edm_[a-z0-9_]+)\s*\(", hdr))
    assert "edm_dpm_multistep" in _lib.SIGNATURES
