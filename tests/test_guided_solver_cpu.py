"""Guided Heun sampling, host side (no GPU): which evaluations a DeterministicSolver guides, the constructor's
validation of the guidance settings, the generate CLI flags and the C ABI declarations of the guided updates."""
import math
import os
import re

import pytest
import torch

from tinyedm_amd import DeterministicSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _guide(x, sigma, labels):       # a bare callable guide: never evaluated on the host
    raise AssertionError("the guide must not be evaluated by guided_evaluations()")


def test_guided_evaluations_with_interval_match_fp32_table():
    lo, hi = 0.28, 5.42
    sol = DeterministicSolver(num_steps=32, guide=_guide, guidance=2.0, guidance_interval=(lo, hi))
    flags = sol.guided_evaluations()
    t = sol.t_steps
    assert t.dtype == torch.float32
    expected = []
    for i in range(32):          # loop order: Euler at t_i, then (but for the last step) the correction at t_{i+1}
        expected.append(bool(lo < t[i].item() <= hi))
        if i < 31:
            expected.append(bool(lo < t[i + 1].item() <= hi))
    assert len(flags) == 63
    assert list(flags) == expected
    assert sum(flags) == 20


def test_guided_evaluations_without_interval_and_at_guidance_one():
    assert DeterministicSolver(num_steps=32, guide=_guide, guidance=2.0).guided_evaluations() == (True,) * 63
    assert DeterministicSolver(num_steps=32, guide=_guide, guidance=1.0).guided_evaluations() == (False,) * 63
    assert DeterministicSolver(num_steps=32, guide=_guide, guidance=1.0,
                               guidance_interval=(0.28, 5.42)).guided_evaluations() == (False,) * 63
    assert DeterministicSolver(num_steps=32).guided_evaluations() == (False,) * 63


def test_guidance_attributes_take_effect_at_the_next_query():
    sol = DeterministicSolver(num_steps=18, guide=_guide, guidance=1.0)
    assert not any(sol.guided_evaluations())
    sol.guidance = 3.0
    assert all(sol.guided_evaluations())
    sol.guidance_interval = (0.5, 2.0)
    flags = sol.guided_evaluations()
    assert 0 < sum(flags) < len(flags)


def test_positional_signature_and_sigma_table_unchanged():
    a = DeterministicSolver(18, 0.002, 80.0, 7.0, None)
    b = DeterministicSolver(18, 0.002, 80.0, 7.0, None, guide=_guide, guidance=2.0, guidance_interval=(0.1, 1.0))
    assert torch.equal(a.t_steps, b.t_steps)
    with pytest.raises(TypeError):
        DeterministicSolver(18, 0.002, 80.0, 7.0, None, _guide)       # guide is keyword-only


@pytest.mark.parametrize("w", [math.nan, math.inf, -math.inf])
def test_non_finite_guidance_rejected(w):
    with pytest.raises(ValueError, match="finite"):
        DeterministicSolver(num_steps=8, guide=_guide, guidance=w)


def test_guidance_without_guide_rejected():
    with pytest.raises(ValueError, match="guide"):
        DeterministicSolver(num_steps=8, guidance=2.0)
    DeterministicSolver(num_steps=8, guidance=1.0)          # unguided: no guide needed
    sol = DeterministicSolver(num_steps=8)
    sol.guidance = 0.5
    with pytest.raises(ValueError, match="guide"):
        sol.guided_evaluations()


@pytest.mark.parametrize("interval", [(-0.1, 1.0), (1.0, 1.0), (2.0, 1.0), (math.nan, 1.0)])
def test_bad_guidance_interval_rejected(interval):
    with pytest.raises(ValueError, match="guidance_interval"):
        DeterministicSolver(num_steps=8, guide=_guide, guidance=2.0, guidance_interval=interval)


def test_generate_help_lists_guidance_flags(capsys):
    from tinyedm_amd.generate import main
    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--guide_ckpt_path", "--guide_load_ema", "--guide_config_name", "--guidance", "--guidance_interval"):
        assert re.search(rf"(^|\s){flag}(\s|$)", out, re.M), flag


def test_guided_updates_declared_in_header():
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    declared = set(re.findall(r"\b(edm_[a-z0-9_]+)\s*\(", hdr))
    assert {"edm_heun_euler_guided", "edm_heun_correct_guided"} <= declared
