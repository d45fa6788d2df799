"""Zero-shot restoration (DDNM), host side (no GPU): the CPU reference itself (A A+ = I, A+ A an orthogonal projector,
the decoupling identity of the analytic Gaussian denoiser in fp64), the validation of LinearDegradation and of solve()'s
degradation / measurement on the three solvers, all raised before a device is touched, the generate CLI argument errors,
and the C ABI declarations of edm_degrade and edm_project_denoised."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import restoration_ref as R
from tinyedm_amd import DeterministicSolver, LinearDegradation, MultistepSolver, StochasticSolver, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_OPERATORS = [(s, g) for s in (1, 2, 4, 8) for g in (False, True) if (s, g) != (1, False)]


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("scale,gray", ALL_OPERATORS)
def test_reference_operator_algebra(scale, gray):
    g = torch.Generator().manual_seed(scale + 10 * gray)
    x = torch.randn(3, 3, 16, 16, generator=g, dtype=torch.float64)
    y = torch.randn(3, 1 if gray else 3, 16 // scale, 16 // scale, generator=g, dtype=torch.float64)
    assert R.degrade(x, scale, gray).shape == y.shape
    assert R.pinv(y, scale, gray, 3).shape == x.shape
    assert (R.degrade(R.pinv(y, scale, gray, 3), scale, gray) - y).abs().max() <= 1e-15          # A A+ = I
    P = lambda v: R.pinv(R.degrade(v, scale, gray), scale, gray, 3)
    assert (P(P(x)) - P(x)).abs().max() <= 1e-15                                                  # idempotent
    z = torch.randn(3, 3, 16, 16, generator=g, dtype=torch.float64)
    assert abs(((P(x) * z).sum() - (x * P(z)).sum()).item()) <= 1e-11                             # symmetric
    assert (P(x).norm() <= x.norm()).item()                                                       # never enlarges
    assert (R.degrade(R.project(x, y, scale, gray), scale, gray) - y).abs().max() <= 1e-14        # A D^ = y
    assert R.block_terms(scale, gray, 3) == scale * scale * (3 if gray else 1)


def _tables(order=None):
    sol = DeterministicSolver(num_steps=18) if order is None else MultistepSolver(num_steps=18, order=order)
    t = sol.t_steps.double().tolist()
    return t, (None if order is None else sol.multistep_coefficients().double().tolist())


@pytest.mark.parametrize("order", [None, 1, 2, 3], ids=["heun", "multistep1", "multistep2", "multistep3"])
@pytest.mark.parametrize("scale,gray", R.OPERATORS)
def test_decoupling_identity_fp64(scale, gray, order):
    """D is an isotropic affine map and commutes with the projector, so the ODE decouples:
    restore(x0, y) = A+ y + (I - A+ A) plain(x0)"""
    t, coeffs = _tables(order)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(16, 3, 16, 16, generator=g, dtype=torch.float64)
    y = R.degrade(R.MU + R.SD * torch.randn(16, 3, 16, 16, generator=g, dtype=torch.float64), scale, gray)
    proj = R.projector(y, scale, gray)
    if order is None:
        plain, rest = R.solve_heun(R.gaussian, t, x0), R.solve_heun(R.gaussian, t, x0, proj)
    else:
        plain = R.solve_multistep(R.gaussian, t, coeffs, x0)
        rest = R.solve_multistep(R.gaussian, t, coeffs, x0, proj)
    Pp = R.pinv(R.degrade(plain, scale, gray), scale, gray, 3)
    e = R.rel(rest, R.pinv(y, scale, gray, 3) + plain - Pp)
    print(f"decoupling ({scale}, {gray}) {order}: rel {e:.2e}")
    assert e <= 1e-13, e
    assert (R.degrade(rest, scale, gray) - y).abs().max() <= 1e-14
    assert R.rel(rest, plain) >= 0.05                           # the measurement moved the sample


# ------------------------------------------------------------------ LinearDegradation
def test_linear_degradation_value_type():
    d = LinearDegradation()
    assert (d.scale, d.gray) == (4, False) and d == LinearDegradation(4, False) and d != LinearDegradation(4, True)
    assert "scale=4" in repr(d)
    with pytest.raises(Exception):
        d.scale = 2                                             # frozen
    for scale, gray in ALL_OPERATORS:
        assert LinearDegradation(scale, gray).measurement_shape((5, 3, 16, 24)) == \
            (5, 1 if gray else 3, 16 // scale, 24 // scale)
    import tinyedm
    assert tinyedm.LinearDegradation is LinearDegradation


@pytest.mark.parametrize("scale,gray,match", [
    (1, False, "identity"), (3, False, "scale"), (0, True, "scale"), (16, False, "scale"), (2.0, False, "scale"),
    ("4", False, "scale"), (True, True, "scale"), (None, False, "scale"), (4, 1, "gray"), (4, None, "gray"),
])
def test_linear_degradation_rejects(scale, gray, match):
    with pytest.raises(ValueError, match=match):
        LinearDegradation(scale, gray)


def test_linear_degradation_shapes_and_devices():
    d = LinearDegradation(4, True)
    for shape in ((2, 3, 10, 8), (2, 3, 8, 10), (2, 9, 8, 8), (2, 3, 8), (2, 3, 8, 8, 1), (0, 3, 8, 8)):
        with pytest.raises(ValueError, match="degradation"):
            d.measurement_shape(shape)
    assert LinearDegradation(4, False).measurement_shape((2, 9, 8, 8)) == (2, 9, 2, 2)      # only gray limits C
    with pytest.raises(ValueError, match="image"):
        d.measure(torch.zeros(2, 3, 8, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="degradation"):
        d.measure(torch.zeros(2, 3, 6, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        d.measure(torch.zeros(2, 3, 8, 8))
    with pytest.raises(ValueError, match="channels"):
        d.pinv(torch.zeros(2, 1, 2, 2), 0)
    with pytest.raises(ValueError, match="pinv"):
        d.pinv(torch.zeros(2, 3, 2, 2), 3)                      # a gray measurement has one channel
    with pytest.raises(ValueError, match="pinv"):
        LinearDegradation(2).pinv(torch.zeros(2, 3, 2, 2), 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        d.pinv(torch.zeros(2, 1, 2, 2), 3)


def test_new_ops_have_no_cpu_path_and_validate_first():
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.degrade(x, 2, False)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.project_denoised(x, torch.zeros(2, 3, 4, 4), 2, False)
    assert ops.measurement_shape((2, 3, 8, 8), 8, True) == (2, 1, 1, 1)
    for bad in ((3, False), (1, False), (2, 1)):
        with pytest.raises(ValueError, match="degradation"):
            ops.check_degradation(*bad)


# ------------------------------------------------------------------ solve()
def _model(x, sigma, labels):
    raise AssertionError("the model must not be evaluated on the host")


SOLVERS = {"heun": lambda **kw: DeterministicSolver(num_steps=8, **kw),
           "stochastic": lambda **kw: StochasticSolver(num_steps=8, S_churn=10.0, **kw),
           "multistep": lambda **kw: MultistepSolver(num_steps=8, order=3, **kw)}
X0 = torch.zeros(2, 3, 8, 8)


@pytest.fixture(params=sorted(SOLVERS))
def sol(request):
    return SOLVERS[request.param]()


def test_solve_needs_both_or_neither(sol):
    with pytest.raises(ValueError, match="go together"):
        sol.solve(_model, X0, degradation=LinearDegradation(2))
    with pytest.raises(ValueError, match="go together"):
        sol.solve(_model, X0, measurement=torch.zeros(2, 3, 4, 4))


@pytest.mark.parametrize("deg", [(2, False), "sr4", 4, ops])
def test_solve_rejects_foreign_operators(sol, deg):
    with pytest.raises(ValueError, match="LinearDegradation"):
        sol.solve(_model, X0, degradation=deg, measurement=torch.zeros(2, 3, 4, 4))


@pytest.mark.parametrize("y,match", [
    (torch.zeros(2, 3, 2, 2), "shape"), (torch.zeros(2, 1, 4, 4), "shape"), (torch.zeros(1, 3, 4, 4), "shape"),
    (torch.zeros(2, 3, 16), "shape"), (torch.zeros(2, 3, 4, 4, dtype=torch.int32), "floating"),
    (np.zeros((2, 3, 4, 4), np.float32), "tensor"),
])
def test_solve_rejects_bad_measurements(sol, y, match):
    with pytest.raises(ValueError, match=match):
        sol.solve(_model, X0, degradation=LinearDegradation(2), measurement=y)


def test_solve_rejects_mask_and_bad_state(sol):
    y = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match="mask"):
        sol.solve(_model, X0, image=torch.zeros_like(X0), mask=torch.ones(8, 8), degradation=LinearDegradation(2),
                  measurement=y)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        sol.solve(_model, torch.zeros(2, 192), degradation=LinearDegradation(2), measurement=y)
    with pytest.raises(ValueError, match="multiples"):
        sol.solve(_model, torch.zeros(2, 3, 6, 6), degradation=LinearDegradation(4), measurement=y)
    with pytest.raises(ValueError, match="at most"):
        sol.solve(_model, torch.zeros(2, 9, 8, 8), degradation=LinearDegradation(2, True),
                  measurement=torch.zeros(2, 1, 4, 4))
    with pytest.raises(ValueError, match="on "):
        sol.solve(_model, X0, degradation=LinearDegradation(2), measurement=y.to("meta"))
    assert sol.solve_index == 0


@pytest.mark.parametrize("scale,gray", ALL_OPERATORS)
def test_valid_arguments_reach_the_device_check(sol, scale, gray):
    """every accepted operator passes the host validation; what stops the call then is the missing GPU"""
    deg = LinearDegradation(scale, gray)
    y = torch.zeros(deg.measurement_shape(X0.shape), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sol.solve(_model, X0, degradation=deg, measurement=y)
    with pytest.raises(RuntimeError, match="no CPU path"):
        sol.solve(_model, X0, start_step=5, image=torch.zeros_like(X0), degradation=deg, measurement=y)


def test_invert_and_likelihood_do_not_take_the_arguments():
    s = DeterministicSolver(num_steps=8)
    for fn in (s.invert, s.log_likelihood):
        with pytest.raises(TypeError):
            fn(_model, X0, degradation=LinearDegradation(2), measurement=torch.zeros(2, 3, 4, 4))
    doc = DeterministicSolver.__doc__
    for word in ("DDNM", "degradation", "not implemented"):
        assert word in doc


# ------------------------------------------------------------------ generate CLI
ARGS = ["--config_name", "cifar10_cond", "--output_dir", "unused", "--num_samples", "4", "--image_size", "32",
        "--num_classes", "10", "--batch_size", "4", "--num_steps", "6"]


@pytest.mark.parametrize("extra,match", [
    (["--restore_scale", "4"], "--restore_scale needs --init_dir"),
    (["--restore_gray"], "--restore_gray needs --init_dir"),
    (["--init_dir", "d", "--restore_scale", "3"], "--restore_scale"),
    (["--init_dir", "d", "--restore_scale", "0"], "--restore_scale"),
    (["--init_dir", "d", "--save_degraded", "x"], "--save_degraded needs"),
    (["--init_dir", "d", "--restore_report", "r.json"], "--restore_report needs"),
    (["--init_dir", "d", "--restore_scale", "4", "--mask_box", "0", "0", "8", "8"], "--mask_box are exclusive"),
    (["--init_dir", "d", "--restore_gray", "--invert_to", "l.pt"], "--invert_to are exclusive"),
    (["--init_dir", "d", "--restore_scale", "2", "--likelihood_to", "l.json"], "--likelihood_to are exclusive"),
    (["--init_dir", "d", "--restore_scale", "4", "--start_step", "6"], "--start_step must be below"),
])
def test_cli_argument_errors(capsys, extra, match):
    from tinyedm_amd.generate import main
    with pytest.raises(SystemExit) as e:
        main(ARGS + extra)
    assert e.value.code == 2                                    # an argparse error: nothing was loaded
    assert match in capsys.readouterr().err


def test_cli_scale_must_divide_image_size(capsys):
    from tinyedm_amd.generate import main
    args = [a if a != "32" else "12" for a in ARGS]
    with pytest.raises(SystemExit) as e:
        main(args + ["--init_dir", "d", "--restore_scale", "8"])
    assert e.value.code == 2 and "--restore_scale 8 must divide" in capsys.readouterr().err


def test_generate_function_rejects_the_same(tmp_path):
    from tinyedm_amd.generate import generate
    missing = str(tmp_path / "missing.ckpt")                    # never opened: the checks run first
    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="init_dir"):
        generate(missing, False, out, 4, 32, 10, 4, restore_scale=4)
    with pytest.raises(ValueError, match="init_dir"):
        generate(missing, False, out, 4, 32, 10, 4, restore_gray=True)
    with pytest.raises(ValueError, match="restore_scale"):
        generate(missing, False, out, 4, 32, 10, 4, init_dir=str(tmp_path), restore_scale=5)
    with pytest.raises(ValueError, match="exclusive"):
        generate(missing, False, out, 4, 32, 10, 4, init_dir=str(tmp_path), restore_scale=4, mask_box=(0, 0, 8, 8))
    with pytest.raises(ValueError, match="save_degraded"):
        generate(missing, False, out, 4, 32, 10, 4, init_dir=str(tmp_path), save_degraded=str(tmp_path / "d"))
    assert not (tmp_path / "out").exists()


def test_generate_help_lists_restoration_flags(capsys):
    from tinyedm_amd.generate import main
    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--restore_scale", "--restore_gray", "--save_degraded", "--restore_report"):
        assert re.search(rf"(^|\s){flag}(\s|$)", out, re.M), flag
    import tinyedm.generate
    assert tinyedm.generate.main is main or callable(tinyedm.generate.main)


# ------------------------------------------------------------------ the C ABI
def test_new_entries_declared_in_header_and_lib():
    from tinyedm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    declared = set(re.findall(r"\b(edm_[a-z0-9_]+)\s*\(", hdr))
    for name in ("edm_degrade", "edm_project_denoised"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["edm_degrade"]) == 9 and len(_lib.SIGNATURES["edm_project_denoised"]) == 13
    for phrase in ("channels ascending", "bit for bit", "DEVICE pointer"):      # the contract is written down
        assert phrase in hdr
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    exported = set(re.findall(r"\bT (edm_[a-z0-9_]+)", nm.stdout))
    assert {"edm_degrade", "edm_project_denoised"} <= exported
