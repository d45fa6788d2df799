"""The adaptive solver, host side (no GPU): the fp64 numpy restatement tests/adaptive_ref.py is itself put to the test, so
that every condition tests/test_adaptive_solver_gpu.py leans on is checked here, on two analytic denoisers
(d = 48, B = 8, torch.manual_seed(0), sigma 80 -> 0.002, atol = rtol / 10):

 * Gaussian data N(0, 0.5^2 I): D(x, t) = x / (1 + 4 t^2), exact solution x(t) = x(T) sqrt((0.25 + t^2) / (0.25 + T^2));
 * a 4-component mixture with s = 0.1, its truth from the reference itself at rtol = 1e-9 (stored as
   tests/golden/adaptive_mixture_truth.npz for the GPU test, and checked against the recomputation here).

Errors are the per-sample RMS of the difference to the truth, in data units (the data has rms ~0.5).  Then the host
validation of AdaptiveSolver and of the generate flags, and the C ABI declarations."""
import math
import os
import re

import numpy as np
import pytest
import torch

import adaptive_ref as R
from tinyedm_amd import AdaptiveSolver, DeterministicSolver, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_, B_ = 48, 8
RTOLS = (1e-2, 1e-3, 1e-4)
SPAN = AdaptiveSolver().span()                      # (sigma_max, sigma_min, h0) as the fp32 table values
SPAN_UP = AdaptiveSolver().span(upwards=True)


def setting():
    """torch.manual_seed(0)'s stream: the mixture's means, then x0 ~ N(0, I), both fp64"""
    g = torch.Generator().manual_seed(0)
    means = 0.5 * torch.randn(4, D_, generator=g, dtype=torch.float64)
    x0 = torch.randn(B_, D_, generator=g, dtype=torch.float64)
    return means.numpy(), x0.numpy()


MIX_S, MIX_W = 0.1, (0.1, 0.2, 0.3, 0.4)


def gaussian(x, t):
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    return 0.25 / (0.25 + t * t) * x


def mixture(means):
    logw = np.log(np.array(MIX_W))

    def D(x, t):
        """the posterior mean E[y | y + t n = x] of the mixture"""
        v = MIX_S ** 2 + np.asarray(t, dtype=np.float64).reshape(-1, 1) ** 2          # [B, 1]
        d = x[:, None, :] - means[None]
        logp = logw[None] - 0.5 * (d * d).sum(-1) / v - 0.5 * means.shape[1] * np.log(v)
        p = np.exp(logp - logp.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        return (p[:, :, None] * (means[None] + (MIX_S ** 2 / v)[:, :, None] * d)).sum(axis=1)
    return D


def gaussian_exact(x0):
    T0, T1 = SPAN[0], SPAN[1]
    x_min = x0 * T0 * math.sqrt((0.25 + T1 ** 2) / (0.25 + T0 ** 2))
    return x_min + (0.0 - T1) * ((x_min - gaussian(x_min, np.full(len(x0), T1))) / T1)     # the closing Euler step


def rms(a, b):
    return np.sqrt(((np.asarray(a, dtype=np.float64) - b) ** 2).reshape(len(b), -1).mean(axis=1))


@pytest.fixture(scope="module")
def world(golden_dir):
    means, x0 = setting()
    mix = mixture(means)
    truth = R.solve(mix, x0, SPAN, rtol=1e-9, atol=1e-10, max_iterations=10 ** 6)
    assert (truth.status == R.DONE).all()
    dens = {"gaussian": (gaussian, gaussian_exact(x0)), "mixture": (mix, truth.x)}
    runs = {(n, r): R.solve(D, x0, SPAN, rtol=r, atol=r / 10, keep_states=True) for n, (D, _) in dens.items() for r in RTOLS}
    return x0, means, dens, runs


def test_stored_truth_is_the_reference_at_1e9(world, golden_dir):
    _, _, dens, _ = world
    g = np.load(os.path.join(golden_dir, "adaptive_mixture_truth.npz"))
    # the stored array is this computation on another host: libm's exp / log may differ in the last bit and with it an
    # accept decision near E = 1 somewhere in the 67 804 iterations.  Either run is within about rtol = 1e-9 of the ODE's
    # solution (the 0.2..1.9 rtol of the runs below), so the two differ by a few 1e-9 at the most; the smallest bound
    # the truth is used under is 4e-4
    assert np.abs(g["truth"] - dens["mixture"][1]).max() <= 1e-8
    assert np.array_equal(g["span"], np.array(SPAN))


@pytest.mark.parametrize("rtol", RTOLS)
@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_every_sample_finishes_within_tolerance(world, name, rtol):
    _, _, dens, runs = world
    r = runs[name, rtol]
    assert (r.status == R.DONE).all() and r.iterations <= 1024
    assert r.iterations == (r.accepted + r.rejected).max() and r.evaluations == 2 * r.iterations + 1
    e = rms(r.x, dens[name][1]).max()
    print(f"{name} rtol {rtol:g}: {r.iterations} iterations, worst rms error {e:.3g} = {e / rtol:.2f} rtol")
    assert e <= 4 * rtol, e


@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_error_falls_and_steps_grow_with_the_tolerance(world, name):
    _, _, dens, runs = world
    e = [rms(runs[name, r].x, dens[name][1]).max() for r in RTOLS]
    acc = [runs[name, r].accepted.min() for r in RTOLS]
    assert e[0] / e[1] >= 3 and e[1] / e[2] >= 3, e
    assert acc[0] < acc[1] < acc[2], acc


def test_mixture_samples_take_their_own_number_of_steps(world):
    _, _, _, runs = world
    for r in RTOLS:
        assert len(set(runs["mixture", r].accepted.tolist())) > 1


@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_a_sample_alone_gives_the_bits_of_the_batch(world, name):
    x0, _, dens, runs = world
    for b in (0, 5):
        alone = R.solve(dens[name][0], x0[b:b + 1], SPAN, rtol=1e-3, atol=1e-4)
        assert np.array_equal(alone.x[0], runs[name, 1e-3].x[b])
        assert alone.accepted[0] == runs[name, 1e-3].accepted[b] and alone.rejected[0] == runs[name, 1e-3].rejected[b]


@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_a_rejected_step_leaves_x_and_t_unchanged(world, name):
    _, _, _, runs = world
    trace = runs[name, 1e-3].trace
    seen = 0
    for (t, accept, E, x), (t_next, _, _, x_next) in zip(trace, trace[1:]):
        for b in np.flatnonzero(~accept):
            assert t_next[b] == t[b] and np.array_equal(x_next[b], x[b])
            seen += bool(t[b] != SPAN[1]) and not E[b] <= 1.0
        for b in np.flatnonzero(accept):
            assert t_next[b] < t[b] and E[b] <= 1.0
    assert seen >= B_           # every sample rejects at least the first proposal, the table's 80 -> 57


@pytest.mark.parametrize("rtol", RTOLS)
@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_invert_then_solve_returns_the_image(world, name, rtol):
    _, means, dens, _ = world
    g = np.random.default_rng(1)
    img = 0.5 * g.standard_normal((B_, D_)) if name == "gaussian" else \
        means[g.integers(0, 4, B_)] + MIX_S * g.standard_normal((B_, D_))
    kw = dict(rtol=rtol, atol=rtol / 10)
    lat = R.invert(dens[name][0], img, SPAN_UP, **kw)
    assert (lat.status == R.DONE).all() and (lat.t == SPAN[0]).all() and lat.evaluations == 2 * lat.iterations
    back = R.solve(dens[name][0], lat.x, SPAN, **kw)
    e = rms(back.x, img).max()
    print(f"{name} rtol {rtol:g}: round trip {e:.3g} = {e / rtol:.2f} rtol")
    assert e <= 8 * rtol, e


def test_the_snap_lands_on_t_end_exactly(world):
    _, _, _, runs = world
    for r in runs.values():
        assert (r.t == SPAN[1]).all()
    for dtype in (np.float64, np.float32):
        assert R.snap(dtype(1.0), dtype(-0.5), 0.5, dtype) == dtype(0.5)                # lands on it
        assert R.snap(dtype(1.0), dtype(-0.7), 0.5, dtype) == dtype(0.5)                # passes it
        assert R.snap(dtype(1.0), dtype(-0.4975), 0.5, dtype) == dtype(0.5)             # within 1 % of |h|
        assert R.snap(dtype(1.0), dtype(-0.49), 0.5, dtype) == dtype(dtype(1.0) + dtype(-0.49))
        assert R.snap(dtype(0.5), dtype(0.2), 1.0, dtype) == dtype(np.float64(dtype(0.5)) + np.float64(dtype(0.2)))
        assert R.snap(dtype(0.5), dtype(0.6), 1.0, dtype) == dtype(1.0)                 # upwards


def test_controller_rows():
    c = R.Controller()
    row = R.Row(1.0, 0.8, -0.2)
    ok, r = R.control(row, 0.25, 0.1, c)                    # well under 1: accepted, 0.9 / sqrt(0.25) = 1.8
    assert ok and r.t == 0.8 and r.accepted == 1 and math.isclose(r.h, -0.2 * 1.8) and not r.after_reject
    assert math.isclose(r.t1, 0.8 - 0.36)
    ok, r = R.control(row, 1e-12, 0.1, c)                   # the growth is capped at fac_max; the step then snaps
    assert ok and math.isclose(r.h, -1.0) and r.t1 == 0.1
    ok, r = R.control(row, 4.0, 0.1, c)                     # over 1: rejected, 0.9 / 2
    assert not ok and r.t == 1.0 and r.rejected == 1 and math.isclose(r.h, -0.09) and r.after_reject
    ok, r2 = R.control(r, 0.01, 0.1, c)                     # the step after a rejection does not grow
    assert ok and math.isclose(r2.h, r.t1 - r.t) and not r2.after_reject
    ok, r = R.control(row, float("nan"), 0.1, c)            # NaN: rejected at fac_min
    assert not ok and math.isclose(r.h, -0.04) and r.status == R.ACTIVE
    ok, r = R.control(R.Row(1.0, 0.1, -0.9), 0.5, 0.1, c)   # reaches t_end: done, t1 = t
    assert ok and r.status == R.DONE and r.t == 0.1 and r.t1 == 0.1
    assert R.control(r, 0.5, 0.1, c) == (False, r)          # and stays as it is
    ok, r = R.control(R.Row(1.0, 1.0 - 2e-6, -2e-6), 100.0, 0.1, c)     # under the floor: failed
    assert not ok and r.status == R.FAILED and r.t1 == r.t


# ------------------------------------------------------------------ host validation
def _never(*a, **k):
    raise AssertionError("nothing may be evaluated")


@pytest.mark.parametrize("kw,match", [
    ({"rtol": -1e-3}, "rtol"), ({"rtol": math.nan}, "rtol"), ({"atol": math.inf}, "atol"), ({"rtol": 0.0, "atol": 0.0}, "both"),
    ({"rtol": "1e-3"}, "rtol"), ({"max_iterations": 0}, "max_iterations"), ({"max_iterations": 2.5}, "max_iterations"),
    ({"safety": 0.0}, "safety"), ({"safety": 1.5}, "safety"), ({"fac_min": 1.0}, "fac_min"), ({"fac_max": 0.5}, "fac_max"),
    ({"fac_max": math.inf}, "finite"), ({"h_floor": -1.0}, "h_floor"), ({"num_steps": 1}, "num_steps"),
    ({"guidance": 2.0}, "needs a guide"), ({"guidance": math.nan, "guide": _never}, "finite"),
    ({"guidance": 2.0, "guide": _never, "guidance_interval": (0.1, 5.0)}, "guidance_interval"),
    ({"guidance_interval": (0.1, 5.0)}, "guidance_interval"), ({"sigma_min": 90.0}, "sigma_min"), ({"dtype": "float64"}, "float32"),
])
def test_invalid_settings_rejected(kw, match):
    with pytest.raises(ValueError, match=match):
        AdaptiveSolver(**kw)


def test_constructor_and_defaults():
    s = AdaptiveSolver()
    assert isinstance(s, DeterministicSolver)
    assert (s.rtol, s.atol, s.max_iterations, s.safety, s.fac_min, s.fac_max) == (1e-3, 1e-4, 1024, 0.9, 0.2, 5.0)
    assert s.last_stats is None
    ts = DeterministicSolver(num_steps=18).t_steps.tolist()
    assert s.span() == (ts[0], ts[17], ts[1] - ts[0]) and s.span(upwards=True) == (ts[17], ts[0], ts[16] - ts[17])
    assert AdaptiveSolver(32).span()[2] == DeterministicSolver(32).t_steps[1].item() - ts[0]
    with pytest.raises(TypeError):
        AdaptiveSolver(18, 0.002, 80.0, 7.0, None, 1e-3)        # the tolerances are keyword-only
    import tinyedm
    assert tinyedm.AdaptiveSolver is AdaptiveSolver and tinyedm.solvers.AdaptiveSolver is AdaptiveSolver
    s.rtol = -1.0                                               # plain attributes, checked again at every solve
    with pytest.raises(ValueError, match="rtol"):
        s.solve(_never, torch.zeros(1, 3, 4, 4))


@pytest.mark.parametrize("kw", [
    {"graph": True}, {"start_step": 3}, {"image": torch.zeros(1, 3, 4, 4)}, {"mask": torch.ones(4, 4)},
    {"degradation": object()}, {"measurement": torch.zeros(1, 3, 2, 2)}, {"operator": object()}, {"dps_scale": 1.0},
])
def test_solve_refuses_on_the_host(kw):
    # x0 is a host tensor: the refusal comes before the "no CPU path" error, so before any launch
    with pytest.raises(ValueError, match="not implemented for the adaptive solver"):
        AdaptiveSolver().solve(_never, torch.zeros(1, 3, 4, 4), **kw)


def test_invert_and_likelihood_refuse_on_the_host():
    s = AdaptiveSolver()
    for kw in ({"graph": True}, {"end_step": 2}):
        with pytest.raises(ValueError, match="not implemented for the adaptive solver"):
            s.invert(_never, torch.zeros(1, 3, 4, 4), **kw)
    with pytest.raises(ValueError, match="likelihood"):
        s.log_likelihood(_never, torch.zeros(1, 3, 4, 4))
    for call in (s.solve, s.invert):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(_never, torch.zeros(1, 3, 4, 4))


def test_ops_have_no_cpu_path():
    x = torch.zeros(2, 3, 4, 4)
    t = torch.ones(2)
    with pytest.raises(ValueError, match="CPU"):
        ops.adapt_euler(x, x, t, t)
    with pytest.raises(ValueError, match="CPU"):
        ops.adapt_commit(x, x.clone(), torch.ones(2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="point from"):
        ops.adapt_begin(2, 80.0, 0.002, 1.0, "cpu")
    assert [ops.adapt_chunks(n) for n in (1, 1024, 1025, 3072, 4099, 10 ** 6)] == [1, 1, 2, 3, 5, 64]


def test_the_library_states_the_chunk_rule():
    """edm_sample_chunks (host logic): the rule the kernels index `part` with, against its closed form; ops sizes the
    workspaces of the adaptive and the parallel solver with the library's value instead of a copy of the formula"""
    from tinyedm_amd import _lib
    for CHW in (1, 4, 5, 1024, 1025, 1028, 3072, 65536, 65540, 2 ** 31):
        want = min(((CHW + 3) // 4 + 255) // 256, ops.NLL_MAX_CHUNKS)
        assert _lib.call("edm_sample_chunks", CHW) == want, CHW
        assert ops.adapt_chunks(CHW) == want and ops.picard_chunks(CHW) == want, CHW
    assert ops.NLL_MAX_CHUNKS == 64 and ops.adapt_chunks(2 ** 31) == 64


GEN = dict(ckpt_path="missing.ckpt", load_ema=False, num_samples=4, image_size=32, num_classes=10, batch_size=4)


@pytest.mark.parametrize("kw,match", [
    ({"guidance_interval": (0.1, 5.0)}, "--guidance_interval"), ({"S_churn": 5.0}, "S_churn"),
    ({"init_dir": "d"}, "--init_dir without --invert_to"), ({"init_dir": "d", "mask_box": (1, 1, 5, 5)}, "--mask_box"),
    ({"init_dir": "d", "restore_scale": 4}, "--restore_scale"), ({"init_dir": "d", "restore_gray": True}, "--restore_scale"),
    ({"init_dir": "d", "dps_scale": 1.0, "blur_std": 1.0}, "--dps_scale"),
    ({"init_dir": "d", "likelihood_to": "o.json"}, "--likelihood_to"),
    ({"init_dir": "d", "invert_to": "o.pt", "start_step": 2}, "--start_step"),
    ({"rtol": -1.0}, "--rtol"), ({"atol": math.nan}, "--atol"), ({"rtol": 0.0, "atol": 0.0}, "both"),
    ({"max_iterations": 0}, "--max_iterations"),
])
def test_generate_refuses_before_anything_is_loaded(tmp_path, kw, match):
    from tinyedm_amd.generate import generate
    with pytest.raises(ValueError, match=match):
        generate(output_dir=str(tmp_path / "out"), solver="adaptive", **{**GEN, **kw})
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("flag", ["rtol", "atol", "max_iterations", "solver_report"])
@pytest.mark.parametrize("solver", ["heun", "dpmpp"])
def test_generate_adaptive_flags_need_the_adaptive_solver(tmp_path, solver, flag):
    from tinyedm_amd.generate import generate
    value = {"rtol": 1e-3, "atol": 1e-4, "max_iterations": 10, "solver_report": "r.json"}[flag]
    with pytest.raises(ValueError, match=f"--{flag} needs --solver adaptive"):
        generate(output_dir=str(tmp_path / "out"), solver=solver, **GEN, **{flag: value})


def test_generate_cli_flags(capsys, tmp_path):
    from tinyedm_amd.generate import _validate, main
    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--rtol", "--atol", "--max_iterations", "--solver_report"):
        assert re.search(rf"(^|\s){flag}(\s|$)", out, re.M), flag
    assert "adaptive" in out
    args = ["--ckpt_path", "missing.ckpt", "--output_dir", str(tmp_path / "out"), "--num_samples", "4", "--image_size", "32",
            "--num_classes", "10", "--batch_size", "4", "--solver", "adaptive"]
    with pytest.raises(ValueError, match="S_churn"):
        main(args + ["--S_churn", "5"])
    with pytest.raises(SystemExit):
        main(args + ["--guidance_interval", "0.1", "5"])
    assert not (tmp_path / "out").exists()
    # what it accepts: plain, guided, and --invert_to
    base = dict(solver="adaptive", S_churn=0.0, init_dir=None, start_step=0, num_steps=18, mask_box=None, invert_to=None,
                likelihood_to=None, network_dtype="f32x3", num_probes=1, dequantize=False, image_size=32, dps_scale=None,
                blur_std=None, blur_radius=2, measurement_noise=0.0, restore_scale=1, restore_gray=False, save_degraded=None,
                restore_report=None, labels_to=None, guided=False)
    assert _validate(**base, rtol=1e-2, solver_report="r.json") == (False, False)
    assert _validate(**{**base, "guided": True, "labels_to": "l.json"}) == (False, False)
    assert _validate(**{**base, "init_dir": "d", "invert_to": "o.pt"}) == (False, False)


def test_adaptive_declared_in_header_and_lib():
    from tinyedm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    declared = set(re.findall(r"\b(edm_[a-z0-9_]+)\s*\(", hdr))
    for name in ("edm_adapt_begin", "edm_adapt_euler", "edm_adapt_correct", "edm_adapt_control", "edm_adapt_commit"):
        assert name in declared and name in _lib.SIGNATURES
    assert int(re.search(r"#define EDM_ADAPT_ROWS (\d+)", hdr).group(1)) == ops.ADAPT_ROWS
