"""Diffusion posterior sampling without a device: the fp64 restatements of tests/dps_ref.py are what they claim to be (the
operators' adjoint identities, a DPS loop that does pull the sample towards the measurement on the cases the GPU test runs),
and the argument validation of solve(operator=, measurement=, dps_scale=), GaussianBlur and input_vjp that needs no GPU."""
import pytest
import torch

import dps_ref as P
import restoration_ref as R


def _inner(a, b):
    return (a.double() * b.double()).sum().item()


@pytest.mark.parametrize("radius,std", [(1, 0.7), (2, 1.0), (4, 2.5)])
@pytest.mark.parametrize("shape", [(3, 3, 16, 16), (2, 3, 6, 10)])
def test_blur_is_self_adjoint(radius, std, shape):
    g = torch.Generator().manual_seed(radius)
    u = torch.randn(shape, generator=g, dtype=torch.float64)
    v = torch.randn(shape, generator=g, dtype=torch.float64)
    op = P.Blur(std, radius)
    assert abs(sum(op.taps) - 1.0) <= 1e-15
    lhs, rhs = _inner(op.measure(u), v), _inner(u, op.adjoint(v))
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (lhs, rhs)
    # zero padding: a constant image loses mass at the border, the interior keeps it
    one = op.measure(torch.ones(1, 1, 16, 16, dtype=torch.float64))
    assert abs(one[0, 0, 8, 8].item() - 1.0) <= 1e-14 and one[0, 0, 0, 0].item() < 1.0


@pytest.mark.parametrize("scale,gray", R.OPERATORS)
def test_box_adjoint_identity(scale, gray):
    g = torch.Generator().manual_seed(scale)
    u = torch.randn(3, 3, 16, 16, generator=g, dtype=torch.float64)
    op = P.Box(scale, gray)
    v = torch.randn(op.measure(u).shape, generator=g, dtype=torch.float64)
    lhs, rhs = _inner(op.measure(u), v), _inner(u, op.adjoint(v, 3))
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (lhs, rhs)
    # A+ = n A^T
    assert R.rel(op.adjoint(v, 3) * R.block_terms(scale, gray, 3), R.pinv(v, scale, gray, 3)) <= 1e-15


def _schedule(n=P.ANALYTIC_STEPS, smin=0.002, smax=80.0, rho=7.0):
    i = torch.arange(n, dtype=torch.float64)
    t = (smax ** (1 / rho) + i / (n - 1) * (smin ** (1 / rho) - smax ** (1 / rho))) ** rho
    return torch.cat([t, torch.zeros(1, dtype=torch.float64)])


@pytest.mark.parametrize("name", sorted(P.ANALYTIC_CASES))
def test_reference_dps_lowers_the_residual(name):
    """the comparison of tests/test_dps_gpu.py is meaningful: on its seeds and scales the reference loop ends closer to y"""
    spec, scale = P.ANALYTIC_CASES[name]
    op = P.analytic_operator(spec)
    x0, y = P.analytic_inputs(spec)
    t = _schedule()
    res = {}
    for z in (0.0, scale):
        x = P.solve_dps(P.gaussian_vjp, R.gaussian, t, x0, op, y, z)
        assert torch.isfinite(x).all()
        res[z] = (op.measure(x) - y).flatten(1).norm(dim=1)
    plain = R.solve_heun(R.gaussian, t, x0)
    assert R.rel(P.solve_dps(P.gaussian_vjp, R.gaussian, t, x0, op, y, 0.0), plain) <= 1e-13
    print(f"{name}: ||A x - y|| {res[0.0].tolist()} -> {res[scale].tolist()}")
    assert bool((res[scale] < 0.8 * res[0.0]).all()), (res[0.0], res[scale])


def test_autograd_vjp_is_the_gaussian_vjp():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 8, 8, generator=g, dtype=torch.float64)
    v = torch.randn(2, 3, 8, 8, generator=g, dtype=torch.float64)
    s = torch.tensor(1.7, dtype=torch.float64)
    D, pull = P.autograd_vjp(R.gaussian)(x, s)
    D2, pull2 = P.gaussian_vjp(x, s)
    assert R.rel(D, D2) <= 1e-15 and R.rel(pull(v), pull2(v)) <= 1e-15


def test_update_restatement_keeps_x_where_the_norm_is_zero():
    x = torch.randn(2, 1, 2, 2, dtype=torch.float64)
    g = torch.ones_like(x)
    out = P.update(x, g, torch.tensor([0.0, 2.0], dtype=torch.float64), 3.0)
    assert torch.equal(out[0], x[0]) and torch.allclose(out[1], x[1] + 1.5)


# ------------------------------------------------------------------ argument validation that needs no device
def _gauss(x, s, labels=None):
    return R.gaussian(x, s)


def test_solve_refuses_bad_posterior_arguments():
    import tinyedm_amd as T
    x0 = torch.randn(2, 3, 8, 8)
    blur, box = T.GaussianBlur(1.0, 2), T.LinearDegradation(2)
    y = torch.randn(2, 3, 8, 8)
    yb = torch.randn(2, 3, 4, 4)
    sol = T.DeterministicSolver(num_steps=4)
    cases = {
        "degradation": dict(degradation=box, operator=blur, measurement=y),
        "graph=True": dict(operator=blur, measurement=y, graph=True),
        "mask": dict(operator=blur, measurement=y, image=y, mask=torch.ones(8, 8)),
        "dps_scale": dict(operator=blur, measurement=y, dps_scale=-1.0),
        "measurement must have shape": dict(operator=blur, measurement=yb),
        "go together": dict(operator=blur),
        "needs operator": dict(dps_scale=1.0),
        "must be a LinearDegradation or a GaussianBlur": dict(operator="blur", measurement=y),
    }
    for word, kw in cases.items():
        with pytest.raises(ValueError, match=word):
            sol.solve(_gauss, x0, **kw)
    with pytest.raises(ValueError, match="measurement must have shape"):
        sol.solve(_gauss, x0, operator=box, measurement=y)
    with pytest.raises(ValueError, match="dps_scale"):
        sol.solve(_gauss, x0, operator=box, measurement=yb, dps_scale=float("nan"))
    with pytest.raises(ValueError, match="guide"):
        T.DeterministicSolver(num_steps=4, guide=_gauss, guidance=2.0).solve(_gauss, x0, operator=blur, measurement=y)
    with pytest.raises(ValueError, match="MultistepSolver"):
        T.MultistepSolver(num_steps=4).solve(_gauss, x0, operator=blur, measurement=y)
    # StochasticSolver takes the arguments: it gets as far as the device check
    with pytest.raises(RuntimeError, match="GPU tensor"):
        T.StochasticSolver(num_steps=4).solve(_gauss, x0, operator=blur, measurement=y, dps_scale=0.5)


@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
def test_posterior_sampling_needs_the_bf16_path(dtype):
    import tinyedm_amd as T
    den = T.Denoiser(3, 3, ("Enc",), ("Dec",), (32,), (32,), (True,), 0.0, 0.5, 0.3, 0.3, 32, 2).eval()
    den.set_eval_dtype(dtype)
    x0 = torch.randn(1, 3, 8, 8)
    with pytest.raises(ValueError, match="--network_dtype bf16"):
        T.DeterministicSolver(num_steps=4).solve(den, x0, operator=T.GaussianBlur(), measurement=x0)
    with pytest.raises(ValueError, match=r"set_eval_dtype\(\"bf16\"\)"):
        T.input_vjp(den, x0, torch.ones(1), torch.zeros(1, 32), x0)


def test_gaussian_blur_validation_and_taps():
    import tinyedm_amd as T
    for bad in (dict(radius=0), dict(radius=5), dict(radius=True), dict(std=0.0), dict(std=float("inf")), dict(radius=1.5)):
        with pytest.raises(ValueError):
            T.GaussianBlur(**{"std": 1.0, "radius": 2, **bad})
    b = T.GaussianBlur(1.3, 3)
    assert len(b.taps) == 7 and b.taps == b.taps[::-1]
    ref = P.gaussian_taps(1.3, 3)
    assert max(abs(a - c) for a, c in zip(b.taps, ref)) <= 2.0 ** -25
    assert b.measurement_shape((2, 3, 6, 10)) == (2, 3, 6, 10)
    with pytest.raises(ValueError):
        b.measurement_shape((3, 6, 10))
    with pytest.raises(ValueError, match="channels"):
        T.LinearDegradation(2).adjoint(torch.zeros(1, 3, 4, 4), 0)
    with pytest.raises(ValueError, match="no measurement"):
        T.LinearDegradation(2, True).adjoint(torch.zeros(1, 3, 4, 4), 3)


CLI = ["--output_dir", "unused", "--config_name", "cifar10_cond", "--num_samples", "4", "--batch_size", "4", "--num_steps", "4",
       "--num_classes", "10", "--image_size", "32", "--init_dir", "photos"]


@pytest.mark.parametrize("extra,word", [
    (["--dps_scale", "1.0", "--blur_std", "1.5"], "--network_dtype bf16"),
    (["--blur_std", "1.5", "--network_dtype", "bf16"], "--blur_std needs --dps_scale"),
    (["--measurement_noise", "0.1", "--restore_scale", "4"], "--measurement_noise needs --dps_scale"),
    (["--dps_scale", "1.0", "--network_dtype", "bf16"], "ONE measurement operator"),
    (["--dps_scale", "1.0", "--network_dtype", "bf16", "--blur_std", "1.0", "--restore_gray"], "ONE measurement operator"),
    (["--dps_scale", "-1", "--network_dtype", "bf16", "--blur_std", "1.0"], "--dps_scale must be"),
    (["--dps_scale", "1", "--network_dtype", "bf16", "--blur_std", "1.0", "--blur_radius", "5"], "radius"),
    (["--dps_scale", "1", "--network_dtype", "bf16", "--blur_std", "1.0", "--solver", "dpmpp"], "--solver heun"),
    (["--dps_scale", "1", "--network_dtype", "bf16", "--blur_std", "1.0", "--guide_unconditional", "--guidance", "2"], "guide"),
    (["--dps_scale", "1", "--network_dtype", "bf16", "--blur_std", "1.0", "--mask_box", "1", "1", "4", "4"], "exclusive"),
])
def test_generate_refuses_on_the_host(capsys, extra, word):
    """the argument parser exits with status 2 before anything is loaded or launched"""
    from tinyedm_amd import generate as G
    with pytest.raises(SystemExit) as e:
        G.main(CLI + extra)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_generate_restore_flags_keep_meaning_ddnm():
    """without --dps_scale nothing about --restore_* changes: the checks return 'restoring, not posterior'"""
    from tinyedm_amd import generate as G
    assert G._check_posterior(None, None, 2, 0.0, 4, False, "f32x3", "heun", False) is False
    assert G._check_restoration("photos", 4, False, None, None, None, None, None, 32) is True
    assert G._check_posterior(1.0, None, 2, 0.0, 4, False, "bf16", "heun", False) is True
    assert G._check_posterior(0.0, 1.0, 2, 0.1, 1, False, "bf16", "heun", False) is True
    assert G._check_restoration("photos", 1, False, "d", "r.json", None, None, None, 32, blur=True) is True


def test_input_vjp_of_a_foreign_model_is_plain_autograd():
    """a model that is not this library's goes through torch.autograd.grad on its forward (here: on the CPU, in fp64)"""
    import tinyedm_amd as T
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 8, 8, generator=g)
    v = torch.randn(2, 3, 8, 8, generator=g)
    s = torch.tensor(0.9)
    D, gx = T.input_vjp(_gauss, x, s, None, v)
    c = R.SD ** 2 / (R.SD ** 2 + 0.9 ** 2)
    assert D.dtype == gx.dtype == torch.float32 and not D.requires_grad
    assert R.rel(D, R.gaussian(x.double(), s.double())) <= 1e-6 and R.rel(gx, c * v.double()) <= 1e-6
    with pytest.raises(ValueError, match="cotangent must have D's shape"):
        T.input_vjp(_gauss, x, s, None, v[:1])
    with pytest.raises(ValueError, match="cotangent is required"):
        T.input_vjp(_gauss, x, s, None)
