"""Diffusion posterior sampling on the GPU: the measurement-side kernels against fp64 restatements (tests/dps_ref.py) and their
exact properties, DPS solves of the analytic Gaussian denoiser (J is a known scalar: the whole loop is closed-form) and of
the tiny networks against the same loop composed from the CPU oracle, dps_scale = 0 == the plain solve, the refused
combinations, and the generate CLI end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dps_ref as P
import restoration_ref as R
from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs
from parity_log import record

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------ 1. kernels vs fp64
SHAPES = [(7, 3, 32, 32), (5, 3, 6, 10), (3, 4, 64, 64)]


def _data(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.3 + 0.5 * torch.randn(shape, generator=g), 0.3 + 0.5 * torch.randn(shape, generator=g)


@pytest.mark.parametrize("radius", [1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_blur2d_vs_fp64(ops, shape, radius):
    import tinyedm_amd as T
    x, _ = _data(shape, radius)
    blur = T.GaussianBlur(0.8 * radius, radius)
    taps = blur.taps
    ref = P.blur(x.double(), [float(t) for t in taps])      # the same fp32 taps, in fp64
    got = ops.blur2d(x.to(DEV), taps)
    terms = (2 * radius + 1) ** 2
    lim = (terms + 3) * U * x.abs().max().item()
    e = (got.cpu().double() - ref).abs().max().item()
    print(f"blur2d {shape} radius {radius}: max abs {e:.3e} (limit {lim:.3e})")
    record(f"dps/blur2d_{'x'.join(map(str, shape))}_r{radius}_vs_fp64", e, lim)
    assert got.shape == x.shape and e <= lim, (e, lim)
    assert torch.equal(blur.measure(x.to(DEV)), got) and torch.equal(blur.adjoint(x.to(DEV), shape[1]), got)
    # a plane's result depends on nothing but the plane
    assert torch.equal(ops.blur2d(x[1:2, 2:3].contiguous().to(DEV), taps), got[1:2, 2:3])
    # self-adjoint on the device too: <A u, v> = <u, A v> to the rounding of the sums
    v = _data(shape, 9)[1].to(DEV)
    lhs = (got.double() * v.double()).sum().item()
    rhs = (x.to(DEV).double() * ops.blur2d(v, taps).double()).sum().item()
    assert abs(lhs - rhs) <= 2 * lim * x.numel() * max(v.abs().max().item(), x.abs().max().item()), (lhs, rhs)


@pytest.mark.parametrize("scale,gray", [(2, False), (4, True), (1, True)])
def test_degrade_adjoint_vs_fp64(ops, scale, gray):
    import tinyedm_amd as T
    shape = (5, 3, 8, 12)
    g = torch.Generator().manual_seed(scale)
    r = torch.randn(R.degrade(torch.zeros(shape), scale, gray).shape, generator=g)
    got = T.LinearDegradation(scale, gray).adjoint(r.to(DEV), 3).cpu()
    ref = P.degrade_adjoint(r.double(), scale, gray, 3)
    lim = 2 * U * r.abs().max().item()          # 1 / n in fp32 and one product
    assert got.shape == shape and (got.double() - ref).abs().max().item() <= lim
    # the adjoint identity against the device's own A
    u = torch.randn(shape, generator=g).to(DEV)
    lhs = (T.LinearDegradation(scale, gray).measure(u).double() * r.to(DEV).double()).sum().item()
    rhs = (u.double() * got.to(DEV).double()).sum().item()
    n = R.block_terms(scale, gray, 3)
    assert abs(lhs - rhs) <= 2 * (n + 3) * U * u.numel() * u.abs().max().item() * r.abs().max().item(), (lhs, rhs)


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_residual_and_update_vs_fp64(ops, shape):
    y, AD = _data(shape, 3)
    r, nrm = ops.dps_residual(y.to(DEV), AD.to(DEV))
    r_ref, n_ref = P.residual(y.double(), AD.double())
    n = y[0].numel()
    big = max(y.abs().max().item(), AD.abs().max().item())
    assert (r.cpu().double() - r_ref).abs().max().item() <= U * 2 * big
    # the norm: n squares summed (each term carries the subtraction's rounding twice), one square root
    e = ((nrm.cpu().double() - n_ref).abs() / n_ref).max().item()
    lim = (n + 3) * U
    print(f"dps_residual {shape}: norm rel {e:.3e} (limit {lim:.3e})")
    record(f"dps/residual_norm_{'x'.join(map(str, shape))}_vs_fp64", e, lim)
    assert e <= lim, (e, lim)
    # bit-identical across runs and independent of B
    r2, nrm2 = ops.dps_residual(y.to(DEV), AD.to(DEV))
    assert torch.equal(r, r2) and torch.equal(nrm, nrm2)
    for b in (0, shape[0] - 1):
        assert torch.equal(ops.dps_residual(y[b:b + 1].to(DEV), AD[b:b + 1].to(DEV))[1], nrm[b:b + 1])
    # the update
    x, g = _data(shape, 4)
    scale = 1.7
    got = ops.dps_update(x.to(DEV), g.to(DEV), nrm, scale)
    ref = P.update(x.double(), g.double(), nrm.cpu().double(), scale)
    lim = (2 + 3) * U * max(x.abs().max().item(), (scale / nrm.min().item()) * g.abs().max().item())
    e = (got.cpu().double() - ref).abs().max().item()
    record(f"dps/update_{'x'.join(map(str, shape))}_vs_fp64", e, lim)
    assert e <= lim, (e, lim)
    # a zero norm or a zero scale keeps x bit for bit
    nz = nrm.clone()
    nz[0] = 0.0
    kept = ops.dps_update(x.to(DEV), g.to(DEV), nz, scale)
    assert torch.equal(kept[0], x[0].to(DEV)) and torch.equal(kept[1:], got[1:])
    assert torch.equal(ops.dps_update(x.to(DEV), g.to(DEV), nrm, 0.0), x.to(DEV))
    with pytest.raises(ValueError):
        ops.dps_update(x.to(DEV), g.to(DEV), nrm, -1.0)


# ------------------------------------------------------------------ 2. the analytic Gaussian denoiser
def _gaussian(x, s, labels=None):
    s = s.double()
    return (R.MU + R.SD ** 2 / (R.SD ** 2 + s * s) * (x.double() - R.MU)).float()


def _operator(spec):
    import tinyedm_amd as T
    return T.LinearDegradation(spec[1], spec[2]) if spec[0] == "box" else T.GaussianBlur(spec[1], spec[2])


def _ref_operator(spec, op):
    """the fp64 restatement with the device operator's own fp32 taps"""
    return P.Box(spec[1], spec[2]) if spec[0] == "box" else P.Blur(spec[1], spec[2], taps=[float(t) for t in op.taps])


def _lift(ops, sol, x0_shape, solve_index, dtype):
    """the churn of a StochasticSolver with the noise the GPU kernel draws (tests/test_restoration_gpu.py)"""
    s = sol.churn_schedule()
    rec = ops.churn_record(sol.seed, solve_index, DEV)
    t = sol.t_steps.to(dtype)

    def lift(x, i):
        if not s.gamma[i] > 0:
            return x, t[i]
        noise = ops.heun_churn(torch.zeros(x0_shape, device=DEV), 1.0, rec, i).cpu().to(dtype)
        return x + s.c[i] * noise, torch.as_tensor(s.t_hat[i], dtype=dtype)
    return lift


@pytest.mark.parametrize("solver", ["heun", "stochastic"])
@pytest.mark.parametrize("name", sorted(P.ANALYTIC_CASES))
def test_gaussian_denoiser_dps_is_closed_form(ops, name, solver):
    import tinyedm_amd as T
    spec, scale = P.ANALYTIC_CASES[name]
    op = _operator(spec)
    ref_op = _ref_operator(spec, op)
    x0, y = P.analytic_inputs(spec)
    if solver == "heun":
        sol = T.DeterministicSolver(num_steps=P.ANALYTIC_STEPS)
    else:
        sol = T.StochasticSolver(num_steps=P.ANALYTIC_STEPS, S_churn=20.0, S_min=0.05, S_max=50.0, seed=77)
    sol.solve_index = 3
    t32, t64 = sol.t_steps, sol.t_steps.double()
    lift64 = _lift(ops, sol, x0.shape, 3, torch.float64) if solver == "stochastic" else None
    lift32 = _lift(ops, sol, x0.shape, 3, torch.float32) if solver == "stochastic" else None
    ref = P.solve_dps(P.gaussian_vjp, R.gaussian, t64, x0, ref_op, y, scale, lift64)
    D32 = lambda x, s: _gaussian(x, s)
    cpu32 = P.solve_dps(P.autograd_vjp(D32), D32, t32, x0.float(), ref_op, y.float(), scale, lift32)
    assert cpu32.dtype == torch.float32
    e32 = R.rel(cpu32, ref)
    lim = max(4.0 * e32, 1e-6)          # the bound of the restoration test's analytic case: 4x the CPU fp32 composition
    x_hip = sol.solve(_gaussian, x0.float().to(DEV), operator=op, measurement=y.float().to(DEV), dps_scale=scale).cpu()
    assert sol.solve_index == 3 + (solver == "stochastic")     # (a churned solve uses up its noise, as ever)
    e = R.rel(x_hip, ref)
    print(f"gaussian DPS {solver} {name}: rel {e:.3e} (CPU fp32 composition {e32:.3e}, limit {lim:.3e})")
    record(f"dps/gaussian_{solver}_{name}_vs_fp64", e, lim)
    assert e <= lim, (e, lim)
    sol.solve_index = 3
    x_plain = sol.solve(_gaussian, x0.float().to(DEV)).cpu()
    res = lambda x: (ref_op.measure(x.double()) - y).flatten(1).norm(dim=1)
    assert bool((res(x_hip) < 0.8 * res(x_plain)).all())         # the measurement pulled the sample


# ------------------------------------------------------------------ 3. tiny networks against the oracle's composition
def _edm(Pm, ecfg, dcfg, dtype="bf16"):
    import tinyedm_amd as T
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), dcfg.dropout_rate,
                     dcfg.sigma_data, dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    emb.load_state_dict({k[len("embedding."):]: v for k, v in Pm.items() if k.startswith("embedding.")}, strict=True)
    den.load_state_dict({k[len("denoiser."):]: v for k, v in Pm.items() if k.startswith("denoiser.")}, strict=True)
    den.set_eval_dtype(dtype)
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                  steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01)
    return model.to(DEV).eval()


SCHED = dict(num_steps=4, sigma_min=0.05, sigma_max=10.0, rho=5.0)


@pytest.fixture(scope="module")
def tiny():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    em, dm = tiny_cfgs(10)
    Pm = O.init_params(em, dm, torch.Generator().manual_seed(7), gains_nonzero=True)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 3, 8, 8, generator=g)
    labels = torch.randint(0, 10, (2,), generator=g)
    image = 0.5 * torch.randn(2, 3, 8, 8, generator=g)
    return _edm(Pm, em, dm), (Pm, em, dm), x0, labels, image


def _oracle_fn(Pm, em, dm, labels, bf16):
    def fn(x, s):
        sig = torch.as_tensor(s, dtype=torch.float32).reshape(-1).expand(x.shape[0])
        return O.edm_forward(Pm, em, dm, x, sig, labels, bf16=bf16).float()
    return fn


@pytest.mark.parametrize("name", ["box", "blur"])
def test_tiny_network_dps_vs_oracle_composition(ops, tiny, name):
    """d_ref = the distance between the oracle's bf16 and fp32 compositions of the same 4-step DPS loop (oracle forward,
    oracle autograd, dps_ref operators); the HIP solve may be at most 2 d_ref from either"""
    import tinyedm_amd as T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    model, (Pm, em, dm), x0, labels, image = tiny
    spec = ("box", 2, False) if name == "box" else ("blur", 1.0, 2)
    op = _operator(spec)
    ref_op = _ref_operator(spec, op)
    g = torch.Generator().manual_seed(11)
    y = ref_op.measure(image)
    y = (y + 0.05 * torch.randn(y.shape, generator=g)).float()
    sol = T.DeterministicSolver(**SCHED)
    scale = 1.0
    x_hip = sol.solve(model, x0.to(DEV), labels.to(DEV), operator=op, measurement=y.to(DEV), dps_scale=scale).cpu()
    outs = {}
    for bf16 in (False, True):
        fn = _oracle_fn(Pm, em, dm, labels, bf16)
        with torch.no_grad():
            outs[bf16] = P.solve_dps(P.autograd_vjp(fn), fn, sol.t_steps, x0, ref_op, y, scale)
    d_ref = R.rel(outs[True], outs[False])
    d32, d16 = R.rel(x_hip, outs[False]), R.rel(x_hip, outs[True])
    print(f"tiny DPS {name}: d_ref (oracle bf16 vs fp32) {d_ref:.3e}; HIP vs fp32 {d32:.3e}, vs bf16 {d16:.3e}")
    record(f"dps/tiny_{name}_d_ref_oracle_bf16_vs_fp32", d_ref, 2 * d_ref)
    record(f"dps/tiny_{name}_hip_vs_fp32_oracle", d32, 2 * d_ref)
    record(f"dps/tiny_{name}_hip_vs_bf16_oracle", d16, 2 * d_ref)
    assert d32 <= 2 * d_ref and d16 <= 2 * d_ref, (d32, d16, d_ref)
    x_plain = sol.solve(model, x0.to(DEV), labels.to(DEV)).cpu()
    assert R.rel(x_plain, outs[False]) > 2 * max(d32, d_ref)        # the measurement mattered


# ------------------------------------------------------------------ 4. dps_scale = 0, determinism, refusals
@pytest.mark.parametrize("solver", ["heun", "stochastic"])
def test_zero_scale_is_the_plain_solve(tiny, solver):
    import tinyedm_amd as T
    model, _, x0, labels, image = tiny
    mk = (lambda: T.DeterministicSolver(**SCHED)) if solver == "heun" else \
        (lambda: T.StochasticSolver(**SCHED, S_churn=10.0, S_min=0.1, S_max=8.0, seed=5))
    x0d, lab = x0.to(DEV), labels.to(DEV)
    for op in (T.GaussianBlur(1.0, 2), T.LinearDegradation(2), T.LinearDegradation(1, True)):
        y = op.measure(image.to(DEV))
        plain = mk().solve(model, x0d, lab)
        assert torch.equal(mk().solve(model, x0d, lab, operator=op, measurement=y, dps_scale=0.0), plain)
        a = mk().solve(model, x0d, lab, operator=op, measurement=y, dps_scale=0.7)
        b = mk().solve(model, x0d, lab, operator=op, measurement=y, dps_scale=0.7)
        assert torch.equal(a, b) and not torch.equal(a, plain) and torch.isfinite(a).all()


def test_refused_combinations(tiny):
    import tinyedm_amd as T
    model, _, x0, labels, image = tiny
    x0d, lab, img = x0.to(DEV), labels.to(DEV), image.to(DEV)
    blur, box = T.GaussianBlur(1.0, 1), T.LinearDegradation(2)
    y = blur.measure(img)
    sol = T.DeterministicSolver(**SCHED)
    for word, kw in {"degradation": dict(degradation=box, operator=blur, measurement=y),
                     "graph=True": dict(operator=blur, measurement=y, graph=True),
                     "mask": dict(operator=blur, measurement=y, image=img, mask=torch.ones(8, 8, device=DEV)),
                     "dps_scale": dict(operator=blur, measurement=y, dps_scale=-0.5),
                     "measurement must have shape": dict(operator=box, measurement=y)}.items():
        with pytest.raises(ValueError, match=word):
            sol.solve(model, x0d, lab, **kw)
    with pytest.raises(ValueError, match="guide"):
        T.DeterministicSolver(**SCHED, guide="unconditional", guidance=2.0).solve(model, x0d, lab, operator=blur, measurement=y)
    with pytest.raises(ValueError, match="MultistepSolver"):
        T.MultistepSolver(**SCHED).solve(model, x0d, lab, operator=blur, measurement=y)
    for dtype in ("f32", "f32x3"):
        model.denoiser.set_eval_dtype(dtype)
        try:
            with pytest.raises(ValueError, match="--network_dtype bf16"):
                sol.solve(model, x0d, lab, operator=blur, measurement=y)
        finally:
            model.denoiser.set_eval_dtype("bf16")
    # nothing was left behind: the plain solve is still the plain solve
    assert torch.equal(sol.solve(model, x0d, lab), T.DeterministicSolver(**SCHED).solve(model, x0d, lab))


# ------------------------------------------------------------------ 5. generate CLI
CLI = ["--config_name", "cifar10_cond", "--num_samples", "4", "--batch_size", "4", "--num_steps", "4", "--num_classes",
       "10", "--image_size", "32", "--num_workers", "0"]


def _generate(out, *extra, ok=True):
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "generate.py"), "--output_dir", str(out), *CLI, *extra]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr[-2000:]
    return r


def _load(d):
    from PIL import Image
    return np.stack([np.asarray(Image.open(os.path.join(d, f"{i}.png"))).astype(np.int64) for i in range(4)])


def test_generate_cli_posterior_sampling(ops, tmp_path):
    _generate(tmp_path / "plain", "--network_dtype", "bf16")
    plain = _load(tmp_path / "plain")
    noise = 0.05
    _generate(tmp_path / "dps", "--init_dir", str(tmp_path / "plain"), "--dps_scale", "1.0", "--blur_std", "1.5",
              "--blur_radius", "3", "--measurement_noise", str(noise), "--network_dtype", "bf16", "--restore_report",
              str(tmp_path / "r.json"), "--save_degraded", str(tmp_path / "d"))
    out, deg = _load(tmp_path / "dps"), _load(tmp_path / "d")
    rep = json.load(open(tmp_path / "r.json"))
    print(f"DPS deblurring report: {rep}")
    assert out.shape == deg.shape == (4, 32, 32, 3)
    assert rep["measurement_noise"] == noise and rep["dps_scale"] == 1.0 and rep["blur_std"] == 1.5 and rep["num_images"] == 4
    assert np.isfinite(rep["measurement_rms"]) and rep["measurement_rms"] > 0
    assert np.isfinite(rep["psnr_restored"]) and np.isfinite(rep["psnr_degraded"])
    assert all((out[i] != plain[i]).any() and (deg[i] != plain[i]).any() for i in range(4))
    # (the command line's refusals need no device: tests/test_dps_cpu.py)
