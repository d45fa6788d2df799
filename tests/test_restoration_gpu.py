"""Zero-shot restoration (DDNM) on the GPU: the two kernels against an fp64 restatement and their exact identities, the
projected solves of the tiny networks against the CPU composition (tests/restoration_ref.py), measurement consistency
of the results, the analytic Gaussian denoiser (where the ODE decouples and pins the whole plumbing), eager == hipGraph
and the graph cache, and the generate CLI end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

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


def _dev(t, offset=0):
    """t on the device, `offset` floats behind a 16-byte boundary (offset 1: the element-by-element path)"""
    buf = torch.empty(t.numel() + offset, device=DEV)
    out = buf[offset:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 * offset and out.is_contiguous()
    return out


# ------------------------------------------------------------------ 1. kernels vs an fp64 restatement
KERNEL_CASES = [((7, 3, 32, 32), s, g, 0) for s in (2, 4, 8) for g in (False, True)] + \
    [((3, 4, 64, 64), 8, False, 0), ((5, 3, 6, 10), 2, False, 0), ((2, 8, 8, 8), 1, True, 0), ((7, 3, 32, 32), 4, False, 1),
     ((7, 3, 32, 32), 2, True, 1)]


@pytest.mark.parametrize("shape,scale,gray,offset", KERNEL_CASES,
                         ids=[f"{'x'.join(map(str, c[0]))}-s{c[1]}{'g' if c[2] else ''}{'-misaligned' if c[3] else ''}"
                              for c in KERNEL_CASES])
def test_kernels_vs_fp64(ops, shape, scale, gray, offset):
    g = torch.Generator().manual_seed(scale + 100 * gray)
    D = 0.3 + 0.5 * torch.randn(shape, generator=g)
    y = R.degrade(0.3 + 0.5 * torch.randn(shape, generator=g), scale, gray)
    n = R.block_terms(scale, gray, shape[1])
    lim = (n + 3) * U * max(D.abs().max().item(), y.abs().max().item())
    got_y = ops.degrade(_dev(D, offset), scale, gray).cpu()
    e_deg = (got_y.double() - R.degrade(D.double(), scale, gray)).abs().max().item()
    got = ops.project_denoised(_dev(D, offset), _dev(y, offset), scale, gray).cpu()
    e = (got.double() - R.project(D.double(), y.double(), scale, gray)).abs().max().item()
    print(f"degrade {shape} ({scale}, {gray}) offset {offset}: max abs {e_deg:.3e}; project {e:.3e} (limit {lim:.3e})")
    record(f"restoration/project_{'x'.join(map(str, shape))}_s{scale}{'g' if gray else ''}_o{offset}_vs_fp64", e, lim)
    assert got_y.shape == y.shape and got.shape == D.shape
    assert e_deg <= lim and e <= lim, (e_deg, e, lim)
    # guided: D = Dg + w (Dm - Dg), w from device memory
    Dg = 0.3 + 0.5 * torch.randn(shape, generator=g)
    w = torch.full((1,), 1.75, device=DEV)
    mix = Dg.double() + 1.75 * (D.double() - Dg.double())
    got = ops.project_denoised(_dev(D, offset), _dev(y, offset), scale, gray, Dg=_dev(Dg, offset), w_dev=w).cpu()
    e = (got.double() - R.project(mix, y.double(), scale, gray)).abs().max().item()
    # (the mix itself rounds twice more: a subtraction and an fma, on values up to 1.75 * 2 max + max)
    limg = (n + 3) * U * max(mix.abs().max().item(), y.abs().max().item()) + 2 * U * 4.5 * max(
        D.abs().max().item(), Dg.abs().max().item())
    print(f"guided project {shape} ({scale}, {gray}): max abs {e:.3e} (limit {limg:.3e})")
    assert e <= limg, (e, limg)


# ------------------------------------------------------------------ 2. exact identities
@pytest.mark.parametrize("shape,scale,gray", [((7, 3, 32, 32), 2, False), ((7, 3, 32, 32), 4, True),
                                              ((7, 3, 32, 32), 8, False), ((7, 3, 16, 16), 1, True),
                                              ((7, 3, 6, 10), 2, True), ((7, 4, 64, 64), 8, False)])
def test_exact_identities(ops, shape, scale, gray):
    g = torch.Generator().manual_seed(11)
    D = 0.3 + 0.5 * torch.randn(shape, generator=g)
    Dg = 0.3 + 0.5 * torch.randn(shape, generator=g)
    y = R.degrade(0.5 * torch.randn(shape, generator=g), scale, gray)
    yd = ops.degrade(_dev(D), scale, gray)
    out = ops.project_denoised(_dev(D), _dev(y), scale, gray)
    # both memory paths give the same bits (where the vector path exists: W % 4 == 0)
    assert torch.equal(ops.degrade(_dev(D, 1), scale, gray), yd)
    assert torch.equal(ops.project_denoised(_dev(D, 1), _dev(y), scale, gray), out)
    assert torch.equal(ops.project_denoised(_dev(D), _dev(y, 1), scale, gray), out)
    # a sample's result does not depend on B
    for b in (0, 3, 6):
        assert torch.equal(ops.degrade(_dev(D[b:b + 1]), scale, gray), yd[b:b + 1])
        assert torch.equal(ops.project_denoised(_dev(D[b:b + 1]), _dev(y[b:b + 1]), scale, gray), out[b:b + 1])
    # project(D, degrade(D)) == D: the correction is an exact zero
    assert torch.equal(ops.project_denoised(_dev(D), yd, scale, gray), _dev(D))
    assert torch.equal(ops.project_denoised(_dev(D, 1), yd, scale, gray), _dev(D))
    # project(0, y) == A+ y
    back = ops.project_denoised(torch.zeros(shape, device=DEV), _dev(y), scale, gray)
    assert torch.equal(back.cpu(), R.pinv(y, scale, gray, shape[1]))
    # guided with w == 0 is the unguided call fed Dg; out= is honoured
    w0 = torch.zeros(1, device=DEV)
    buf = torch.empty(shape, device=DEV)
    r = ops.project_denoised(_dev(D), _dev(y), scale, gray, Dg=_dev(Dg), w_dev=w0, out=buf)
    assert r is buf and torch.equal(buf, ops.project_denoised(_dev(Dg), _dev(y), scale, gray))
    # the result is consistent with y to the bound of the kernel test
    n = R.block_terms(scale, gray, shape[1])
    e = (R.degrade(out.cpu().double(), scale, gray) - y.double()).abs().max().item()
    assert e <= (n + 3) * U * max(out.abs().max().item(), y.abs().max().item())


def test_linear_degradation_on_the_device(ops):
    import tinyedm_amd as T
    g = torch.Generator().manual_seed(2)
    img = torch.randn(3, 3, 16, 16, generator=g, dtype=torch.float64)
    for scale, gray in R.OPERATORS:
        deg = T.LinearDegradation(scale, gray)
        y = deg.measure(img.to(DEV))
        assert y.dtype == torch.float32 and tuple(y.shape) == deg.measurement_shape(img.shape)
        assert torch.equal(y, ops.degrade(img.float().to(DEV), scale, gray))
        assert torch.equal(deg.pinv(y, 3).cpu(), R.pinv(y.cpu(), scale, gray, 3))
        n = R.block_terms(scale, gray, 3)                                   # A A+ = I up to the sum's own rounding
        assert (deg.measure(deg.pinv(y, 3)) - y).abs().max().item() <= (n + 1) * U * y.abs().max().item()


def test_nonfinite_operands_set_health(ops):
    ops.check_health(DEV, "before")
    for shape, scale, gray, idx in (((7, 3, 32, 32), 4, False, (3, 1, 5, 17)), ((5, 3, 6, 10), 2, True, (4, 2, 5, 9))):
        ys = ops.measurement_shape(shape, scale, gray)
        for which in ("Dm", "Dg", "y"):
            t = {"Dm": torch.zeros(shape, device=DEV), "Dg": torch.zeros(shape, device=DEV),
                 "y": torch.zeros(ys, device=DEV)}
            t[which][idx if which != "y" else (idx[0], 0, 0, 0)] = float("nan") if which != "Dg" else float("inf")
            w = torch.full((1,), 0.5, device=DEV)
            ops.project_denoised(t["Dm"], t["y"], scale, gray, Dg=t["Dg"], w_dev=w)
            with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
                ops.check_health(DEV, f"project_denoised {which}")
    ops.check_health(DEV, "after")


def test_new_ops_reject_bad_operands(ops):
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    y = torch.zeros(2, 3, 4, 4, device=DEV)
    w = torch.ones(1, device=DEV)
    bad = [
        (ValueError, lambda: ops.degrade(x, 3, False)),
        (ValueError, lambda: ops.degrade(x, 1, False)),
        (ValueError, lambda: ops.degrade(x, 16, False)),
        (ValueError, lambda: ops.degrade(torch.zeros(2, 3, 6, 8, device=DEV), 4, False)),
        (ValueError, lambda: ops.degrade(torch.zeros(2, 9, 8, 8, device=DEV), 2, True)),
        (ValueError, lambda: ops.degrade(torch.zeros(2, 192, device=DEV), 2, False)),
        (ValueError, lambda: ops.degrade(x.transpose(2, 3), 2, False)),
        (TypeError, lambda: ops.degrade(x.double(), 2, False)),
        (RuntimeError, lambda: ops.degrade(x.cpu(), 2, False)),
        (ValueError, lambda: ops.project_denoised(x, y, 4, False)),
        (ValueError, lambda: ops.project_denoised(x, y, 2, True)),
        (ValueError, lambda: ops.project_denoised(x, y[:1], 2, False)),
        (TypeError, lambda: ops.project_denoised(x, y.double(), 2, False)),
        (TypeError, lambda: ops.project_denoised(x.half(), y, 2, False)),
        (RuntimeError, lambda: ops.project_denoised(x, y.cpu(), 2, False)),
        (RuntimeError, lambda: ops.project_denoised(x.cpu(), y, 2, False)),
        (ValueError, lambda: ops.project_denoised(x, y, 2, False, Dg=x.clone())),
        (ValueError, lambda: ops.project_denoised(x, y, 2, False, w_dev=w)),
        (ValueError, lambda: ops.project_denoised(x, y, 2, False, Dg=x[:1], w_dev=w)),
        (ValueError, lambda: ops.project_denoised(x, y, 2, False, Dg=x.clone(), w_dev=torch.ones(2, device=DEV))),
        (ValueError, lambda: ops.project_denoised(x, y, 2, False, out=x)),
        (ValueError, lambda: ops.project_denoised(x, y, 2, False, out=torch.zeros(2, 3, 8, 4, device=DEV))),
    ]
    from tinyedm_amd import _lib
    calls = _lib.N_CALLS
    for exc, fn in bad:
        with pytest.raises(exc):
            fn()
    assert _lib.N_CALLS == calls                    # nothing was launched


# ------------------------------------------------------------------ 3. trajectories vs the CPU composition
def _edm(P, ecfg, dcfg, dtype):
    """an eval-mode EDM on the GPU with the oracle's parameters (the set-up of tests/test_image_conditioned_gpu.py)"""
    import tinyedm_amd as T
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), dcfg.dropout_rate,
                     dcfg.sigma_data, dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    emb.load_state_dict({k[len("embedding."):]: v for k, v in P.items() if k.startswith("embedding.")}, strict=True)
    den.load_state_dict({k[len("denoiser."):]: v for k, v in P.items() if k.startswith("denoiser.")}, strict=True)
    den.set_eval_dtype(dtype)
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                  steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01)
    return model.to(DEV).eval()


def _oracle_D(Pm, em, dm, bf16, labels, guide=None):
    def D(x, s):
        sig = s.reshape(-1).expand(x.shape[0])
        Dm = O.edm_forward(Pm, em, dm, x, sig, labels, bf16=bf16).float()
        if guide is None:
            return Dm
        Pg, eg, dg, w, (lo, hi) = guide
        if not lo < float(s) <= hi:
            return Dm
        gl = labels if eg.num_classes is not None else None
        Dg = O.edm_forward(Pg, eg, dg, x, sig, gl, bf16=bf16).float()
        return Dg + w * (Dm - Dg)
    return D


SCHED = dict(num_steps=8, sigma_min=0.01, sigma_max=20.0, rho=5.0)
CASES = ["heun_bf16", "heun_f32", "stochastic_bf16", "multistep2_bf16", "multistep3_f32"]


def _case_solver(case, **kw):
    import tinyedm_amd as T
    if case.startswith("stochastic"):
        return T.StochasticSolver(**SCHED, S_churn=30.0, S_min=0.3, S_max=8.0, seed=1234, **kw)
    if case.startswith("multistep"):
        return T.MultistepSolver(**SCHED, order=int(case[9]), seed=1234, **kw)
    return T.DeterministicSolver(**SCHED, seed=1234, **kw)


def _inputs():
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 3, 8, 8, generator=g)
    labels = torch.randint(0, 10, (2,), generator=g)
    image = 0.5 * torch.randn(2, 3, 8, 8, generator=g)
    return x0, labels, image


def _reference_solve(ops, sol, D, x0, proj, start, image, solve_index):
    """the solver's composition on the CPU in fp32, with the churn noise the GPU kernel draws"""
    import tinyedm_amd as T
    t = sol.t_steps
    if isinstance(sol, T.MultistepSolver):
        return R.solve_multistep(D, t, sol.multistep_coefficients(start_step=start).tolist(), x0, proj, start, image)
    lift = None
    if isinstance(sol, T.StochasticSolver):
        s = sol.churn_schedule()
        rec = ops.churn_record(sol.seed, solve_index, DEV)

        def lift(x, i):
            if not s.gamma[i] > 0:
                return x, t[i]
            return x + s.c[i] * ops.heun_churn(torch.zeros(x0.shape, device=DEV), 1.0, rec, i).cpu(), s.t_hat[i]
    return R.solve_heun(D, t, x0, proj, start, image, lift)


def _consistency(x_out, y, scale, gray):
    """max |A x - y| with A in fp64 on the fp32 result, and the bound (n + 8) 2^-24 max(|x|, |y|): the projection's
    n + 3 roundings and the last Euler step's subtraction, division, multiplication and addition on top"""
    n = R.block_terms(scale, gray, x_out.shape[1])
    e = (R.degrade(x_out.double().cpu(), scale, gray) - y.double().cpu()).abs().max().item()
    return e, (n + 8) * U * max(x_out.abs().max().item(), y.abs().max().item())


@pytest.mark.parametrize("scale,gray", [(2, False), (4, True)], ids=["s2", "s4gray"])
@pytest.mark.parametrize("case,start", [(c, 0) for c in CASES] + [("heun_bf16", 5)])
def test_restored_trajectory_vs_reference(ops, case, start, scale, gray):
    import tinyedm_amd as T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    em, dm = tiny_cfgs(10)
    Pm = O.init_params(em, dm, torch.Generator().manual_seed(7))
    bf16 = case.endswith("bf16")
    main = _edm(Pm, em, dm, "bf16" if bf16 else "f32")
    sol = _case_solver(case)
    x0, labels, image = _inputs()
    deg = T.LinearDegradation(scale, gray)
    y = R.degrade(image, scale, gray)
    back = R.pinv(y, scale, gray, 3)                    # a partial solve is entered from A+ y, never from the image
    sol.solve_index = 5
    x_hip = sol.solve(main, x0.to(DEV), labels.to(DEV), start_step=start, image=back.to(DEV) if start else None,
                      degradation=deg, measurement=y.to(DEV)).cpu()
    assert sol.solve_index == 5 + case.startswith("stochastic")
    with torch.no_grad():
        x_ref = _reference_solve(ops, sol, _oracle_D(Pm, em, dm, bf16, labels), x0, R.projector(y, scale, gray), start,
                                 back if start else None, 5)
    e = R.rel(x_hip, x_ref)
    lim = 1e-2 if bf16 else 2e-4
    print(f"{case} ({scale}, {gray}) start {start}: rel {e:.3e} (limit {lim:.0e})")
    record(f"restoration/{case}_s{scale}{'g' if gray else ''}_start{start}_vs_{'bf16' if bf16 else 'fp32'}_oracle", e, lim)
    assert e <= lim, e
    c, clim = _consistency(x_hip, y, scale, gray)
    print(f"  consistency max |A x - y| {c:.3e} (limit {clim:.3e})")
    assert c <= clim, (c, clim)
    plain = _case_solver(case)
    plain.solve_index = 5
    kw = dict(start_step=start, image=back.to(DEV)) if start else {}
    x_plain = plain.solve(main, x0.to(DEV), labels.to(DEV), **kw).cpu()
    assert R.rel(x_plain, x_ref) > 5 * e                # the measurement mattered


def test_guided_restoration_vs_reference(ops):
    import tinyedm_amd as T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    em, dm = tiny_cfgs(10)
    eg, dg = tiny_cfgs(None)
    Pm = O.init_params(em, dm, torch.Generator().manual_seed(7))
    Pg = O.init_params(eg, dg, torch.Generator().manual_seed(11))
    interval = (0.2, 7.0)
    x0, labels, image = _inputs()
    main = _edm(Pm, em, dm, "bf16")
    guide = _edm(Pg, eg, dg, "bf16")
    for case, (scale, gray) in (("heun_bf16", (2, False)), ("multistep2_bf16", (4, True))):
        sol = _case_solver(case, guide=guide, guidance=2.0, guidance_interval=interval)
        flags = sol.guided_evaluations()
        assert any(flags) and not all(flags)            # the interval guides only part of the evaluations
        y = R.degrade(image, scale, gray)
        x_hip = sol.solve(main, x0.to(DEV), labels.to(DEV), degradation=T.LinearDegradation(scale, gray),
                          measurement=y.to(DEV)).cpu()
        with torch.no_grad():
            D = _oracle_D(Pm, em, dm, True, labels, (Pg, eg, dg, 2.0, interval))
            x_ref = _reference_solve(ops, sol, D, x0, R.projector(y, scale, gray), 0, None, 0)
            x_unguided = _reference_solve(ops, sol, _oracle_D(Pm, em, dm, True, labels), x0,
                                          R.projector(y, scale, gray), 0, None, 0)
        e = R.rel(x_hip, x_ref)
        print(f"guided {case} ({scale}, {gray}): rel {e:.3e} (limit 3e-2)")
        record(f"restoration/cfg_{case}_s{scale}{'g' if gray else ''}_vs_bf16_oracle", e, 3e-2)
        assert e <= 3e-2, e
        assert R.rel(x_unguided, x_ref) > 5 * e         # the guidance mattered too
        c, clim = _consistency(x_hip, y, scale, gray)
        assert c <= clim, (c, clim)


# ------------------------------------------------------------------ 4. + 5. the analytic Gaussian denoiser
def _gaussian(x, s, labels=None):
    s = s.double()
    return (R.MU + R.SD ** 2 / (R.SD ** 2 + s * s) * (x.double() - R.MU)).float()


@pytest.mark.parametrize("order", [None, 1, 2, 3], ids=["heun", "multistep1", "multistep2", "multistep3"])
@pytest.mark.parametrize("scale,gray", R.OPERATORS)
def test_gaussian_denoiser_decouples(ops, scale, gray, order):
    """restore(x0, y) = A+ y + (I - A+ A) plain(x0): every evaluation projected, none twice, the right y"""
    import tinyedm_amd as T
    sol = T.DeterministicSolver(num_steps=18) if order is None else T.MultistepSolver(num_steps=18, order=order)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(16, 3, 16, 16, generator=g)
    y = R.degrade(R.MU + R.SD * torch.randn(16, 3, 16, 16, generator=g), scale, gray)
    t32, t64 = sol.t_steps, sol.t_steps.double()
    D32 = lambda x, s: _gaussian(x, s)
    if order is None:
        ref = R.solve_heun(R.gaussian, t64, x0.double(), R.projector(y.double(), scale, gray))
        cpu32 = R.solve_heun(D32, t32, x0, R.projector(y, scale, gray))
        plain64 = R.solve_heun(R.gaussian, t64, x0.double())
    else:
        co = sol.multistep_coefficients()
        ref = R.solve_multistep(R.gaussian, t64, co.double().tolist(), x0.double(), R.projector(y.double(), scale, gray))
        cpu32 = R.solve_multistep(D32, t32, co.tolist(), x0, R.projector(y, scale, gray))
        plain64 = R.solve_multistep(R.gaussian, t64, co.double().tolist(), x0.double())
    assert cpu32.dtype == torch.float32
    # the reference satisfies the identity (tests/test_restoration_cpu.py asserts it to 1e-13)
    ident = R.pinv(y.double(), scale, gray, 3) + plain64 - R.pinv(R.degrade(plain64, scale, gray), scale, gray, 3)
    assert R.rel(ref, ident) <= 1e-13
    e32 = R.rel(cpu32, ref)
    lim = max(4.0 * e32, 1e-6)          # 4x: the kernels' other summation order and their fma contraction
    deg = T.LinearDegradation(scale, gray)
    x_hip = sol.solve(_gaussian, x0.to(DEV), degradation=deg, measurement=y.to(DEV)).cpu()
    e = R.rel(x_hip, ref)
    name = "heun" if order is None else f"multistep{order}"
    print(f"gaussian {name} ({scale}, {gray}): rel {e:.3e} (CPU fp32 composition {e32:.3e}, limit {lim:.3e})")
    record(f"restoration/gaussian_{name}_s{scale}{'g' if gray else ''}_vs_fp64", e, lim)
    assert e <= lim, (e, lim)
    x_plain = sol.solve(_gaussian, x0.to(DEV)).cpu()
    moved = R.rel(x_hip, x_plain)
    print(f"  distance to the plain solve {moved:.3f}")
    assert moved >= 0.05, moved
    c, clim = _consistency(x_hip, y, scale, gray)
    print(f"  consistency max |A x - y| {c:.3e} (limit {clim:.3e})")
    record(f"restoration/consistency_{name}_s{scale}{'g' if gray else ''}", c, clim)
    assert c <= clim, (c, clim)


# ------------------------------------------------------------------ 6. eager and hipGraph
@pytest.fixture(scope="module")
def pair(ops):
    em, dm = tiny_cfgs(10)
    main = _edm(O.init_params(em, dm, torch.Generator().manual_seed(7)), em, dm, "bf16")
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(3, 3, 8, 8, generator=g).to(DEV)
    labels = torch.randint(0, 10, (3,), generator=g).to(DEV)
    img = [(0.5 * torch.randn(3, 3, 8, 8, generator=g)).to(DEV) for _ in range(2)]
    return main, x0, labels, img


@pytest.mark.parametrize("case", ["heun_bf16", "stochastic_bf16", "multistep3_bf16"])
def test_hipgraph_replay_and_cache_key(pair, case):
    import tinyedm_amd as T
    main, x0, labels, img = pair
    sol = _case_solver(case)
    d2, d4g = T.LinearDegradation(2), T.LinearDegradation(4, True)

    def both(**kw):
        i = sol.solve_index
        e = sol.solve(main, x0, labels, **kw)
        sol.solve_index = i
        r = sol.solve(main, x0, labels, graph=True, **kw)
        assert torch.equal(r, e)
        return r
    n = lambda: len(sol._graphs[main])
    a = both(degradation=d2, measurement=d2.measure(img[0]))            # capture
    assert n() == 1
    b = both(degradation=d2, measurement=d2.measure(img[1]))            # a new y replays the same entry
    assert n() == 1 and not torch.equal(a, b)
    both(degradation=d4g, measurement=d4g.measure(img[0]))              # another operator: a new entry
    assert n() == 2
    both(degradation=d2, measurement=d2.measure(img[0]), start_step=3, image=d2.pinv(d2.measure(img[0]), 3))
    assert n() == 3
    both(degradation=T.LinearDegradation(2, False), measurement=d2.measure(img[0]).double())    # equal operator, fp64 y
    assert n() == 3
    # degradation=None afterwards is the solve of a solver that never saw a measurement, eager and captured
    fresh = _case_solver(case)
    fresh.solve_index = sol.solve_index
    for graph in (False, True):
        i = sol.solve_index
        assert torch.equal(sol.solve(main, x0, labels, graph), fresh.solve(main, x0, labels, graph))
        sol.solve_index = fresh.solve_index = i
    assert n() == 4 == sol.MAX_GRAPHS
    both(degradation=T.LinearDegradation(8), measurement=T.LinearDegradation(8).measure(img[0]))    # the oldest goes
    assert n() == 4


def test_zero_churn_restoration_is_deterministic_restoration(pair):
    import tinyedm_amd as T
    main, x0, labels, img = pair
    deg = T.LinearDegradation(4)
    y = deg.measure(img[0])
    det = T.DeterministicSolver(**SCHED)
    sto = T.StochasticSolver(**SCHED, S_churn=0.0)
    for graph in (False, True):
        assert torch.equal(sto.solve(main, x0, labels, graph, degradation=deg, measurement=y),
                           det.solve(main, x0, labels, graph, degradation=deg, measurement=y))


def test_captured_restoration_reports_corruption(ops, pair):
    import tinyedm_amd as T
    main, x0, labels, img = pair
    deg = T.LinearDegradation(2)
    sol = T.DeterministicSolver(**SCHED)
    y = deg.measure(img[0])
    sol.solve(main, x0, labels, graph=True, degradation=deg, measurement=y)
    bad = y.clone()
    bad[1, 2, 3, 0] = float("nan")
    with pytest.raises(ops.GraphCorruptionError):
        sol.solve(main, x0, labels, graph=True, degradation=deg, measurement=bad)
    assert torch.isfinite(sol.solve(main, x0, labels, graph=True, degradation=deg, measurement=y)).all()


# ------------------------------------------------------------------ 6b. a replay refreshes every per-call input
REPLAY_SCHED = dict(num_steps=5, sigma_min=0.01, sigma_max=20.0, rho=5.0)
REPLAY_MODES = ["heun", "guided", "churned", "multistep3", "inpaint", "sdedit", "restore", "invert", "likelihood"]


@pytest.fixture(scope="module")
def f32x3_model(ops):
    em, dm = tiny_cfgs(10)
    return _edm(O.init_params(em, dm, torch.Generator().manual_seed(7)), em, dm, "f32x3")     # (the likelihood needs fp32)


def _replay_inputs(ops, call):
    """everything a call can pass, different for call 0 and call 1 (same shapes: the second call must replay)"""
    import tinyedm_amd as T
    g = torch.Generator().manual_seed(50 + call)
    x0 = torch.randn(2, 3, 8, 8, generator=g).to(DEV)
    labels = torch.randint(0, 10, (2,), generator=g).to(DEV)
    image = (0.5 * torch.randn(2, 3, 8, 8, generator=g)).to(DEV)
    mask = torch.zeros(1, 1, 8, 8, device=DEV)      # broadcast over the batch; both values present, another half per call
    mask[..., :, :4] = 1.0
    if call:
        mask = 1.0 - mask.transpose(2, 3)
    y = T.LinearDegradation(2).measure((0.5 * torch.randn(2, 3, 8, 8, generator=g)).to(DEV))
    assert tuple(y.shape) == (2, 3, 4, 4)
    return dict(x0=x0, labels=labels, image=image, mask=mask, y=y, guidance=(2.0, 3.5)[call], solve_index=(0, 7)[call])


def _replay_solver(mode):
    import tinyedm_amd as T
    if mode == "guided":
        return T.DeterministicSolver(**REPLAY_SCHED, seed=11, guide="unconditional", guidance=2.0)
    if mode == "churned":
        return T.StochasticSolver(**REPLAY_SCHED, seed=11, S_churn=30.0, S_min=0.3, S_max=8.0)
    if mode == "multistep3":
        return T.MultistepSolver(**REPLAY_SCHED, seed=11, order=3)
    return T.DeterministicSolver(**REPLAY_SCHED, seed=11)


def _replay_call(mode, sol, model, inp, graph):
    import tinyedm_amd as T
    x0, labels, image = inp["x0"], inp["labels"], inp["image"]
    sol.solve_index = inp["solve_index"]
    if mode == "guided":
        sol.guidance = inp["guidance"]
    if mode == "inpaint":
        return sol.solve(model, x0, labels, graph, image=image, mask=inp["mask"])
    if mode == "sdedit":
        return sol.solve(model, x0, labels, graph, start_step=2, image=image)
    if mode == "restore":
        return sol.solve(model, x0, labels, graph, degradation=T.LinearDegradation(2), measurement=inp["y"])
    if mode == "invert":
        return sol.invert(model, image, labels, graph, end_step=1)
    if mode == "likelihood":
        return torch.cat([t.double().flatten() for t in sol.log_likelihood(
            model, image, labels, graph, end_step=1, num_probes=2, return_latent=True)])
    return sol.solve(model, x0, labels, graph)


@pytest.mark.parametrize("mode", REPLAY_MODES)
def test_replay_refreshes_every_per_call_input(ops, f32x3_model, mode):
    """Capture each mode once, then call it again with EVERY per-call input changed (x0, labels, image, mask values,
    measurement, guidance weight, solve_index): the replay must equal, bit for bit, a fresh eager solver given the same
    inputs, and the cache must still hold the one entry.  A static tensor that a replay forgets to refresh keeps the
    first call's value and fails here."""
    sol = _replay_solver(mode)
    results = []
    for call in (0, 1):
        inp = _replay_inputs(ops, call)
        got = _replay_call(mode, sol, f32x3_model, inp, True)
        want = _replay_call(mode, _replay_solver(mode), f32x3_model, inp, False)
        assert torch.equal(got, want), (mode, call)
        assert len(sol._graphs[f32x3_model]) == 1
        results.append(got)
    assert not torch.equal(results[0], results[1])
    if mode == "churned":
        assert any(s[0] for s in sol._churn_steps())        # (the schedule does churn on this table)


# ------------------------------------------------------------------ 7. generate CLI
CLI = ["--config_name", "cifar10_cond", "--num_samples", "4", "--batch_size", "4", "--num_steps", "4", "--num_classes",
       "10", "--image_size", "32", "--num_workers", "0"]


def _generate(out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "generate.py"), "--output_dir", str(out), *CLI, *extra]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def _load(d):
    from PIL import Image
    return np.stack([np.asarray(Image.open(os.path.join(d, f"{i}.png"))).astype(np.int64) for i in range(4)])


def test_generate_cli_restoration(ops, tmp_path):
    _generate(tmp_path / "plain")
    plain = _load(tmp_path / "plain")
    assert plain.shape == (4, 32, 32, 3)
    args = ("--init_dir", str(tmp_path / "plain"), "--restore_scale", "4", "--restore_report", str(tmp_path / "r.json"),
            "--save_degraded", str(tmp_path / "d"))
    _generate(tmp_path / "sr", *args)
    sr, low = _load(tmp_path / "sr"), _load(tmp_path / "d")
    rep = json.load(open(tmp_path / "r.json"))
    print(f"4x super-resolution report: {rep}")
    # the bound of the consistency tests with n = 16, at the magnitude the run reports (fp32, before the uint8 conversion)
    assert 0.0 <= rep["consistency"] <= (16 + 8) * U * rep["max_abs"], rep
    assert rep["psnr_restored"] > 0 and rep["psnr_degraded"] > 0 and rep["num_images"] == 4
    assert all((sr[i] != plain[i]).any() and (sr[i] != low[i]).any() for i in range(4))
    blocks = low.reshape(4, 8, 4, 8, 4, 3)
    assert (blocks == blocks[:, :, :1, :, :1]).all()                    # A+ y is constant on 4x4 blocks
    assert (low != low[:, :1, :1]).any()
    _generate(tmp_path / "sr2", *args[:3], "4")
    assert np.array_equal(_load(tmp_path / "sr2"), sr)                  # a repeated run is byte-identical
    # one mean / std for all channels: equal normalised channels are then equal grey levels
    _generate(tmp_path / "gray", "--init_dir", str(tmp_path / "plain"), "--restore_gray", "--save_degraded",
              str(tmp_path / "dg"), "--start_step", "1", "--solver", "dpmpp", "--mean", "0.5", "0.5", "0.5", "--std",
              "0.25", "0.25", "0.25")
    dg = _load(tmp_path / "dg")
    assert (dg[..., 0] == dg[..., 1]).all() and (dg[..., 1] == dg[..., 2]).all() and (dg != dg[:, :1, :1]).any()
    assert all((_load(tmp_path / "gray")[i] != plain[i]).any() for i in range(4))
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "generate.py"), "--output_dir", str(tmp_path / "x"), *CLI,
           "--restore_scale", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--init_dir" in r.stderr
