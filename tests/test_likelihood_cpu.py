"""Host-side checks of the likelihood evaluation (no GPU): bits_per_dim, the validation of
DeterministicSolver.log_likelihood, the new refusals of generate's argument checks, and the restated probe stream."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import likelihood_ref as R
from parity_log import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _solvers():
    import tinyedm_amd.solvers as S
    return S


def test_bits_per_dim_by_hand():
    S = _solvers()
    # d = 12, three channels: bpd = (3000 / 12 + (log(255*0.5) + log(255*0.25) + log(255*1.0)) / 3) / ln 2
    want = (250.0 + (math.log(127.5) + math.log(63.75) + math.log(255.0)) / 3.0) / math.log(2.0)
    got = S.bits_per_dim(torch.tensor([-3000.0], dtype=torch.float64), 12, (0.5, 0.25, 1.0))
    assert got.dtype == torch.float64 and got.device.type == "cpu" and got.shape == (1,)
    err = abs(got.item() - want)
    record("likelihood/bits_per_dim_by_hand_abs", err, 1e-12)
    assert err <= 1e-12, (got.item(), want)
    # a scalar std is every channel's; fp32 logp is widened, not the other way round
    a = S.bits_per_dim(torch.tensor([-3000.0, 10.0]), 12, 0.5)
    assert a.dtype == torch.float64
    assert abs(a[0].item() - (250.0 + math.log(127.5)) / math.log(2.0)) <= 1e-12
    # the inverse relation: logp = -(bpd ln 2 - mean log((levels - 1) std)) d, and one nat per dim is 1 / ln 2 bits
    back = -(a * math.log(2.0) - math.log(127.5)) * 12
    assert torch.allclose(back, torch.tensor([-3000.0, 10.0], dtype=torch.float64), rtol=0, atol=1e-9)
    lo, hi = S.bits_per_dim(torch.tensor([-120.0, -132.0]), 12, 0.5)
    assert abs((hi - lo).item() - 1.0 / math.log(2.0)) <= 1e-12
    # levels: 16 grey levels are 4 bits fewer per dim than 256 up to the (levels - 1) convention
    assert abs((S.bits_per_dim(0.0, 1, 1.0, 16) - math.log2(15.0)).item()) <= 1e-12
    for bad in (dict(dims=0), dict(dims=1.5), dict(dims=True), dict(std=0.0), dict(std=(0.5, -1.0)), dict(levels=1)):
        kw = dict(logp=torch.zeros(1), dims=12, std=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            S.bits_per_dim(**kw)


def _refuse(fn, exc=ValueError, match=None):
    with pytest.raises(exc, match=match):
        fn()


def test_log_likelihood_validation():
    S = _solvers()
    sol = S.DeterministicSolver(num_steps=8)
    img = torch.zeros(2, 3, 8, 8)

    def D(x, s, labels=None):
        return x
    for end in (-1, 8, 1.0, True, None):
        _refuse(lambda: sol.log_likelihood(D, img, end_step=end), match="end_step")
    for k in (0, -1, 33, 1.0, True):
        _refuse(lambda: sol.log_likelihood(D, img, num_probes=k), match="num_probes")
    _refuse(lambda: sol.log_likelihood(D, img.long()), match="floating-point")
    _refuse(lambda: sol.log_likelihood(D, [[0.0]]), match="floating-point")
    _refuse(lambda: sol.log_likelihood(D, img), RuntimeError, match="GPU tensor")        # valid arguments, CPU image
    assert sol.solve_index == 0         # a refused call draws nothing
    for delta in (0.0, -1e-2, math.nan, math.inf, "x", True):
        bad = S.DeterministicSolver(num_steps=8, delta=delta)
        _refuse(lambda: bad.log_likelihood(D, img), match="delta")
        _refuse(lambda: bad.probe_widths(), match="delta")
    for seed, index in ((-1, 0), (1 << 64, 0), (0, -1), (0, 1 << 32), (0.5, 0)):
        bad = S.DeterministicSolver(num_steps=8)
        bad.seed, bad.solve_index = seed, index          # (plain attributes, read at every solve)
        _refuse(lambda: bad.log_likelihood(D, img))
    # subclasses refuse through the inversion hook
    _refuse(lambda: S.MultistepSolver(num_steps=8).log_likelihood(D, img), match="Multistep")
    _refuse(lambda: S.StochasticSolver(num_steps=8, S_churn=10.0).log_likelihood(D, img), match="churn")
    _refuse(lambda: S.StochasticSolver(num_steps=8).log_likelihood(D, img), RuntimeError, match="GPU tensor")
    # bf16 evaluation is refused before anything touches a device
    import tinyedm_amd as T
    den = T.Denoiser.__new__(T.Denoiser)
    torch.nn.Module.__init__(den)
    assert den.eval_dtype == "bf16"
    _refuse(lambda: sol.log_likelihood(den.eval(), img), match="bf16")


def test_probe_widths():
    S = _solvers()
    sol = S.DeterministicSolver(num_steps=8, delta=3e-2)
    t = sol.t_steps[:8].double()
    h = sol.probe_widths(0.5)
    assert len(h) == 8 and S.NLL_DELTA == S.DeterministicSolver().delta
    want = (3e-2 * (t * t + 0.25).sqrt()).float().tolist()
    assert h == want
    assert sol.probe_widths(0.5, 1e-3)[0] == pytest.approx(1e-3 * math.sqrt(80.0 ** 2 + 0.25), rel=1e-6)


def test_check_conditioning_refusals():
    from tinyedm_amd.generate import _check_conditioning as chk
    ok = dict(init_dir="d", start_step=0, mask_box=None, invert_to=None, solver="heun", S_churn=0.0, image_size=32)
    chk(**ok)
    chk(**ok, likelihood_to="o.json", num_probes=3, dequantize=True, network_dtype="f32")
    _refuse(lambda: chk(**dict(ok, init_dir=None), likelihood_to="o.json"), match="--init_dir")
    _refuse(lambda: chk(**dict(ok, solver="dpmpp"), likelihood_to="o.json"), match="Heun")
    _refuse(lambda: chk(**dict(ok, S_churn=5.0), likelihood_to="o.json"), match="S_churn")
    _refuse(lambda: chk(**dict(ok, mask_box=(1, 1, 5, 5)), likelihood_to="o.json"), match="--mask_box")
    _refuse(lambda: chk(**dict(ok, invert_to="l.pt"), likelihood_to="o.json"), match="--invert_to")
    _refuse(lambda: chk(**ok, likelihood_to="o.json", network_dtype="bf16"), match="bf16")
    _refuse(lambda: chk(**ok, num_probes=2), match="--num_probes needs")
    _refuse(lambda: chk(**ok, dequantize=True), match="--dequantize needs")
    for k in (0, 33, 1.5, True):
        _refuse(lambda: chk(**ok, likelihood_to="o.json", num_probes=k), match="--num_probes")


@pytest.mark.parametrize("extra,needle", [
    (["--likelihood_to", "o.json"], "--init_dir"),
    (["--init_dir", "d", "--likelihood_to", "o.json", "--network_dtype", "bf16"], "bf16"),
    (["--init_dir", "d", "--likelihood_to", "o.json", "--solver", "dpmpp"], "Heun"),
    (["--init_dir", "d", "--likelihood_to", "o.json", "--mask_box", "1", "1", "5", "5"], "--mask_box"),
    (["--init_dir", "d", "--num_probes", "2"], "--likelihood_to"),
    (["--init_dir", "d", "--dequantize"], "--likelihood_to"),
], ids=["no-init", "bf16", "dpmpp", "mask", "probes-alone", "dequantize-alone"])
def test_cli_parser_refusals(extra, needle, tmp_path):
    """an argument error leaves with status 2 before anything is loaded (no GPU, no checkpoint)"""
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "generate.py"), "--output_dir", str(tmp_path), "--config_name",
           "cifar10_cond", "--num_samples", "4", "--batch_size", "4", "--num_classes", "10", "--image_size", "32", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and needle in r.stderr, r.stderr[-1500:]


def test_ops_reject_before_launch():
    """the wrappers validate on the host: a CPU tensor never reaches the library"""
    from tinyedm_amd import ops
    x = torch.zeros(2, 3, 4, 4)
    rec = torch.zeros(4, dtype=torch.int32)
    L = torch.zeros(2, dtype=torch.float64)
    for fn in (lambda: ops.nll_probe(x, 0.1, rec, 0), lambda: ops.heun_euler_div(x, x, 1.0, 2.0, 0.1, 0.1, rec, 1, L),
               lambda: ops.heun_correct_div(x, x, x, x, 1.0, 2.0, 0.1, rec, 1, L), lambda: ops.nll_prior(x, 1.0, L)):
        _refuse(fn, RuntimeError, match="no CPU path")
    assert ops.NLL_MAX_STEPS == ops.INPAINT_MAX_STEPS == 1 << 16


def test_restated_probe_stream():
    """the restatement the GPU tests compare against: +-1, balanced, its own tags, one bit per probe"""
    shape, seed = (5, 3, 7, 9), 0x9E3779B97F4A7C15
    e = R.probe_signs(shape, seed, 3, 5, 0, 3)
    assert e.shape == (3,) + shape and set(e.unique().tolist()) == {-1.0, 1.0}
    assert abs(e.mean().item()) < 0.1
    # the evaluation index and the step move the tag; probes are different bits of the same words
    w0 = R.philox_words(shape, seed, 3, R.NLL_TAG ^ 5)
    assert np.array_equal(w0, R.philox_words(shape, seed, 3, 0x4E4C0005))
    for tag in (0x43480000 ^ 5, 0x49500000 ^ 5, (R.NLL_TAG + (1 << 16)) ^ 5, R.NLL_TAG ^ 4):
        assert (R.philox_words(shape, seed, 3, tag) != w0).mean() > 0.99
    assert not torch.equal(e[0], e[1]) and not torch.equal(e[0], R.probe_signs(shape, seed, 3, 5, 1, 1)[0])
    assert torch.equal(e[:1], R.probe_signs(shape, seed, 3, 5, 0, 1))
    # Philox4x32-10 known answer (Random123 kat_vectors: zero counter, zero key)
    kat = [int(v) for v in R.philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert kat == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_recursion_closed_form_cpu():
    """the fp64 restatement against the closed form for a diagonal Gaussian: second order at the step counts the GPU
    test uses (16 -> 32 -> 64 falls by >= 3.8x at each doubling)"""
    S = _solvers()
    g = torch.Generator().manual_seed(1)
    MU = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64).view(1, 3, 1, 1)
    SV = torch.tensor([0.25, 0.5, 1.0], dtype=torch.float64).view(1, 3, 1, 1)
    img = (MU + SV.sqrt() * torch.randn(16, 3, 8, 8, generator=g, dtype=torch.float64)).float().double()
    err = {}
    for N in (16, 32, 64):
        t = S.DeterministicSolver(num_steps=N).t_steps.double()
        lp, _ = R.nll_recursion(lambda x, i: MU + SV / (SV + t[i] ** 2) * (x - MU),
                                lambda x, i, step, ev: (SV / (SV + t[i] ** 2)).expand(x.shape).flatten(1).sum(1), img, t)
        var = (SV + t[N - 1] ** 2).expand(img.shape)
        exact = (-0.5 * torch.log(2 * math.pi * var) - (img - MU) ** 2 / (2 * var)).flatten(1).sum(1)
        err[N] = ((lp - exact).abs().max() / 192).item()
    assert err[16] / err[32] >= 3.8 and err[32] / err[64] >= 3.8, err
