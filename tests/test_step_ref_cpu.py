"""Checks of the training-step restatements themselves (tests/step_ref.py; no GPU): the two Diffuser streams never share
a counter, the dropout threshold and keep rate, the fp64 Adam + EMA against the oracle, and the error bounds that
tests/test_step_exact_gpu.py holds the kernels to against a numpy float32 evaluation of the same expressions.
(The Philox known-answer vectors are in tests/test_evaluate_cpu.py.)"""
import math

import numpy as np
import pytest
import torch

import elementwise_ref
import step_ref as S
from oracle import edm_oracle as O

SEED = 0x0BADC0FFEE123457


def test_diffuser_streams_share_no_counter():
    """B < 2^16 samples and B * CHW / 4 < 2^16 quads: no counter tuple of the noise stream is one of the sigma stream"""
    for step in (0, 3, 2 ** 32 - 1, S.NOISE_TAG, S.SIGMA_TAG):
        noise = set(zip(*(c.tolist() for c in S.noise_counters(np.arange(0, 4 << 16, 4), step))))
        sigma = set(zip(*(c.tolist() for c in S.sigma_counters(1 << 16, step))))
        assert len(noise) == len(sigma) == 1 << 16
        assert not noise & sigma
    # every element of a quad shares its counter and takes another normal of it
    c = S.noise_counters(np.arange(8), 5)
    assert c[0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and set(c[2].tolist()) == {0xD1FF} and set(c[3].tolist()) == {5}
    n = S.diffuse_unit_noise(np.arange(8), SEED, 5)
    assert len(set(n.tolist())) == 8
    # and the streams are different numbers, not only different counters
    s, n0 = S.diffuse_sigma(8, -1.2, 1.2, SEED, 5)
    assert not set(n0.tolist()) & set(n.tolist())
    assert np.array_equal(s, np.exp(S.f32(-1.2) + S.f32(1.2) * n0))


def test_diffuse_ref_composes_its_parts():
    clean = np.random.default_rng(0).standard_normal((3, 5))
    noisy, sigma, unit = S.diffuse_ref(clean, -1.2, 1.2, 1, 3)
    assert noisy.shape == unit.shape == (3, 5) and sigma.shape == (3,)
    assert np.array_equal(unit.ravel(), S.diffuse_unit_noise(np.arange(15), 1, 3))
    assert np.array_equal(noisy, clean + sigma[:, None] * unit)
    # a sample's sigma depends on nothing but (b, seed, step); the noise on nothing but the flat index
    assert np.array_equal(S.diffuse_sigma(1, -1.2, 1.2, 1, 3)[0], sigma[:1])
    assert np.array_equal(S.diffuse_unit_noise([14, 3], 1, 3), unit.ravel()[[14, 3]])


@pytest.mark.parametrize("p,thr", [(0.1, 6554), (0.13, 8520), (0.25, 16384), (0.5, 32768), (0.999, 65470), (5e-6, 0)])
def test_dropout_threshold_by_hand(p, thr):
    assert S.dropout_threshold(p) == thr
    keep, scale = S.dropout_keep_ref(64, p, SEED, 5, 6)
    assert keep.dtype == np.uint8 and keep.shape == (64,)
    assert scale == 65536.0 / (65536 - thr) == elementwise_ref.dropout_scale(p)
    if thr == 0:
        assert keep.all() and scale == 1.0


def test_dropout_p0_keeps_everything():
    keep, scale = S.dropout_keep_ref(24, 0.0, SEED, 0, 0)
    assert keep.all() and scale == 1.0 == elementwise_ref.dropout_scale(0.0)


@pytest.mark.parametrize("p", [0.1, 0.13, 0.5])
def test_dropout_keep_rate(p):
    n = 1 << 20
    keep, _ = S.dropout_keep_ref(n, p, SEED, 5, 6)
    q = 1.0 - S.dropout_threshold(p) / 65536.0
    dev = abs(keep.mean() - q) / math.sqrt(q * (1 - q) / n)
    assert dev <= 5.0, f"p = {p}: keep rate {keep.mean():.6f} vs {q:.6f}, {dev:.2f} standard deviations"
    # a subset of the elements is the same subset of the mask
    idx = np.array([0, 7, 8, 9, n - 1])
    assert np.array_equal(S.dropout_keep_ref(n, p, SEED, 5, 6, elems=idx)[0], keep[idx])


def test_dropout_lane_order_by_hand():
    """element j of a chunk: bits 16 (j & 1) .. of word j >> 1, kept iff >= thr"""
    r = [int(w) for w in S.philox4x32_10(3, 0, 5, 6, SEED & S.U32, SEED >> 32)]
    lanes = [r[0] & 0xFFFF, r[0] >> 16, r[1] & 0xFFFF, r[1] >> 16, r[2] & 0xFFFF, r[2] >> 16, r[3] & 0xFFFF, r[3] >> 16]
    keep, _ = S.dropout_keep_ref(32, 0.5, SEED, 5, 6)
    assert keep[24:32].tolist() == [int(x >= 32768) for x in lanes]


@pytest.mark.parametrize("step", [1, 7, 100000])
def test_adam_ema_ref_is_the_oracle_at_fp64(step):
    g = torch.Generator().manual_seed(step)
    n = 257
    th, gr, m = (torch.randn(n, generator=g, dtype=torch.float64) for _ in range(3))
    v, ema = torch.rand(n, generator=g, dtype=torch.float64) * 0.01, torch.randn(n, generator=g, dtype=torch.float64)
    lr, b1, b2, eps, beta = (S.f32(x) for x in (0.02, 0.9, 0.999, 1e-8, 0.37))
    ref = S.adam_ema_ref(th.numpy(), gr.numpy(), m.numpy(), v.numpy(), ema.numpy(), [ema.numpy()], [beta], lr=lr, b1=b1,
                         b2=b2, eps=eps, bc1=1 - b1 ** step, bc2sqrt=math.sqrt(1 - b2 ** step), ema_beta=beta, grad_scale=1.0)
    O.adam_step(th, gr, m, v, step, lr, b1, b2, eps)
    O.ema_step(ema, th, beta)
    for key, t in (("theta", th), ("m", m), ("v", v), ("ema", ema)):
        err = np.abs(ref[key] - t.numpy()).max() / np.abs(t.numpy()).max()
        assert err <= 1e-12, (key, err)
    assert np.array_equal(ref["profiles"][0], ref["ema"]) and np.array_equal(ref["mag_profiles"][0], ref["mag_ema"])


def test_bias_corrections_are_the_kernels():
    assert S.bias_corrections(0.9, 0.999, 1) == (S.f32(1.0 - S.f32(0.9)), S.f32(math.sqrt(1.0 - S.f32(0.999))))
    bc1, bc2s = S.bias_corrections(0.9, 0.999, 1)
    assert abs(bc1 - 0.1) < 1e-7 and bc1 != 0.1            # float32(0.9) is not 0.9
    assert S.bias_corrections(0.9, 0.999, 100000)[0] == 1.0
    for s in (7, 100000):
        bc1, bc2s = S.bias_corrections(0.9, 0.999, s)
        assert bc1 == S.f32(bc1) and bc2s == S.f32(bc2s)
        assert abs(bc2s - math.sqrt(1 - S.f32(0.999) ** s)) <= 2.0 ** -24         # one rounding of a number <= 1


@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("step", [1, 7, 100000])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_adam_bounds_hold_for_the_fp32_restatement(step, grad_scale, fma):
    """the bounds the kernels are held to, against the same expressions in numpy float32 with and without fused
    multiply-adds: a bound this evaluation broke would be the bound's fault, not a kernel's"""
    n = 65540
    st = S.adam_state(n, 11 + step)
    bc1, bc2s = S.bias_corrections(0.9, 0.999, step)
    hp = dict(lr=S.f32(2e-3), b1=S.f32(0.9), b2=S.f32(0.999), eps=S.f32(1e-8), bc1=bc1, bc2sqrt=bc2s, ema_beta=S.f32(0.9),
              grad_scale=grad_scale)
    ref = S.adam_ema_ref(st["theta"], st["grad"], st["m"], st["v"], st["ema"], [], [], **hp)
    bound = S.adam_ema_bounds(ref, st["theta"], hp["ema_beta"])
    got = S.adam_ema_f32(st["theta"], st["grad"], st["m"], st["v"], st["ema"], fma=fma, **hp)
    for key in ("m", "v", "theta", "ema"):
        err = np.abs(got[key].astype(np.float64) - ref[key])
        ratio = np.where(err == 0, 0.0, err / np.maximum(bound[key], 1e-300)).max()
        print(f"fp32 restatement, step {step}, grad_scale {grad_scale}, fma {fma}: {key} err / bound {ratio:.3f}")
        assert ratio <= 1.0, (key, ratio)
    z = n // 2
    assert got["theta"][z] == st["theta"][z] and ref["dtheta"][z] == 0 and got["m"][z] == 0 and got["v"][z] == 0
