"""Continuous non-leaking augmentation (zoom, rotate, stretch, shift; DESIGN.md, "Continuous augmentation"), host side: the
invariants of the numpy definition (tests/augment_warp_ref.py) in fp64, its geometry against an analytic image, its fp32
evaluation against the a-priori bound the GPU test uses, the word -> draw mapping, and the host plumbing."""
import math
import os

import numpy as np
import pytest

import augment_ref as R
import augment_warp_ref as WR

SIZES = [(5, 5), (8, 12), (32, 32)]
EXACT = 1e-8        # byte units: 20x the 4.4e-10 measured on the fp64 prototype, three orders under fp32 resolution (255 * 2^-24)
MIXED = dict(s=1.1, theta=-0.4, a=1.15, phi=0.7, ty=1.3, tx=-0.8)


def _plane(H, W):
    return np.random.default_rng(H * 100 + W).integers(0, 256, (H, W)).astype(np.float64)


def test_taps_are_orthonormal_and_the_centroid_is_the_documented_one():
    h = WR.TAPS
    assert abs(h.sum() - math.sqrt(2)) < 1e-12
    for k in range(6):
        assert abs((h[:12 - 2 * k] * h[2 * k:]).sum() - (1.0 if k == 0 else 0.0)) < 1e-12, k
    assert abs(WR.CENTROID - 0.09826089954573) < 1e-13
    assert np.array_equal(WR.reflect(np.arange(-5, 10), 4), [1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3])


@pytest.mark.parametrize("H,W", SIZES)
def test_identity_and_constant_planes_are_reproduced(H, W):
    S = _plane(H, W)
    assert np.allclose(WR.theta_matrix(H, W), WR.IDENTITY, atol=1e-13, rtol=0)
    err = np.abs(WR.warp_plane(S, WR.IDENTITY) - S).max()
    print(f"identity {H}x{W}: {err:.3g} byte units")
    assert err <= EXACT
    for kw in (dict(), MIXED, dict(theta=2.5, s=0.5, ty=0.7 * H, tx=-0.6 * W)):
        err = np.abs(WR.warp_plane(np.full((H, W), 200.0), WR.theta_matrix(H, W, **kw)) - 200.0).max()
        assert err <= EXACT, (kw, err)


@pytest.mark.parametrize("H,W", SIZES)
def test_a_whole_pixel_shift_is_the_reflected_translate_of_the_exact_ops(H, W):
    S = _plane(H, W)
    n = 0
    for sy in range(-(H // 8), H // 8 + 1):
        for sx in range(-(W // 8), W // 8 + 1):
            want = R.forward_image(S[None], dict(xflip=0, yflip=0, sx=sx, sy=sy, k=0))[0]
            err = np.abs(WR.warp_plane(S, WR.theta_matrix(H, W, ty=sy, tx=sx)) - want).max()
            assert err <= EXACT, (sy, sx, err)
            n += 1
    assert n == (2 * (H // 8) + 1) * (2 * (W // 8) + 1)


def _smooth(y, x):
    """two sinusoids, both under 0.08 cycles per pixel: (0.07, 0.03) -> 0.076, (0.02, -0.06) -> 0.063"""
    return 128 + 60 * np.sin(2 * np.pi * (0.07 * y + 0.03 * x)) + 50 * np.cos(2 * np.pi * (0.02 * y - 0.06 * x) + 1)


@pytest.mark.parametrize("name,kw", [("rot90", dict(theta=math.pi / 2)), ("rot0.6", dict(theta=0.6)), ("zoom1.25", dict(s=1.25)),
                                     ("mixed", MIXED)])
def test_geometry_against_an_analytic_image(name, kw):
    """the output at p_out is the image at p_src = ctr + F^-1 (p_out - ctr - t), where the source lies >= 4 pixels inside:
    <= 1.5 byte units (0.77 measured on the prototype, which a wrong half-pixel convention multiplies)"""
    worst, seen = 0.0, 0
    for H, W in SIZES:
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        D = WR.warp_plane(_smooth(yy, xx), WR.theta_matrix(H, W, **kw))
        sy, sx = WR.p_src(H, W, yy, xx, **kw)
        inside = (sy >= 4) & (sy <= H - 5) & (sx >= 4) & (sx <= W - 5)
        if inside.any():
            worst = max(worst, np.abs(D - _smooth(sy, sx))[inside].max())
            seen += int(inside.sum())
    print(f"geometry {name}: worst {worst:.3g} byte units over {seen} pixels")
    assert seen >= 500 and worst <= 1.5


@pytest.mark.parametrize("H,W", SIZES)
def test_fp32_evaluation_stays_inside_the_a_priori_bound(H, W):
    """numpy fp32 against fp64 with the same fp32 matrix, inside plane_bound (what the GPU test allows the kernel)"""
    S = _plane(H, W)
    worst = 0.0
    for kw in (dict(), dict(theta=math.pi / 2), MIXED, dict(theta=2.5, s=0.5, ty=0.7 * H, tx=-0.6 * W), dict(s=2.2, a=2.2, phi=1.0)):
        th = WR.theta_matrix(H, W, **kw).astype(np.float32)
        D64, bound = WR.plane_bound(S, th)
        err = np.abs(WR.warp_plane(S, th, np.float32).astype(np.float64) - D64)
        worst = max(worst, (err / bound).max())
        assert bool((err <= bound).all()), (kw, (err / bound).max())
    print(f"fp32 vs fp64 {H}x{W}: worst error / bound = {worst:.3g}")


def test_draws_words_and_ranges():
    seed, epoch, thr = 11, 5, R.threshold(0.5)
    for b in range(40):
        en = R._words(b, 32, R.TAG, epoch, seed)
        d = WR.draws(b, 32, 32, 0.5, 0b1011, seed, epoch)
        assert d["enabled"] == (en[0] < thr, en[1] < thr, False, en[3] < thr)
        assert WR.draws(b, 32, 32, 0.0, 15, seed, epoch)["enabled"] == (False,) * 4
        assert WR.draws(b, 32, 32, 1.0, 15, seed, epoch)["enabled"] == (True,) * 4
        assert WR.draws(b, 32, 32, 1.0, 0, seed, epoch)["enabled"] == (False,) * 4
    # the parameters come from words 33 and 34
    w0, w1 = R._words(3, 33, R.TAG, epoch, seed), R._words(3, 34, R.TAG, epoch, seed)
    d = WR.draws(3, 28, 32, 1.0, 15, seed, epoch)
    assert d["theta"] == math.pi * (2 * WR.uni(w0[2]) - 1) and d["phi"] == math.pi * (2 * WR.uni(w1[1]) - 1)
    assert d["n_s"] == WR.bm(w0[0], w0[1])[0] and d["n_a"] == WR.bm(w0[3], w1[0])[0]
    assert (d["n_x"], d["n_y"]) == WR.bm(w1[2], w1[3])[:2]
    assert d["ty"] == 0.125 * 28 * d["n_y"] and d["tx"] == 0.125 * 32 * d["n_x"] and d["s"] == 2 ** (0.2 * d["n_s"])
    assert 0 < WR.uni(0) and WR.uni(0xFFFFFFFF) < 1 and np.float32(WR.uni(0xFFFFFFFF)) == WR.uni(0xFFFFFFFF)
    # a masked-off op never moves another's parameters
    c = WR.draws(3, 28, 32, 1.0, 0b1010, seed, epoch)
    assert (c["theta"], c["n_x"], c["n_y"]) == (d["theta"], d["n_x"], d["n_y"]) and c["n_s"] == c["n_a"] == c["phi"] == 0.0
    assert c["s"] == c["a"] == 1.0
    # the exact ops' draws do not move when the continuous ops join them (different counter words)
    data = np.random.default_rng(0).integers(0, 256, (7, 1, 8, 8), dtype=np.uint8)
    idx = np.arange(20) % 7
    _, want_a, want_d = R.batch(data, idx, 0.5, R.OPS, True, seed, epoch)
    _, _, aug, _, _, ds, _ = WR.batch(data, idx, 0.5, R.OPS, WR.WARP_OPS, True, seed, epoch)
    assert ds == want_d and np.array_equal(aug[:, :6].astype(np.float32), want_a)
    # coverage over 400 samples
    full = [WR.draws(b, 32, 32, 1.0, 15, seed, 0) for b in range(400)]
    assert {d["theta"] > 0 for d in full} == {True, False} and {d["s"] > 1 for d in full} == {True, False}
    assert {d["a"] > 1 for d in full} == {True, False} and {d["ty"] > 0 for d in full} == {True, False}
    assert all(abs(d["theta"]) < math.pi and abs(d["n_s"]) <= 5.8 and abs(d["n_x"]) <= 5.8 for d in full)
    half = [WR.draws(b, 32, 32, 0.5, 15, seed, 0) for b in range(400)]
    for i in range(4):
        assert {d["enabled"][i] for d in half} == {True, False}
    # labels: zeros for a disabled op
    lab = WR.labels(WR.draws(3, 32, 32, 1.0, 0b0010, seed, epoch))
    assert lab[0] == 0 and lab[3:].tolist() == [0.0] * 4 and lab[1] == math.cos(d["theta"]) - 1 and lab[2] == math.sin(d["theta"])
    assert not WR.labels(WR.draws(3, 32, 32, 0.0, 15, seed, epoch)).any()


def test_masks_and_constants():
    from tinyedm_amd import _lib, ops
    assert ops.AUGMENT_WARP_OPS == WR.WARP_OPS == ("zoom", "rotate", "stretch", "shift")
    assert ops.AUGMENT_DIM_WARP == WR.DIM == 13 and ops.AUGMENT_DIM == 6 and len(ops.AUGMENT_OPS) == 4
    assert ops.augment_warp_mask(()) == 0 and ops.augment_warp_mask(ops.AUGMENT_WARP_OPS) == 15
    assert ops.augment_warp_mask(("zoom", "shift")) == 0b1001 == WR.mask_of(("zoom", "shift"))
    with pytest.raises(ValueError, match="unknown continuous augmentation op"):
        ops.augment_warp_mask(("xflip",))
    with pytest.raises(ValueError, match="unknown augmentation op"):
        ops.augment_op_mask(("zoom",))
    assert len(_lib.SIGNATURES["edm_u8_gather_augment_warp_normalize"]) == len(_lib.SIGNATURES["edm_u8_gather_augment_normalize"]) + 2
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tinyedm_hip.h")).read()
    assert "int edm_u8_gather_augment_warp_normalize(" in header


def test_datamodule_arguments_and_config():
    from tinyedm.config import compose, instantiate
    from tinyedm_amd import datamodules as DM
    dm = DM.CIFAR10DataModule("nowhere", 32, batch_size=4, device="cpu")
    assert dm.augment_warp_ops == ()
    dm = DM.MNISTDataModule(4, augment_prob=0.25, augment_ops=(), augment_warp_ops=["zoom", "shift"], device="cpu")
    assert dm.augment_warp_ops == ("zoom", "shift") and dm.augment_ops == ()
    with pytest.raises(ValueError, match="unknown augment_warp_ops"):
        DM.MNISTDataModule(4, augment_warp_ops=("translate",))
    with pytest.raises(ValueError, match="unknown augment_warp_ops"):
        DM.CIFAR10DataModule("nowhere", augment_warp_ops=("scale",))
    # sizes the resampling kernel does not take are refused when the set is made resident
    for shape in ((2, 1, 65, 65), (2, 1, 1, 8), (2, 1, 8, 80)):
        with pytest.raises(ValueError, match="augment_warp_ops: images of 2 .. 64"):
            dm._resident(np.zeros(shape, np.uint8), np.zeros(2, np.int64))
    # ... and only then: without the continuous ops (or with augment_prob 0) the same set passes
    plain = DM.MNISTDataModule(4, augment_prob=0.25, augment_ops=(), device="cpu")
    off = DM.MNISTDataModule(4, augment_prob=0.0, augment_warp_ops=("zoom",), device="cpu")
    for m in (plain, off):
        x, y = m._resident(np.zeros((2, 1, 65, 65), np.uint8), np.zeros(2, np.int64))
        assert tuple(x.shape) == (2, 1, 65, 65)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    conf = os.path.join(root, "experiments", "conf")
    cfg, base = compose("cifar10_augment_warp", conf, []), compose("cifar10_augment", conf, [])
    assert list(cfg.datamodule.augment_warp_ops) == list(WR.WARP_OPS) and cfg.model.embedding.augment_dim == 13
    assert cfg.datamodule.augment_prob == base.datamodule.augment_prob and cfg.datamodule.augment_ops == base.datamodule.augment_ops
    assert cfg.model.denoiser == base.model.denoiser and cfg.trainer == base.trainer
    model = instantiate(cfg.model)
    assert model.embedding.augment_dim == 13 and tuple(model.embedding.aug_embed.weight.shape) == (256, 13)
    dm = instantiate(cfg.datamodule)
    assert isinstance(dm, DM.CIFAR10DataModule) and dm.augment_warp_ops == WR.WARP_OPS and dm.augment_prob == 0.12


def test_the_error_hint_names_the_batchs_label_width():
    import torch
    from test_augment_cpu import _tiny_edm
    model = _tiny_edm(None)
    x, y = torch.zeros(2, 3, 8, 8), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match=r"augment_dim is 0.*augment_dim=13"):
        model.training_step((x, y, torch.zeros(2, 13)), 0)
    with pytest.raises(ValueError, match=r"augment_dim is 0.*augment_dim=6"):
        model.training_step((x, y, torch.zeros(2, 6)), 0)
