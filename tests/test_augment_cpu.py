"""Non-leaking augmentation (Karras et al. 2022, EDM, App. F.2; exact subset), host side: the composed inverse index map the
gather kernel evaluates against the forward numpy composition (tests/augment_ref.py), the word -> draw mapping, the label
table, and the plumbing that must refuse to augment behind the network's back."""
import itertools
import math

import numpy as np
import pytest
import torch

import augment_ref as R

SIZES = [(4, 4), (5, 5), (8, 8), (28, 28), (32, 32)]


def _draw_cases(H, W, square):
    """every combination of the four ops being applied or not, with every k and the extreme / zero / mixed shifts"""
    Mh, Mw = H // 8, W // 8
    shifts = sorted({(0, 0), (Mw, Mh), (-Mw, -Mh), (Mw, -Mh), (-Mw, 0), (0, Mh), (min(1, Mw), -min(1, Mh))})
    for xf, yf, tr, rot in itertools.product((0, 1), repeat=4):
        if rot and not square:
            continue
        for sx, sy in (shifts if tr else [(0, 0)]):
            for k in ((0, 1, 2, 3) if rot else (0,)):
                yield dict(xflip=xf, yflip=yf, sx=sx, sy=sy, k=k)


@pytest.mark.parametrize("H,W", SIZES + [(8, 12)])
def test_inverse_index_composition_equals_the_forward_numpy_ops(H, W):
    rng = np.random.default_rng(H * 100 + W)
    img = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    n = 0
    for d in _draw_cases(H, W, H == W):
        for flip in (0, 1):
            want = R.forward_image(img, d, flip)
            i, j = R.inverse_index(H, W, d, flip)
            assert i.min() >= 0 and i.max() < H and j.min() >= 0 and j.max() < W, (d, flip)
            assert np.array_equal(img[:, i, j], want), (d, flip)
            n += 1
    assert n >= (16 if H == W else 8)


def test_translate_is_a_shift_with_a_reflected_border():
    img = np.arange(64, dtype=np.uint8).reshape(1, 8, 8)
    out = R.forward_image(img, dict(xflip=0, yflip=0, sx=1, sy=0, k=0))
    assert np.array_equal(out[0, :, 1:], img[0, :, :-1])           # content moves right by one pixel
    assert np.array_equal(out[0, :, 0], img[0, :, 1])              # the vacated column mirrors WITHOUT repeating the edge
    out = R.forward_image(img, dict(xflip=0, yflip=0, sx=0, sy=-1, k=0))
    assert np.array_equal(out[0, :-1], img[0, 1:]) and np.array_equal(out[0, -1], img[0, -2])


def test_label_table_and_columns():
    for k in range(4):
        c, s = R.ROT_LABELS[k]
        assert c == round(math.cos(k * math.pi / 2)) - 1 and s == round(math.sin(k * math.pi / 2))
    lab = R.labels(dict(xflip=1, yflip=0, sx=-3, sy=2, k=3), 28, 32)
    assert lab.dtype == np.float32 and lab.shape == (6,)
    assert lab.tolist() == [1.0, 0.0, float(np.float32(-3) / np.float32(32)), float(np.float32(2) / np.float32(28)), -1.0, -1.0]
    assert not R.labels(dict(xflip=0, yflip=0, sx=0, sy=0, k=0), 5, 5).any()     # untouched image: the all-zero label


def test_word_mapping_is_unbiased_and_thresholds_are_exact():
    # rejection: words at or above (2^32 // n) * n are skipped, so every residue has the same number of accepted words
    n = 9
    lim = (1 << 32) // n * n
    assert (1 << 32) - lim == (1 << 32) % n and lim % n == 0
    assert R.unbiased([lim - 1], n) == (lim - 1) % n
    assert R.unbiased([lim, (1 << 32) - 1, 5], n) == 5
    assert R.unbiased([lim] * R.TRIES, n) == lim % n                # the documented cap: the last word as it is
    assert R.unbiased([12345], 1) == 0                              # M = 0 (sizes below 8): the only shift is zero
    assert R.threshold(0) == 0 and R.threshold(1) == 1 << 32 and R.threshold(0.5) == 1 << 31
    # p = 0 never, p = 1 always, for every sample
    for b in range(40):
        assert R.draws(b, 32, 32, 0.0, 15, seed=3, epoch=1)["enabled"] == (False,) * 4
        assert R.draws(b, 32, 32, 1.0, 15, seed=3, epoch=1)["enabled"] == (True,) * 4
        assert R.draws(b, 32, 32, 1.0, 0b0101, seed=3, epoch=1)["enabled"] == (True, False, True, False)
    # a masked-off op never moves another op's parameters
    a, c = R.draws(7, 32, 32, 1.0, 15, seed=3, epoch=1), R.draws(7, 32, 32, 1.0, 0b1100, seed=3, epoch=1)
    assert (a["sx"], a["sy"], a["k"]) == (c["sx"], c["sy"], c["k"]) and c["xflip"] == c["yflip"] == 0
    # the draws cover their ranges: shifts in [-4, 4], all k, both flip bits
    ds = [R.draws(b, 32, 32, 1.0, 15, seed=11, epoch=0) for b in range(400)]
    assert {d["sx"] for d in ds} == set(range(-4, 5)) == {d["sy"] for d in ds}
    assert {d["k"] for d in ds} == {0, 1, 2, 3} and {d["xflip"] for d in ds} == {0, 1} == {d["yflip"] for d in ds}
    assert all(d["sx"] == d["sy"] == 0 for d in (R.draws(b, 4, 4, 1.0, 15, seed=11, epoch=0) for b in range(50)))


def test_ops_mask_and_constants_agree_with_the_reference():
    from tinyedm_amd import ops
    assert ops.AUGMENT_OPS == R.OPS and ops.AUGMENT_DIM == 6
    assert ops.augment_op_mask(("xflip", "rot90")) == 0b1001 == R.mask_of(("xflip", "rot90"))
    assert ops.augment_op_mask(ops.AUGMENT_OPS) == 15
    with pytest.raises(ValueError, match="unknown augmentation op"):
        ops.augment_op_mask(("scale",))
    for p in (0.0, 0.12, 0.5, 1.0):
        assert ops.label_drop_threshold(p) == R.threshold(p)


def _tiny_edm(augment_dim, num_classes=None):
    import tinyedm_amd as T
    emb = T.Embedding(32, 64, num_classes, augment_dim=augment_dim) if augment_dim is not None else T.Embedding(32, 64, num_classes)
    den = T.Denoiser(3, 3, ("Enc",), ("Dec", "Dec"), (64,), (64, 64), (True, True), embedding_dim=64, num_heads=1)
    return T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                 steady_steps=1, rampup_steps=1, scheduler_interval="step")


def test_edm_batch_arity_errors_raise_before_any_gpu_call():
    model = _tiny_edm(None)
    x, y, aug = torch.zeros(2, 3, 8, 8), torch.zeros(2, dtype=torch.long), torch.zeros(2, 6)
    with pytest.raises(ValueError, match="augment_dim is 0"):
        model.training_step((x, y, aug), 0)
    with pytest.raises(ValueError, match="augment_dim is 0"):
        model.validation_step((x, y, aug), 0)
    with pytest.raises(ValueError, match="4 elements"):
        model.training_step((x, y, aug, aug), 0)
    with pytest.raises(ValueError, match="augment_dim is 0"):
        model.embedding(torch.ones(2), None, aug)
    # with augment_dim > 0 a 3-element batch passes the check (and then meets the missing GPU, like any CPU call)
    model6 = _tiny_edm(6)
    with pytest.raises(RuntimeError, match="no CPU path|GPU tensor"):
        model6.training_step((x, y, aug), 0)


def test_embedding_owns_an_aug_linear_only_when_asked():
    import tinyedm_amd as T
    from tinyedm_amd.networks import Linear
    e0, e6 = T.Embedding(32, 64, 10), T.Embedding(32, 64, 10, augment_dim=6)
    assert e0.augment_dim == 0 and e0.aug_embed is None and "aug_embed.weight" not in e0.state_dict()
    assert isinstance(e6.aug_embed, Linear) and tuple(e6.aug_embed.weight.shape) == (64, 6)
    assert e6.aug_embed.weight._edm_late and e6.sigma_embed.weight._edm_late
    with pytest.raises(ValueError, match="augment_dim"):
        T.Embedding(32, 64, 10, augment_dim=-1)


def test_deinstantiate_omits_augment_dim_at_default_and_keeps_it_at_6():
    import tinyedm
    from tinyedm.config import instantiate
    d0 = tinyedm.utils.deinstantiate(_tiny_edm(None))
    assert "augment_dim" not in d0["embedding"] and "label_dropout" not in d0["embedding"]
    assert "augment_dim" not in tinyedm.utils.deinstantiate(_tiny_edm(0))["embedding"]
    m6 = _tiny_edm(6)
    d6 = tinyedm.utils.deinstantiate(m6)
    assert d6["embedding"]["augment_dim"] == 6 and m6.hparams["embedding"]["augment_dim"] == 6
    again = instantiate(d6)
    assert again.embedding.augment_dim == 6
    again.load_state_dict(m6.state_dict(), strict=True)


def test_datamodule_arguments_and_config():
    import os
    from tinyedm.config import compose, instantiate
    from tinyedm_amd import datamodules as DM
    dm = DM.CIFAR10DataModule("nowhere", 32, batch_size=4, device="cpu")
    assert dm.augment_prob == 0.0 and dm.augment_ops == ("xflip", "yflip", "translate", "rot90")
    dm = DM.MNISTDataModule(4, augment_prob=0.25, augment_ops=["xflip", "translate"], device="cpu")
    assert dm.augment_prob == 0.25 and dm.augment_ops == ("xflip", "translate")
    with pytest.raises(ValueError, match="augment_prob"):
        DM.CIFAR10DataModule("nowhere", augment_prob=1.5)
    with pytest.raises(ValueError, match="unknown augment_ops"):
        DM.MNISTDataModule(4, augment_ops=("scale",))
    # rot90 on a non-square set is refused when the set is made resident (before anything is copied to a device)
    dm = DM.MNISTDataModule(4, augment_prob=0.5, device="cpu")
    with pytest.raises(ValueError, match="rot90 needs square images"):
        dm._resident(np.zeros((2, 1, 8, 12), np.uint8), np.zeros(2, np.int64))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = compose("cifar10_augment", os.path.join(root, "experiments", "conf"), [])
    assert cfg.datamodule.augment_prob == 0.12 and cfg.model.embedding.augment_dim == 6
    assert cfg.datamodule._target_ == "tinyedm.datamodules.CIFAR10DataModule"
    base = compose("cifar10", os.path.join(root, "experiments", "conf"), [])
    model = instantiate(cfg.model)
    assert model.embedding.augment_dim == 6 and tuple(model.embedding.aug_embed.weight.shape) == (256, 6)
    for key in ("lr", "steady_steps", "rampup_steps", "use_ema", "ema_length"):
        assert cfg.model[key] == base.model[key]
    assert cfg.model.denoiser == base.model.denoiser
    dm = instantiate(cfg.datamodule)
    assert isinstance(dm, DM.CIFAR10DataModule) and dm.augment_prob == 0.12 and dm.flip
