"""Continuous non-leaking augmentation (zoom, rotate, stretch, shift; DESIGN.md, "Continuous augmentation") on the GPU: the
resampling gather kernel against the fp64 numpy definition (tests/augment_warp_ref.py) under bounds from the fp32 format,
its exact path bit for bit against the exact-ops kernel, refusals, the resident loaders, and a whole optimisation step --
eager and as a replayed hipGraph -- fed (x, y, 13 augment labels) batches."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_ref as R
import augment_warp_ref as WR
from oracle import data_oracle as DO

DEV = "cuda"
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------ the gather kernel
N_IMAGES = 23
SHAPES = [(1, 5, 5), (3, 8, 12), (1, 28, 28), (3, 32, 32), (1, 64, 64)]
SEED, EPOCH = 2, 3 * 65536 + 7  # a seed whose p = 0.5, B = 65 reference batches cover the cases (_covers): a condition on the inputs
_data_cache = {}


def _dataset(shape):
    """(uint8 numpy (N, C, H, W), the same on the device, index numpy (65,) with repeats): made once per shape"""
    if shape not in _data_cache:
        rng = np.random.default_rng(shape[0] * 1000 + shape[1] * 10 + shape[2])
        data = rng.integers(0, 256, (N_IMAGES,) + shape, dtype=np.uint8)
        index = rng.integers(0, N_IMAGES, 65)
        _data_cache[shape] = (data, torch.from_numpy(data).to(DEV), index)
    return _data_cache[shape]


def _ops_for(shape):
    return R.OPS if shape[1] == shape[2] else R.OPS[:3]


def _covers(ds, wds):
    """every exact and every continuous op both applied and not, samples with no continuous op at all (the exact path) next
    to warped ones, rotations of both signs and zooms on both sides of 1"""
    ok = all({d["enabled"][i] for d in ds} == {True, False} for i in range(3))
    ok = ok and all({d["enabled"][i] for d in wds} == {True, False} for i in range(4))
    ok = ok and {any(d["enabled"]) for d in wds} == {True, False}
    ok = ok and {d["theta"] > 0 for d in wds if d["enabled"][1]} == {True, False}
    return ok and {d["s"] > 1 for d in wds if d["enabled"][0]} == {True, False}


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("shape", SHAPES)
def test_warping_gather_against_the_fp64_definition(ops, shape, B, p, flip):
    """Labels 0-5: the exact ops' table, bit for bit.  Labels 6-12 against fp64 within 64 u max(1, r), u = 2^-24,
    r = sqrt(-2 ln uni) of the column's Box-Muller pair: ROCm's device logf, sqrtf, cosf and sinf are documented at <= 2 ulp
    each (sqrtf <= 1), and the fp32 angle 2 pi uni carries <= 7.5e-7 absolute (the rounded constant and one product, at most
    2 pi each half an ulp of 2 pi ~ 4.8e-7, rounded up), which moves r cos / r sin by <= 7.5e-7 r ~ 12.6 u r; the radius adds
    (2 + 1) u r through logf (halved by the root) and sqrtf, the final product u r: <= about 16 u r, and the bound allows x4.
    The products with cos(phi) / sin(phi) of the stretch columns add 3 u r more, inside the same x4.

    Theta against the fp64 draws is a gross-error check (1e-4 relative for the linear part, 1e-4 (H + W) for the offsets:
    rounding is ~1e-6, a wrong sign, order or centre moves it by >= 1e-2).  The image is then compared with the fp64
    definition evaluated with the matrix the kernel reported, per element, within WR.batch's bound: 2 L delta for the
    fp32 coordinate (L the largest neighbour difference of U, delta = 8 u max |q|), gamma(256) sum |weights * values| for the
    three filter stages, 3 u |result| for the final divide, subtract, divide."""
    data, data_dev, index = _dataset(shape)
    C, H, W = shape
    idx = index[:B]
    ops_ = _ops_for(shape)
    idx_dev = torch.from_numpy(idx).to(DEV)
    x, a, th = ops.u8_gather_augment_warp_normalize(data_dev, idx_dev, flip=flip, seed=SEED, epoch=EPOCH, p=p, ops=ops_,
                                                    warp_ops=WR.WARP_OPS, return_theta=True)
    assert x.dtype == torch.float32 and tuple(x.shape) == (B,) + shape and tuple(a.shape) == (B, 13) and tuple(th.shape) == (B, 6)
    again = ops.u8_gather_augment_warp_normalize(data_dev, idx_dev, flip=flip, seed=SEED, epoch=EPOCH, p=p, ops=ops_,
                                                 warp_ops=WR.WARP_OPS, return_theta=True)
    assert all(torch.equal(u, v) for u, v in zip((x, a, th), again))              # no atomics: the same bits
    x_exact, a_exact = ops.u8_gather_augment_normalize(data_dev, idx_dev, flip=flip, seed=SEED, epoch=EPOCH, p=p, ops=ops_)
    th_np = th.cpu().numpy().astype(np.float64)
    want_x, bound, want_a, tol, want_th, ds, wds = WR.batch(data, idx, p, ops_, WR.WARP_OPS, flip, SEED, EPOCH, thetas=th_np)
    if p == 0.5 and B == 65:
        assert _covers(ds, wds), "pick another seed: the reference batch does not cover the cases"
    # labels
    assert torch.equal(a[:, :6], a_exact) and torch.equal(a[:, :6].cpu(), torch.from_numpy(want_a[:, :6].astype(np.float32)))
    a_np = a.cpu().numpy().astype(np.float64)
    lab_err = np.abs(a_np[:, 6:] - want_a[:, 6:])
    assert bool((lab_err <= tol[:, 6:]).all()), f"labels: worst error / bound {(lab_err / tol[:, 6:]).max():.3g}"
    for b, wd in enumerate(wds):
        for i, cols in enumerate(((6,), (7, 8), (9, 10), (11, 12))):
            if not wd["enabled"][i]:
                assert not a_np[b, list(cols)].any()
    # Theta
    th_np = th_np.reshape(B, 2, 3)
    lin_tol = 1e-4 * np.abs(want_th[:, :, :2]).max(axis=2, keepdims=True)
    assert bool((np.abs(th_np[:, :, :2] - want_th[:, :, :2]) <= lin_tol).all())
    assert bool((np.abs(th_np[:, :, 2] - want_th[:, :, 2]) <= 1e-4 * (H + W)).all())
    # image
    warped = np.array([any(wd["enabled"]) for wd in wds])
    x_np = x.cpu().numpy().astype(np.float64)
    if (~warped).any():
        rows = torch.from_numpy(np.nonzero(~warped)[0]).to(DEV)
        assert torch.equal(x[rows], x_exact[rows])                                          # the exact path: bit for bit
        assert np.array_equal(x_np[~warped], want_x[~warped])
        assert np.array_equal(th_np[~warped], np.broadcast_to(WR.IDENTITY, (int((~warped).sum()), 2, 3)))
    if p == 0.0:
        assert not warped.any() and torch.equal(x, x_exact) and not a[:, 6:].any()
    if warped.any():
        err = np.abs(x_np - want_x)[warped]
        ratio = (err / bound[warped]).max()
        print(f"warp {shape} B={B} p={p} flip={flip}: {int(warped.sum())} warped, worst error / bound = {ratio:.3g}, "
              f"worst error {err.max():.3g}")
        assert ratio <= 1.0
        assert float(np.abs(x_np[warped] - x_exact.cpu().numpy()[warped]).max()) > 1e-3        # and something was warped


@pytest.mark.parametrize("shape", [(3, 32, 32), (3, 8, 12)])
def test_no_continuous_op_is_the_exact_gather(ops, shape):
    _, data_dev, index = _dataset(shape)
    idx = torch.from_numpy(index).to(DEV)
    ops_ = _ops_for(shape)
    for flip in (False, True):
        want_x, want_a = ops.u8_gather_augment_normalize(data_dev, idx, 0.4, 0.3, flip=flip, seed=9, epoch=2, p=0.5, ops=ops_)
        x, a = ops.u8_gather_augment_warp_normalize(data_dev, idx, 0.4, 0.3, flip=flip, seed=9, epoch=2, p=0.5, ops=ops_,
                                                    warp_ops=())
        assert torch.equal(x, want_x) and torch.equal(a[:, :6], want_a) and not a[:, 6:].any() and tuple(a.shape) == (65, 13)
        x, a = ops.u8_gather_augment_warp_normalize(data_dev, idx, 0.4, 0.3, flip=flip, seed=9, epoch=2, p=0.0, ops=ops_)
        assert torch.equal(x, ops.u8_gather_normalize(data_dev, idx, 0.4, 0.3, flip=flip, seed=9, epoch=2)) and not a.any()
    # the exact ops' decisions do not move when the continuous ops join them
    want_x, want_a = ops.u8_gather_augment_normalize(data_dev, idx, flip=True, seed=9, epoch=2, p=0.5, ops=ops_)
    x, a = ops.u8_gather_augment_warp_normalize(data_dev, idx, flip=True, seed=9, epoch=2, p=0.5, ops=ops_, warp_ops=("shift",))
    assert torch.equal(a[:, :6], want_a) and not a[:, 6:11].any() and a[:, 11:].any()
    same = ~a[:, 11:].any(dim=1)
    assert 0 < int(same.sum()) < 65 and torch.equal(x[same], want_x[same]) and not torch.equal(x, want_x)


def test_unsupported_sizes_and_bad_indices_write_nothing(ops):
    from tinyedm_amd import _lib

    def call(data, idx, out, aug, theta, B, C, H, W, n, aug_ops=7):
        _lib.call("edm_u8_gather_augment_warp_normalize", ops._p(data), ops._p(idx), ops._p(out), B, C, H, W, n, 0.5, 0.5, 0,
                  1, 0, 1 << 32, aug_ops, 15, ops._p(aug), ops._p(theta), ops._stream())

    idx = torch.tensor([0, 1, 1, 0], device=DEV)
    for H, W in ((65, 65), (1, 8), (8, 1), (64, 65)):
        data = torch.zeros(2, 1, H, W, dtype=torch.uint8, device=DEV)
        out, aug, theta = (torch.full(s, 7.0, device=DEV) for s in ((4, 1, H, W), (4, 13), (4, 6)))
        with pytest.raises(_lib.HipKernelError, match=r"status -3.*2 \.\. 64"):
            call(data, idx, out, aug, theta, 4, 1, H, W, 2)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((aug == 7.0).all()) and bool((theta == 7.0).all())
    with pytest.raises(_lib.HipKernelError, match=r"2 \.\. 64"):
        ops.u8_gather_augment_warp_normalize(torch.zeros(2, 1, 65, 65, dtype=torch.uint8, device=DEV), idx, p=0.5, ops=())
    _, data_dev, _ = _dataset((3, 8, 12))
    out, aug, theta = (torch.full(s, 7.0, device=DEV) for s in ((4, 3, 8, 12), (4, 13), (4, 6)))
    with pytest.raises(_lib.HipKernelError, match=r"status -3.*rot90 needs square"):         # rot90 with H != W: as today
        call(data_dev, idx, out, aug, theta, 4, 3, 8, 12, N_IMAGES, aug_ops=15)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((aug == 7.0).all()) and bool((theta == 7.0).all())
    # out-of-range index entries are never read: their rows (image, labels, matrix) are left as they were
    bad = torch.tensor([0, N_IMAGES, -1, 3], device=DEV)
    call(data_dev, bad, out, aug, theta, 4, 3, 8, 12, N_IMAGES)
    assert bool((out[1:3] == 7.0).all()) and bool((aug[1:3] == 7.0).all()) and bool((theta[1:3] == 7.0).all())
    for b in (0, 3):
        assert not bool((out[b] == 7.0).any()) and not bool((aug[b] == 7.0).any()) and not bool((theta[b] == 7.0).any())
    # theta may be null
    out2, aug2 = torch.full((4, 3, 8, 12), 7.0, device=DEV), torch.full((4, 13), 7.0, device=DEV)
    call(data_dev, bad, out2, aug2, None, 4, 3, 8, 12, N_IMAGES)
    assert torch.equal(out2, out) and torch.equal(aug2, aug)


def test_loaders_yield_thirteen_labels_only_when_asked(ops, tmp_path):
    from tinyedm_amd import datamodules as DM
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (48, 3, 32, 32), dtype=np.uint8)
    lab = rng.integers(0, 10, 48)
    DO.write_cifar10_batches(str(tmp_path), img, lab, n_train=40)
    dm = DM.CIFAR10DataModule(str(tmp_path), 32, batch_size=16, device=DEV, augment_prob=0.5, augment_warp_ops=WR.WARP_OPS)
    dm.setup("fit")
    data = dm.train_dataset[0]
    loader = dm.train_dataloader()
    seen_warp = False
    for epoch in range(2):
        order = DM.epoch_order(40, True, dm.seed, epoch, loader.rank, loader.world, data.device)
        for bi, batch in enumerate(loader):
            assert len(batch) == 3 and tuple(batch[2].shape)[1] == 13
            idx = order[bi * 16:(bi + 1) * 16].contiguous()
            seed, ep = dm.seed + 7919 * loader.rank, epoch * 65536 + bi
            x, a, th = ops.u8_gather_augment_warp_normalize(data, idx, 0.5, 0.5, flip=True, seed=seed, epoch=ep, p=0.5,
                                                            warp_ops=WR.WARP_OPS, return_theta=True)
            assert torch.equal(batch[0], x) and torch.equal(batch[2], a) and torch.equal(batch[1], dm.train_dataset[1][idx])
            want_x, bound, want_a, tol, _, _, wds = WR.batch(img[:40], idx.cpu().numpy(), 0.5, R.OPS, WR.WARP_OPS, True, seed, ep,
                                                             thetas=th.cpu().numpy())
            assert bool((np.abs(batch[2].cpu().numpy() - want_a) <= tol).all())
            assert bool((np.abs(batch[0].cpu().numpy() - want_x) <= bound).all())
            seen_warp = seen_warp or any(any(wd["enabled"]) for wd in wds)
    assert seen_warp
    for batch in dm.val_dataloader():
        assert len(batch) == 2 and batch[0].shape[1:] == (3, 32, 32)
    # not given: today's tuples from today's op
    dm = DM.CIFAR10DataModule(str(tmp_path), 32, batch_size=16, device=DEV, augment_prob=0.5)
    dm.setup("fit")
    loader = dm.train_dataloader()
    order = DM.epoch_order(40, True, dm.seed, 0, loader.rank, loader.world, data.device)
    for bi, batch in enumerate(loader):
        idx = order[bi * 16:(bi + 1) * 16].contiguous()
        x, a = ops.u8_gather_augment_normalize(dm.train_dataset[0], idx, 0.5, 0.5, flip=True, seed=dm.seed + 7919 * loader.rank,
                                               epoch=bi, p=0.5)
        assert len(batch) == 3 and torch.equal(batch[0], x) and torch.equal(batch[2], a) and tuple(a.shape) == (len(idx), 6)
    dm.setup("test")
    for batch in dm.test_dataloader():
        assert len(batch) == 2
    # a subset of the continuous ops; augment_prob = 0 keeps the pairs
    two = DM.CIFAR10DataModule(str(tmp_path), 32, batch_size=16, device=DEV, augment_prob=1.0, augment_ops=(),
                               augment_warp_ops=("rotate",))
    two.setup("fit")
    x, y, a = next(iter(two.train_dataloader()))
    assert not a[:, :7].any() and not a[:, 9:].any() and bool(a[:, 7:9].any(dim=1).all())
    off = DM.CIFAR10DataModule(str(tmp_path), 32, batch_size=16, device=DEV, augment_warp_ops=WR.WARP_OPS)
    off.setup("fit")
    assert len(next(iter(off.train_dataloader()))) == 2


# ------------------------------------------------------------------------------------------------ the whole step
def _labels13(B, seed):
    """labels of the kind the loader makes: the six exact ones of test_augment_gpu._inputs, then seven continuous ones"""
    from test_augment_gpu import _inputs
    _, _, aug6 = _inputs(B, None, seed)
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(B, 4, generator=g)
    th, ph = (torch.rand(B, generator=g) * 2 - 1) * math.pi, (torch.rand(B, generator=g) * 2 - 1) * math.pi
    on = (torch.rand(B, 4, generator=g) < 0.5).float()
    cont = torch.stack([n[:, 0] * on[:, 0], (th.cos() - 1) * on[:, 1], th.sin() * on[:, 1], n[:, 1] * ph.cos() * on[:, 2],
                        n[:, 1] * ph.sin() * on[:, 2], n[:, 2] * on[:, 3], n[:, 3] * on[:, 3]], dim=1)
    return torch.cat([aug6.cpu(), cont], dim=1).to(DEV)


def test_step_with_thirteen_labels_eager_and_captured_checkpoint_and_sampling(ops, tmp_path):
    """(x, y, aug13) batches through the eager step and through CapturedTrainStep from the same state, under the limits of
    tests/test_augment_gpu.py's six-label test; then the checkpoint round trip and sampling without labels."""
    import tinyedm_amd as T
    from test_augment_gpu import _build, _opt, rel
    from tinyedm_amd import networks as N
    from tinyedm_amd.graph import CapturedTrainStep
    g = torch.Generator().manual_seed(5)
    batches = [((0.5 * torch.randn(8, 3, 16, 16, generator=g)).to(DEV), torch.randint(0, 10, (8,), generator=g).to(DEV),
                _labels13(8, 70 + i)) for i in range(5)]
    model_e = _build(13)
    w0 = model_e.embedding.aug_embed.weight.detach().clone()
    assert tuple(w0.shape)[1] == 13
    opt_e, base_e, sched_e = _opt(model_e)
    opt_e.zero_grad()
    losses_e = []
    for b in batches:
        loss = model_e.training_step(b, 0)
        loss.backward()
        opt_e.step()
        opt_e.zero_grad()
        sched_e.step()
        losses_e.append(float(loss))
    counters_e = (base_e.step_count, opt_e.current_step, N.rng.step)
    model_g = _build(13)
    assert torch.equal(model_g.embedding.aug_embed.weight, w0)
    opt_g, base_g, sched_g = _opt(model_g)
    opt_g.zero_grad()
    step = CapturedTrainStep(model_g, opt_g)
    losses_g = []
    for b in batches:
        loss = step(b)
        sched_g.step()
        losses_g.append(float(loss))
    assert len(step._graphs) == 1
    assert (base_g.step_count, opt_g.current_step, N.rng.step) == counters_e
    assert all(math.isfinite(l) for l in losses_e + losses_g)
    worst = max(abs(a - b) / abs(b) for a, b in zip(losses_g, losses_e))
    assert worst <= 2e-3, (losses_g, losses_e)
    for name, a, b, lim in (("theta", base_g.arena.theta, base_e.arena.theta, 2e-3), ("adam_m", base_g.m, base_e.m, 2e-2),
                            ("adam_v", base_g.v, base_e.v, 2e-2), ("ema", opt_g.ema_arena, opt_e.ema_arena, 2e-3)):
        e = rel(a, b)
        assert e <= lim, f"{name}: rel {e:.3e}"
    for m in (model_e, model_g):
        w = m.embedding.aug_embed.weight.detach()
        assert torch.isfinite(w).all() and not torch.equal(w, w0)
    assert rel(model_g.embedding.aug_embed.weight, model_e.embedding.aug_embed.weight) <= 2e-3
    step.release()
    path = str(tmp_path / "aug13.ckpt")
    torch.save({"hyper_parameters": dict(model_g.hparams), "state_dict": model_g.state_dict()}, path)
    loaded = T.EDM.load_from_checkpoint(path).to(DEV).eval()
    assert loaded.embedding.augment_dim == 13
    assert torch.equal(loaded.embedding.aug_embed.weight, model_g.embedding.aug_embed.weight)
    x0 = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
    lab = torch.arange(4, device=DEV)
    with torch.no_grad():
        sig = torch.full((4,), 1.5, device=DEV)
        assert torch.equal(loaded(x0, sig, lab), loaded(x0, sig, lab, torch.zeros(4, 13, device=DEV)))
    with pytest.raises(ValueError, match=r"shape \(B, 13\)"):
        model_g.training_step((batches[0][0], batches[0][1], torch.zeros(8, 6, device=DEV)), 0)
