"""Non-leaking augmentation (Karras et al. 2022, EDM, App. F.2; exact subset) on the GPU: the augmenting gather kernel
bit-exactly against the numpy restatement (tests/augment_ref.py), the resident loaders, the augment-label conditioning of
Embedding (forward / backward against fp64 on the same fp32 operands, bounds from the fp32 format), and a whole
optimisation step -- eager and as a replayed hipGraph -- fed (x, y, augment_labels) batches."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_ref as R
from oracle import data_oracle as DO
from oracle import edm_oracle as O

DEV = "cuda"
U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------ the gather kernel
N_IMAGES = 23
SHAPES = [(1, 5, 5), (3, 8, 12), (1, 28, 28), (3, 32, 32), (3, 4, 4)]
SEED = 5                # one for which the p = 0.5, B = 65 reference batches cover the cases (_covers): a condition on the inputs
_data_cache = {}


def _dataset(shape):
    """(uint8 numpy (N, C, H, W), the same on the device, index numpy (65,) with repeats): made once per shape"""
    if shape not in _data_cache:
        rng = np.random.default_rng(shape[0] * 1000 + shape[1] * 10 + shape[2])
        data = rng.integers(0, 256, (N_IMAGES,) + shape, dtype=np.uint8)
        index = rng.integers(0, N_IMAGES, 65)
        assert len(set(index.tolist())) < 65
        _data_cache[shape] = (data, torch.from_numpy(data).to(DEV), index)
    return _data_cache[shape]


def _ops_for(shape):
    return R.OPS if shape[1] == shape[2] else R.OPS[:3]


def _covers(ds, H, W, ops_):
    """every op of the mask both applied and not, all four k, shifts of both signs and zero (where the size allows a shift)"""
    ok = all({d["enabled"][i] for d in ds} == {True, False} for i in range(4) if R.OPS[i] in ops_)
    if "rot90" in ops_:
        ok = ok and {d["k"] for d in ds if d["enabled"][3]} == {0, 1, 2, 3}
    for key, size in (("sx", W), ("sy", H)):
        if size // 8:
            s = {int(np.sign(d[key])) for d in ds if d["enabled"][2]}
            ok = ok and s == {-1, 0, 1}
    return ok


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("shape", SHAPES)
def test_augmenting_gather_is_bit_exact(ops, shape, B, p, flip):
    data, data_dev, index = _dataset(shape)
    idx = index[:B]
    ops_ = _ops_for(shape)
    seed, epoch = SEED, 3 * 65536 + 7
    want_x, want_a, ds = R.batch(data, idx, p, ops_, flip, seed, epoch)
    if p == 0.5 and B == 65:
        assert _covers(ds, shape[1], shape[2], ops_), "pick another seed: the reference batch does not cover the cases"
    x, a = ops.u8_gather_augment_normalize(data_dev, torch.from_numpy(idx).to(DEV), flip=flip, seed=seed, epoch=epoch, p=p,
                                           ops=ops_)
    assert x.dtype == torch.float32 and tuple(x.shape) == (B,) + shape and tuple(a.shape) == (B, 6)
    assert torch.equal(a.cpu(), torch.from_numpy(want_a))
    assert torch.equal(x.cpu(), torch.from_numpy(want_x))


@pytest.mark.parametrize("shape", [(3, 32, 32), (3, 8, 12)])
def test_probability_zero_is_the_plain_gather(ops, shape):
    _, data_dev, index = _dataset(shape)
    idx = torch.from_numpy(index).to(DEV)
    for flip in (False, True):
        x, a = ops.u8_gather_augment_normalize(data_dev, idx, 0.4, 0.3, flip=flip, seed=9, epoch=2, p=0.0, ops=_ops_for(shape))
        assert torch.equal(x, ops.u8_gather_normalize(data_dev, idx, 0.4, 0.3, flip=flip, seed=9, epoch=2))
        assert not a.any()
    # the unlabelled flip does not move when the labelled ops join it: same decisions as the plain kernel's
    x, a = ops.u8_gather_augment_normalize(data_dev, idx, flip=True, seed=9, epoch=2, p=1.0, ops=())
    assert torch.equal(x, ops.u8_gather_normalize(data_dev, idx, flip=True, seed=9, epoch=2)) and not a.any()


def test_rot90_on_a_non_square_set_is_unsupported_and_writes_nothing(ops):
    from tinyedm_amd import _lib
    _, data_dev, index = _dataset((3, 8, 12))
    idx = torch.from_numpy(index[:4]).to(DEV)
    out = torch.full((4, 3, 8, 12), 7.0, device=DEV)
    aug = torch.full((4, 6), 7.0, device=DEV)
    with pytest.raises(_lib.HipKernelError, match=r"status -3.*rot90 needs square"):
        _lib.call("edm_u8_gather_augment_normalize", ops._p(data_dev), ops._p(idx), ops._p(out), 4, 3, 8, 12, N_IMAGES, 0.5,
                  0.5, 0, 1, 0, 1 << 32, 15, ops._p(aug), ops._stream())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((aug == 7.0).all())
    with pytest.raises(_lib.HipKernelError, match="rot90 needs square"):
        ops.u8_gather_augment_normalize(data_dev, idx, p=0.5)
    # out-of-range index entries are never read: their rows (image and labels) are left as they were
    bad = torch.tensor([0, N_IMAGES, -1, 3], device=DEV)
    _lib.call("edm_u8_gather_augment_normalize", ops._p(data_dev), ops._p(bad), ops._p(out), 4, 3, 8, 12, N_IMAGES, 0.5,
              0.5, 0, 1, 0, 1 << 32, 7, ops._p(aug), ops._stream())
    assert bool((out[1:3] == 7.0).all()) and bool((aug[1:3] == 7.0).all())
    assert not bool((out[0] == 7.0).any()) and not bool((out[3] == 7.0).any())


def test_loaders_yield_augment_labels_only_when_asked(ops, tmp_path):
    from tinyedm_amd import datamodules as DM
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (48, 3, 32, 32), dtype=np.uint8)
    lab = rng.integers(0, 10, 48)
    DO.write_cifar10_batches(str(tmp_path), img, lab, n_train=40)
    # augment_prob = 0: today's 2-tuples from today's kernel
    dm = DM.CIFAR10DataModule(str(tmp_path), 32, batch_size=16, device=DEV)
    dm.setup("fit")
    data = dm.train_dataset[0]
    loader = dm.train_dataloader()
    for epoch in range(2):
        order = DM.epoch_order(40, True, dm.seed, epoch, loader.rank, loader.world, data.device)
        n = 0
        for bi, batch in enumerate(loader):
            assert len(batch) == 2
            idx = order[bi * 16:(bi + 1) * 16].contiguous()
            want = ops.u8_gather_normalize(data, idx, 0.5, 0.5, flip=True, seed=dm.seed + 7919 * loader.rank,
                                           epoch=epoch * 65536 + bi)
            assert torch.equal(batch[0], want) and torch.equal(batch[1], dm.train_dataset[1][idx])
            n += 1
        assert n == 3
    # augment_prob = 0.5: the train loader alone yields 3-tuples, images and labels the reference's
    dm = DM.CIFAR10DataModule(str(tmp_path), 32, batch_size=16, device=DEV, augment_prob=0.5)
    dm.setup("fit")
    loader = dm.train_dataloader()
    seen_aug = False
    for epoch in range(2):
        order = DM.epoch_order(40, True, dm.seed, epoch, loader.rank, loader.world, data.device)
        for bi, batch in enumerate(loader):
            assert len(batch) == 3
            idx = order[bi * 16:(bi + 1) * 16]
            want_x, want_a, _ = R.batch(img[:40], idx.cpu().numpy(), 0.5, R.OPS, True, dm.seed + 7919 * loader.rank,
                                        epoch * 65536 + bi)
            assert torch.equal(batch[0].cpu(), torch.from_numpy(want_x))
            assert torch.equal(batch[2].cpu(), torch.from_numpy(want_a))
            assert torch.equal(batch[1], dm.train_dataset[1][idx])
            seen_aug = seen_aug or bool(batch[2].any())
    assert seen_aug
    for batch in dm.val_dataloader():
        assert len(batch) == 2 and batch[0].shape[1:] == (3, 32, 32)
    two = DM.CIFAR10DataModule(str(tmp_path), 32, batch_size=16, device=DEV, augment_prob=0.5, augment_ops=("xflip", "translate"))
    two.setup("fit")
    x, y, a = next(iter(two.train_dataloader()))
    assert not a[:, 1].any() and not a[:, 4:].any()


# ------------------------------------------------------------------------------------------------ conditioning
E_DIM, F_DIM, K_AUG, N_CLS = 256, 64, 6, 10


def _embedding(num_classes, label_dropout, seed):
    import tinyedm_amd as T
    torch.manual_seed(seed)
    T.manual_seed(seed)
    mod = T.Embedding(F_DIM, E_DIM, num_classes, 0.5, label_dropout=label_dropout, augment_dim=K_AUG).to(DEV).train()
    state = {k: v.detach().clone() for k, v in mod.named_parameters()}
    return mod, state


def _restore(mod, state):
    """training-mode forwards normalise the master weights in place: every call starts from the same bits"""
    with torch.no_grad():
        for k, p in mod.named_parameters():
            p.copy_(state[k])
            p.grad = None


def _inputs(B, num_classes, seed, distinct=False):
    g = torch.Generator().manual_seed(seed)
    sigma = torch.exp(1.2 * torch.randn(B, generator=g) - 1.2).to(DEV)
    labels = torch.randint(0, N_CLS, (B,), generator=g).to(DEV) if num_classes else None
    if distinct:            # no class twice in the batch (needs num_classes >= B)
        labels = torch.randperm(num_classes, generator=g)[:B].to(DEV)
    # labels of the kind the loader makes: flips in {0, 1}, shifts in [-1/8, 1/8], the rot90 table
    k = torch.randint(0, 4, (B,), generator=g)
    rot = torch.tensor(R.ROT_LABELS)[k]
    aug = torch.cat([torch.randint(0, 2, (B, 2), generator=g).float(), (torch.randint(-4, 5, (B, 2), generator=g) / 32.0),
                     rot], dim=1).to(DEV)
    return sigma, labels, aug


CONFIGS = [(B, nc, pd) for B in (1, 3, 64) for nc, pd in ((None, 0.0), (N_CLS, 0.0), (N_CLS, 0.5))]


@pytest.mark.parametrize("B,num_classes,label_dropout", CONFIGS)
def test_embedding_forward_with_augment_labels(ops, B, num_classes, label_dropout):
    """None and the all-zero label reproduce the un-augmented embedding bit for bit; random labels against fp64 on the same
    fp32 operands.  Bound on es' = es + a . w^T per element: six products and six additions in fp32 (with or without
    contraction) stay within gamma_7 * sum_k |a_k w_k| of the exact dot product's contribution, and the final addition rounds
    once more: u * |es'|.  That interval is pushed through the combine by evaluating the fp64 combine at both of its ends;
    the combine kernel's own fp32 error is the bound tests/test_fp32_sidepath_gpu.py::test_embed_combine derives for it."""
    mod, state = _embedding(num_classes, label_dropout, 3 + B)
    sigma, labels, aug = _inputs(B, num_classes, 17 + B)

    def run(a):
        _restore(mod, state)
        four, out = mod(sigma, labels, a)
        drop = mod.last_label_drop
        return four, out.detach(), None if drop is None else drop.clone()

    four0, out0, drop0 = run(None)
    fourz, outz, dropz = run(torch.zeros_like(aug))
    assert torch.equal(outz, out0) and torch.equal(fourz, four0)
    if label_dropout > 0:
        assert drop0 is not None and torch.equal(drop0, dropz)
        if B == 64:
            assert 0 < int(drop0.sum()) < B
    fourr, outr, dropr = run(aug)
    assert torch.equal(fourr, four0) and not torch.equal(outr, out0)
    # the fp32 operands, from the same kernels on the same starting weights
    _restore(mod, state)
    wsh, wah = mod.sigma_embed.packs()[2], mod.aug_embed.packs()[2]
    es = ops.linear_fwd(four0.contiguous(), wsh)
    got_es = ops.aug_embed_fwd(es.clone(), aug, wah)
    a64, w64, es64 = aug.double().cpu(), wah.double().cpu(), es.double().cpu()
    ref_es = es64 + a64 @ w64.t()
    delta = gamma(7) * (a64.abs() @ w64.abs().t()) + U * ref_es.abs()
    err = (got_es.double().cpu() - ref_es).abs()
    assert bool((err <= delta).all()), f"es': worst error / bound {(err / delta.clamp_min(1e-300)).max():.3g}"
    assert torch.equal(ops.aug_embed_fwd(es.clone(), torch.zeros_like(aug), wah), es)
    # ... through the combine
    t = mod.add_factor
    c = 1.0 / math.sqrt((1 - t) ** 2 + t ** 2)
    keep = torch.zeros(B, 1, dtype=torch.bool)
    cls = torch.zeros(B, E_DIM, dtype=torch.float64)
    if labels is not None:
        wch = mod.class_embed.linear.packs()[2].double().cpu()
        cls = wch.t()[labels.cpu()] * math.sqrt(N_CLS)
        keep = torch.ones(B, 1, dtype=torch.bool) if dropr is None else (dropr.cpu() == 0).view(B, 1)

    def combine64(e):
        pre = torch.where(keep, O.mp_add(e, cls, t), e)
        return pre, O.mp_silu(pre)

    pre_mid, out_mid = combine64(ref_es)
    spread = torch.maximum((combine64(ref_es - delta)[1] - out_mid).abs(), (combine64(ref_es + delta)[1] - out_mid).abs())
    e_pre = torch.where(keep, 6 * U * ((1 - t) * ref_es.abs() + t * cls.abs()) * c, torch.zeros_like(ref_es))
    own = 2 * (1.85 * e_pre + U * (pre_mid.abs() + 4) * (pre_mid * torch.sigmoid(pre_mid)).abs() / 0.596)
    err = (outr.double().cpu() - out_mid).abs()
    bound = spread + own
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"embedding forward B={B} classes={num_classes} dropout={label_dropout}: worst error / bound = {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("B", [1, 3, 64])
def test_aug_embed_wgrad_against_fp64(ops, B):
    """gw[e, k] = sum_b ges[b, e] a[b, k], b ascending: B products and B - 1 additions -> within gamma_B * sum_b |ges a|"""
    g = torch.Generator().manual_seed(B)
    ges = torch.randn(B, E_DIM, generator=g).to(DEV)
    _, _, aug = _inputs(B, None, 5 + B)
    gw = ops.aug_embed_wgrad(ges, aug)
    ref = ges.double().cpu().t() @ aug.double().cpu()
    bound = gamma(B) * (ges.double().cpu().abs().t() @ aug.double().cpu().abs())
    err = (gw.double().cpu() - ref).abs()
    assert tuple(gw.shape) == (E_DIM, K_AUG) and bool((err <= bound).all()), (err / bound.clamp_min(1e-300)).max()
    assert torch.equal(gw, ops.aug_embed_wgrad(ges, aug))


@pytest.mark.parametrize("B,num_classes,label_dropout", [(3, None, 0.0), (64, 64, 0.0), (64, 64, 0.5)])
def test_embedding_backward_with_augment_labels(ops, B, num_classes, label_dropout):
    """ges flows on to sigma_embed and the class weights unchanged: with the all-zero label (es' == es, so the same
    pre-activation) and the same injected gout their gradients are those of the augment_labels=None call bit for bit, and
    aug_embed's is zero; with real labels aug_embed gets a gradient, the same bits on every run.

    The class-weight gradient is bit-comparable only where the existing k_embed_combine_bwd is: it adds the samples of a class
    with float atomics, in an order that changes from launch to launch (two augment_labels=None calls with a repeated class
    differ in the last bits as well: DESIGN.md, "Label dropout", parity).  So the conditional cases have 64 classes and give
    every sample a class of its own -- one addition per address, nothing to reorder -- and every gradient is compared."""
    distinct = num_classes is not None
    mod, state = _embedding(num_classes, label_dropout, 40 + B)
    sigma, labels, aug = _inputs(B, num_classes, 50 + B, distinct=distinct)
    gout = torch.randn(B, E_DIM, generator=torch.Generator().manual_seed(B)).to(DEV)

    def grads(a):
        _restore(mod, state)
        _, out = mod(sigma, labels, a)
        out.backward(gout)
        return {k: (None if p.grad is None else p.grad.clone()) for k, p in mod.named_parameters()}

    def same(k, a, b):
        assert torch.equal(a, b), k

    g_none, g_zero, g_rand, g_again = grads(None), grads(torch.zeros_like(aug)), grads(aug), grads(aug)
    assert g_none["aug_embed.weight"] is None
    for k in g_none:
        if k != "aug_embed.weight":
            same(k, g_zero[k], g_none[k])
    assert not g_zero["aug_embed.weight"].any()
    ga = g_rand["aug_embed.weight"]
    assert tuple(ga.shape) == (E_DIM, K_AUG) and torch.isfinite(ga).all() and float(ga.abs().max()) > 0
    for k in g_rand:
        same(k, g_rand[k], g_again[k])


# ------------------------------------------------------------------------------------------------ the whole step
def _build(augment_dim, seed=11, pdrop=0.1):
    import tinyedm_amd as T
    from oracle.make_golden import tiny_cfgs
    from tinyedm_amd import networks as N
    ecfg, dcfg = tiny_cfgs()
    N._rng_sub_counter[0] = 0
    T.manual_seed(seed)
    torch.manual_seed(seed)
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor, augment_dim=augment_dim)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), pdrop, dcfg.sigma_data,
                     dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    with torch.no_grad():
        den.gain_out.fill_(0.7)
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=True, use_uncertainty=False,
                  steady_steps=3, rampup_steps=3, scheduler_interval="step", lr=2e-3, ema_length=0.13)
    return model.to(DEV).train()


def _opt(model):
    import tinyedm_amd as T
    from tinyedm_amd.ema import EMAOptimizer
    cfg = model.configure_optimizers()
    base, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    return EMAOptimizer(base, device=DEV, gamma=T.sigma_rel_to_gamma(0.13)), base, sched


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def test_augmented_step_eager_and_captured_checkpoint_and_sampling(ops, tmp_path):
    """(x, y, augment_labels) batches through the eager step and through CapturedTrainStep (two warm-up steps, which it runs
    eagerly, then three replays of one graph) from the same state: the criterion of tests/test_graph_gpu.py for the
    un-augmented step.  Then the checkpoint round trip and sampling with nobody passing augment labels."""
    import tinyedm_amd as T
    from tinyedm_amd import networks as N
    from tinyedm_amd.graph import CapturedTrainStep
    g = torch.Generator().manual_seed(5)
    batches = []
    for i in range(5):
        _, _, aug = _inputs(8, None, 70 + i)
        batches.append(((0.5 * torch.randn(8, 3, 16, 16, generator=g)).to(DEV), torch.randint(0, 10, (8,), generator=g).to(DEV),
                        aug))
    model_e = _build(6)
    w0 = model_e.embedding.aug_embed.weight.detach().clone()
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
    model_g = _build(6)
    assert torch.equal(model_g.embedding.aug_embed.weight, w0)
    opt_g, base_g, sched_g = _opt(model_g)
    opt_g.zero_grad()
    step = CapturedTrainStep(model_g, opt_g)
    losses_g = []
    for b in batches:
        loss = step(b)
        sched_g.step()
        losses_g.append(float(loss))
    assert len(step._graphs) == 1 and len(next(iter(step._graphs))) == 4          # the key carries the third element
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
    # checkpoint round trip (the reference's key layout) and sampling without augment labels
    path = str(tmp_path / "aug.ckpt")
    torch.save({"hyper_parameters": dict(model_g.hparams), "state_dict": model_g.state_dict()}, path)
    assert model_g.hparams["embedding"]["augment_dim"] == 6
    loaded = T.EDM.load_from_checkpoint(path).to(DEV).eval()
    assert loaded.embedding.augment_dim == 6
    assert torch.equal(loaded.embedding.aug_embed.weight, model_g.embedding.aug_embed.weight)
    x0 = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
    lab = torch.arange(4, device=DEV)
    with torch.no_grad():
        img = T.DeterministicSolver(num_steps=4).solve(loaded, x0, lab)
        assert tuple(img.shape) == (4, 3, 16, 16) and torch.isfinite(img).all()
        # no labels == the all-zero label: the network's "not augmented"
        sig = torch.full((4,), 1.5, device=DEV)
        assert torch.equal(loaded(x0, sig, lab), loaded(x0, sig, lab, torch.zeros(4, 6, device=DEV)))


def test_augment_labels_into_a_network_without_them_raise(ops):
    model = _build(0)
    x = torch.zeros(4, 3, 16, 16, device=DEV)
    y = torch.zeros(4, dtype=torch.long, device=DEV)
    aug = torch.zeros(4, 6, device=DEV)
    with pytest.raises(ValueError, match="augment_dim is 0"):
        model.training_step((x, y, aug), 0)
    with pytest.raises(ValueError, match="augment_dim is 0"):
        model(x, torch.ones(4, device=DEV), y, aug)
    model6 = _build(6)
    loss = model6.training_step((x + 0.1, y), 0)                # a 2-element batch with augment_dim > 0 passes None
    assert torch.isfinite(loss)
    with pytest.raises(ValueError, match=r"shape \(B, 6\)"):
        model6.training_step((x, y, torch.zeros(4, 5, device=DEV)), 0)
