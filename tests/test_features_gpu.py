"""Denoiser features on the GPU: the pool kernel against the numpy restatement (exact on dyadic inputs, within a derived
bound on random ones, placed where it is told to), the taps against the fp32 CPU oracle's per-block record, the truncation
of the forward, the extractor's batch invariance, the existing feature-space tools as consumers, the two probes, and the
command line end to end (extract, frechet --features on the files, a probe sweep)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import features_ref as R
import frechet_ref
from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs
from parity_log import record

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _model(P, ecfg, dcfg, dtype="f32x3"):
    import tinyedm_amd as T
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), dcfg.dropout_rate,
                     dcfg.sigma_data, dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    emb.load_state_dict({k[len("embedding."):]: v for k, v in P.items() if k.startswith("embedding.")})
    den.load_state_dict({k[len("denoiser."):]: v for k, v in P.items() if k.startswith("denoiser.")})
    den.set_eval_dtype(dtype)
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                  steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01)
    return model.to(DEV).eval()


def _small_cfg():
    """one EncD and one DecU, an attention block on each side, widths 64 and 128, conditional with 3 classes"""
    return tiny_cfgs(num_classes=3)


@pytest.fixture(scope="module")
def small():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ecfg, dcfg = _small_cfg()
    P = O.init_params(ecfg, dcfg, torch.Generator().manual_seed(5), gains_nonzero=True)
    return P, ecfg, dcfg, _model(P, ecfg, dcfg)


# ------------------------------------------------------------------------------------------------ 1-3: the pool kernel
@pytest.mark.parametrize("shape", [(3, 1, 1, 5), (2, 2, 2, 64), (5, 8, 8, 192), (2, 32, 32, 36), (1, 64, 64, 8), (2, 3, 5, 7),
                                   (2, 7, 7, 768), (70000, 1, 1, 4)], ids=str)
def test_pool_exact(ops, shape):
    """inputs k / 8 with |k| <= 64: every partial sum is exact in any order, so the result is one defined number"""
    x = R.eighths(sum(shape), shape)
    got = ops.f32_pool_features(torch.from_numpy(x).to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == (shape[0], shape[3]) and got.is_contiguous()
    assert torch.equal(got.cpu(), torch.from_numpy(R.pool(x)))


def test_pool_placement(ops):
    B, C, Dtot, canary = 3, 7, 40, -777.25
    x = torch.from_numpy(R.eighths(9, (B, 3, 5, C))).to(DEV)
    alone = ops.f32_pool_features(x)
    for offset in (0, 3, 33):
        out = torch.full((B, Dtot), canary, dtype=torch.float32, device=DEV)
        assert ops.f32_pool_features(x, out, offset) is out
        assert torch.equal(out[:, offset:offset + C], alone)
        rest = torch.ones(Dtot, dtype=torch.bool, device=DEV)
        rest[offset:offset + C] = False
        assert bool((out[:, rest] == canary).all()), f"offset {offset}: a column outside [offset, offset + C) was written"
    before = ops._lib.N_CALLS
    out = torch.full((B, Dtot), canary, dtype=torch.float32, device=DEV)
    bad = [dict(out=out, offset=Dtot - C + 1), dict(out=out, offset=-1), dict(out=out.t().contiguous().t(), offset=0),
           dict(out=torch.empty(B, 2 * Dtot, device=DEV)[:, ::2], offset=0), dict(out=out.double(), offset=0),
           dict(out=out.cpu(), offset=0), dict(out=out[:2], offset=0), dict(out=None, offset=3)]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.f32_pool_features(x, **kw)
    for xbad in (x.cpu(), x.double(), x[:, :, :, ::2], x[0]):
        with pytest.raises(ValueError):
            ops.f32_pool_features(xbad)
    assert ops._lib.N_CALLS == before, "a refused call reached the library"
    assert bool((out == canary).all())


@pytest.mark.parametrize("shape", [(4, 64, 64, 64), (3, 7, 7, 100)], ids=str)
def test_pool_random(ops, shape):
    """standard-normal data against the fp64 mean: |err| <= 2^-24 |mean| + HW 2^-52 mean_p |x| (derived: one rounding to
    fp32 plus the fp64 accumulation), and row b does not depend on the batch it came in"""
    x = np.random.default_rng(shape[3]).standard_normal(shape).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    got = ops.f32_pool_features(xd)
    want = x.reshape(shape[0], -1, shape[3]).astype(np.float64).mean(axis=1)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    bound = R.pool_bound(x)
    worst = float((err / bound).max())
    print(f"pool {shape}: worst err / bound {worst:.3f}")
    record(f"features/pool_random_{'x'.join(map(str, shape))}", worst, 1.0)
    assert (err <= bound).all()
    for b in range(shape[0]):
        assert torch.equal(ops.f32_pool_features(xd[b:b + 1]), got[b:b + 1]), f"row {b} depends on the batch"


# ------------------------------------------------------------------------------------------------ 4: taps vs the oracle
@pytest.mark.parametrize("which", ["cifar10", "small"])
def test_taps_against_oracle(which):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if which == "cifar10":
        ecfg, dcfg = O.cifar10_cfg()
        B, hw, labels = 3, 32, None
    else:
        ecfg, dcfg = _small_cfg()
        B, hw = 2, 16
        labels = torch.tensor([2, 0])
    P = O.init_params(ecfg, dcfg, torch.Generator().manual_seed(31), gains_nonzero=True)
    g = torch.Generator().manual_seed(8)
    noisy = torch.randn(B, 3, hw, hw, generator=g) * 1.3
    sigma = torch.exp(torch.randn(B, generator=g) * 1.2 - 1.2)
    rec = {}
    with torch.no_grad():
        _, emb = O.embedding_forward(P, ecfg, sigma, labels)
        O.denoiser_forward(P, dcfg, noisy, sigma, emb, False, False, record=rec)
    n_enc, n_dec = len(dcfg.encoder_block_types), len(dcfg.decoder_block_types)
    prefix = {"enc0": "denoiser.encoder_blocks.0.", "mid": f"denoiser.encoder_blocks.{n_enc - 1}.",
              "dec0": "denoiser.decoder_blocks.0.", f"dec{n_dec - 1}": f"denoiser.decoder_blocks.{n_dec - 1}."}
    model = _model(P, ecfg, dcfg, "f32")
    for dtype in ("f32", "f32x3"):
        model.denoiser.set_eval_dtype(dtype)
        taps = model.forward_taps(noisy.to(DEV), sigma.to(DEV), None if labels is None else labels.to(DEV), tuple(prefix))
        assert list(taps) == list(prefix)
        for name, p in prefix.items():
            t = taps[name]
            assert t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()
            e = rel(t.permute(0, 3, 1, 2).cpu(), rec[p])
            print(f"{which} {dtype} {name}: rel L2 vs the fp32 oracle {e:.3e}")
            record(f"features/{which}_{dtype}_{name}_vs_fp32_oracle", e, 1e-4)
            assert e <= 1e-4, (which, dtype, name, e)


# ------------------------------------------------------------------------------------------------ 5: truncation
def test_truncation(small, monkeypatch):
    _, _, _, model = small
    g = torch.Generator().manual_seed(2)
    noisy = (torch.randn(2, 3, 16, 16, generator=g) * 0.6).to(DEV)
    sigma = torch.tensor([0.1, 0.3], device=DEV)
    labels = torch.tensor([1, 2], device=DEV)
    names = ("enc0", "mid", "dec0", "dec4")
    both = model.forward_taps(noisy, sigma, labels, names)
    for n in names:
        one = model.forward_taps(noisy, sigma, labels, (n,))
        assert list(one) == [n] and torch.equal(one[n], both[n]), n
    with torch.no_grad():                     # a full forward between tapped runs is undisturbed and disturbs nothing
        assert torch.equal(model(noisy, sigma, labels), model(noisy, sigma, labels))
    assert torch.equal(model.forward_taps(noisy, sigma, labels, ("dec4",))["dec4"], both["dec4"])

    class Stop(Exception):
        pass

    def boom(*a, **k):
        raise Stop()
    den = model.denoiser
    monkeypatch.setattr(den.decoder_blocks[0], "forward_f32", boom)
    got = model.forward_taps(noisy, sigma, labels, ("enc0", "mid"))
    assert torch.equal(got["enc0"], both["enc0"]) and torch.equal(got["mid"], both["mid"])
    with pytest.raises(Stop):
        model.forward_taps(noisy, sigma, labels, ("dec0",))
    monkeypatch.undo()
    # refusals: unknown / empty / duplicate names, the bf16 path, training mode
    for bad in ((), ("enc3",), ("dec5",), ("mid", "enc2"), ("enc0", "enc0"), ("encoder0",), ("enc-1",), (3,)):
        with pytest.raises(ValueError, match="enc0"):
            model.forward_taps(noisy, sigma, labels, bad)
    den.set_eval_dtype("bf16")
    try:
        with pytest.raises(ValueError, match="reference precision"):
            model.forward_taps(noisy, sigma, labels, ("mid",))
    finally:
        den.set_eval_dtype("f32x3")
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.forward_taps(noisy.cpu(), sigma.cpu(), labels.cpu(), ("mid",))


# ------------------------------------------------------------------------------------------------ 6: the extractor
def test_extractor(ops, small):
    from tinyedm_amd.features import FeatureExtractor
    _, _, _, model = small
    rng = np.random.default_rng(3)
    images = torch.from_numpy(rng.integers(0, 256, size=(12, 32, 32, 3), dtype=np.uint8))
    taps = ("enc0", "mid")
    ex = FeatureExtractor(model, sigma=0.1, taps=taps, seed=4, batch_size=12)
    assert ex.dim == 64 + 128
    model.train()
    f12 = ex.extract(images)
    assert model.training and model.denoiser.eval_dtype == "f32x3"
    model.eval()
    assert f12.dtype == torch.float32 and tuple(f12.shape) == (12, 192) and f12.is_contiguous() and f12.is_cuda
    assert bool(torch.isfinite(f12).all())
    for bs in (5, 1):
        assert torch.equal(FeatureExtractor(model, 0.1, taps, 4, bs).extract(images), f12), f"batch_size {bs} changed bits"
    assert torch.equal(ex.extract(images), f12)
    perm = rng.permutation(12)
    assert torch.equal(ex.extract(images[perm], ids=perm), f12[torch.from_numpy(perm).to(DEV)])
    assert not torch.equal(FeatureExtractor(model, 0.1, taps, 5, 12).extract(images), f12)
    assert not torch.equal(FeatureExtractor(model, 0.2, taps, 4, 12).extract(images), f12)
    # by hand: normalise, noise image i with the stream (seed, i), tap, pool each tap into its columns
    dev = f12.device
    clean = ops.u8_gather_normalize(images.to(dev).permute(0, 3, 1, 2).contiguous(), torch.arange(12, device=dev), 0.5, 0.5)
    noisy, sigma = ops.eval_diffuse(clean, torch.from_numpy(np.arange(12, dtype=np.uint32)).to(dev),
                                    torch.zeros(12, dtype=torch.int32, device=dev),
                                    torch.tensor([0.1], dtype=torch.float32, device=dev), ops.churn_record(4, 0, dev))
    maps = model.forward_taps(noisy, sigma, None, taps)
    hand = torch.cat([ops.f32_pool_features(maps[t]) for t in taps], dim=1)
    assert torch.equal(hand, f12)
    # float images in network range give the same rows
    assert torch.equal(ex.extract(clean), f12)
    # conditional features differ from label-free ones and need labels
    labels = torch.arange(12) % 3
    fc = FeatureExtractor(model, 0.1, taps, 4, 5, conditional=True).extract(images, labels)
    assert tuple(fc.shape) == (12, 192) and not torch.equal(fc, f12)
    with pytest.raises(ValueError, match="labels"):
        FeatureExtractor(model, 0.1, taps, 4, 5, conditional=True).extract(images)
    for kw in (dict(network_dtype="bf16"), dict(sigma=0.0), dict(sigma=float("nan")), dict(sigma=-1.0), dict(taps=("enc9",)),
               dict(taps=()), dict(batch_size=0), dict(seed=-1)):
        with pytest.raises(ValueError):
            FeatureExtractor(model, **kw)
    with pytest.raises(ValueError, match="distinct"):
        ex.extract(images, ids=[0] * 12)


# ------------------------------------------------------------------------------------------------ 7: the consumers
def test_consumers_accept_features(small):
    from tinyedm_amd import frechet, neighbors, prdc
    from tinyedm_amd.features import FeatureExtractor
    _, _, _, model = small
    rng = np.random.default_rng(11)
    ex = FeatureExtractor(model, sigma=0.1, taps=("mid",), batch_size=32)
    refs = ex.extract(torch.from_numpy(rng.integers(0, 256, size=(64, 32, 32, 3), dtype=np.uint8)))
    samples = ex.extract(torch.from_numpy(rng.integers(0, 256, size=(48, 32, 32, 3), dtype=np.uint8)))
    dd = frechet.DistributionDistance(refs)
    fd = dd.score(samples, kid=False)["fd"]
    assert np.isfinite(fd["fd"]) and np.isfinite(fd["mean_term"]) and fd["mean_term"] > 0.0
    m = prdc.ManifoldMetrics(refs, k=3).score(samples)[3]
    assert all(np.isfinite(m[key]) for key in ("precision", "recall", "density", "coverage"))
    nn = neighbors.NearestNeighbors(refs, k=2)
    dist, idx = nn.search(samples)
    assert bool(torch.isfinite(dist).all()) and tuple(idx.shape) == (48, 2)
    # a set against itself: distance 0 up to the rounding of two equal covariances, nearest distance +0.0 exactly
    own = dd.score(refs, kid=False)["fd"]
    cov = np.cov(refs.cpu().numpy().astype(np.float64), rowvar=False)
    assert own["mean_term"] == 0.0 and abs(own["fd"]) <= frechet_ref.trace_term_bound(cov, cov)
    d0, i0 = nn.search(refs, k=1)
    assert bool((d0 == 0).all()) and not bool(torch.signbit(d0).any())
    assert i0.flatten().tolist() == list(range(64))


# ------------------------------------------------------------------------------------------------ 8: the probes
def test_probes(ops):
    from tinyedm_amd import features as F
    xtr, ytr = R.blobs(seed=0)
    xte, yte = R.blobs(seed=1)
    dtr, dte = torch.from_numpy(xtr).to(DEV), torch.from_numpy(xte).to(DEV)
    want = R.ridge_predict(R.ridge_fit(xtr, ytr, 3), xte)
    probe = F.ridge_probe(dtr, ytr, 3)
    assert (want == yte).all() and probe.predict(dte).cpu().numpy().tolist() == want.tolist()
    assert probe.accuracy(dte, yte) == 1.0 and probe.accuracy(dte, torch.from_numpy(yte).to(DEV)) == 1.0
    fit = R.ridge_fit(xtr, ytr, 3)
    for got, ref in zip((probe.mean, probe.W, probe.prior), fit):
        assert np.abs(got.cpu().numpy() - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    wk = R.knn_predict(xtr, ytr, xte, 20, 3)
    assert (wk == yte).all()
    assert F.knn_predict(dtr, ytr, dte, 20, num_classes=3).cpu().numpy().tolist() == wk.tolist()
    assert F.knn_accuracy(dtr, ytr, dte, yte, 20, num_classes=3) == 1.0
    # an exact logit tie: the query is the training mean (exactly representable), so every logit is the prior 1/2
    tx = torch.tensor([[1.0, 0.0], [3.0, 0.0], [-1.0, 0.0], [-3.0, 0.0]], device=DEV)
    ty = torch.tensor([1, 1, 0, 0])
    tie = F.ridge_probe(tx, ty, 2)
    assert tie.predict(torch.tensor([[0.0, 0.0], [0.5, 0.0], [-0.5, 0.0]], device=DEV)).tolist() == [0, 1, 0]
    # an exact vote tie: k = 4 finds two rows of each class; the nearest row is of class 1, the lower class is 0
    kx = torch.tensor([[1.0, 0.00], [1.0, 0.10], [1.0, 0.20], [1.0, 0.30], [1.0, 5.0]], device=DEV)
    ky = torch.tensor([1, 0, 0, 1, 2])
    q = torch.tensor([[1.0, 0.0]], device=DEV)
    assert F.knn_predict(kx, ky, q, 4, num_classes=3).tolist() == [1]
    assert F.knn_predict(kx, ky, q, 3, num_classes=3).tolist() == [0]          # no tie at k = 3: two votes for class 0
    # a distance tie goes to the lower index: rows 0 and 1 coincide once normalised, k = 1 takes row 0
    assert F.knn_predict(torch.tensor([[2.0, 0.0], [1.0, 0.0], [0.0, 1.0]], device=DEV), torch.tensor([1, 0, 2]),
                         q, 1, num_classes=3).tolist() == [1]
    # refusals
    for fn in (lambda **kw: F.ridge_probe(kw["x"], kw["y"], kw["K"]),
               lambda **kw: F.knn_predict(kw["x"], kw["y"], dte, 1, num_classes=kw["K"])):
        with pytest.raises(ValueError, match=r"\[0, 3\)"):
            fn(x=dtr, y=np.where(ytr == 2, 3, ytr), K=3)
        with pytest.raises(ValueError, match=r"\[0, 3\)"):
            fn(x=dtr, y=np.where(ytr == 2, -1, ytr), K=3)
        with pytest.raises(ValueError, match="fewer rows than classes"):
            fn(x=dtr[:2], y=ytr[:2], K=3)
        with pytest.raises(ValueError, match="no training row of class 2"):
            fn(x=dtr, y=np.where(ytr == 2, 1, ytr), K=3)
        with pytest.raises(ValueError, match="no CPU path"):
            fn(x=dtr.cpu(), y=ytr, K=3)
    with pytest.raises(ValueError, match="k must be"):
        F.knn_predict(dtr, ytr, dte, 33, num_classes=3)


# ------------------------------------------------------------------------------------------------ 9: the command line
def test_cli_end_to_end(small, tmp_path):
    """extract twice (a PNG directory, a built-in split), hand both files to tinyedm.frechet --features, then a probe sweep;
    all in this process (a child would spend its seconds on imports)"""
    import json
    import pickle
    from PIL import Image
    from tinyedm_amd import features as F
    from tinyedm_amd import frechet, neighbors
    _, _, _, model = small
    ckpt = str(tmp_path / "small.ckpt")
    torch.save({"hyper_parameters": dict(model.hparams), "state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, ckpt)
    rng = np.random.default_rng(21)
    png = tmp_path / "png"
    png.mkdir()
    for i in range(10):
        Image.fromarray(rng.integers(0, 256, size=(32, 32, 3), dtype=np.uint8)).save(png / f"{i}.png")
    batches = tmp_path / "data" / "cifar-10-batches-py"
    batches.mkdir(parents=True)
    for name in [f"data_batch_{i}" for i in range(1, 6)] + ["test_batch"]:       # six labelled images a file, three classes
        data = rng.integers(0, 256, size=(6, 3072), dtype=np.uint8)
        lab = [0, 1, 2, 0, 1, 2]
        for r, c in enumerate(lab):                                              # (a block of one colour plane tells the class)
            data[r, c * 1024:(c + 1) * 1024] //= 4
        with open(batches / name, "wb") as f:
            pickle.dump({b"data": data, b"labels": lab}, f)
    a, b = str(tmp_path / "samples.npy"), str(tmp_path / "train.npy")
    lab_out = str(tmp_path / "train_labels.json")
    fa = F.main(["--ckpt_path", ckpt, "--image_dir", str(png), "--out", a, "--taps", "enc1", "mid", "--batch_size", "4"])
    fb = F.main(["--ckpt_path", ckpt, "--dataset", "cifar10", "--data_dir", str(tmp_path / "data"), "--split", "train", "--out", b,
                 "--taps", "enc1", "mid", "--labels_out", lab_out, "--num_images", "24"])
    ra, rb = neighbors.read_features(a, "--features", "frechet"), neighbors.read_features(b, "--ref_features", "frechet")
    assert ra.shape == (10, 256) and rb.shape == (24, 256)
    assert (ra == fa.cpu().numpy()).all() and (rb == fb.cpu().numpy()).all()
    with open(lab_out) as f:
        assert json.load(f) == [0, 1, 2] * 8
    rep = frechet.main(["--features", a, "--ref_features", b, "--no_kid", "--num_subsets", "0", "--report", str(tmp_path / "fd.json")])
    assert np.isfinite(rep["samples"]["fd"]["fd"]) and rep["feature_dim"] == 256
    report = F.main(["--probe", "--ckpt_path", ckpt, "--dataset", "cifar10", "--data_dir", str(tmp_path / "data"), "--sweep_sigmas",
                     "0.1", "0.4", "--sweep_taps", "enc0", "mid", "--k", "3", "--report", str(tmp_path / "probe.json")])
    with open(tmp_path / "probe.json") as f:
        assert json.load(f) == report
    assert report["num_train"] == 30 and report["num_test"] == 6 and report["num_classes"] == 3 and len(report["cells"]) == 4
    assert [(c["sigma"], c["tap"]) for c in report["cells"]] == [(0.1, "enc0"), (0.1, "mid"), (0.4, "enc0"), (0.4, "mid")]
    assert all(0.0 <= c[key] <= 1.0 for c in report["cells"] for key in ("ridge_accuracy", "knn_accuracy"))
    assert report["best"] in report["cells"]
