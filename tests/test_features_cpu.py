"""Denoiser features, the parts that need no GPU: the numpy restatement (tests/features_ref.py) against independent
arithmetic, the host side of the probes, tap-name parsing, every refusal of the command line, the .npy hand-over to the
tools that read --features, and the refusal of CPU tensors."""
import json

import numpy as np
import pytest
import torch

import features_ref as R
from tinyedm_amd import features as F
from tinyedm_amd import neighbors as N
from tinyedm_amd.networks import tap_positions


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("shape", [(3, 1, 1, 5), (2, 2, 2, 64), (5, 8, 8, 192), (2, 32, 32, 36), (1, 64, 64, 8), (2, 3, 5, 7),
                                   (2, 7, 7, 768), (70000, 1, 1, 4)], ids=str)
def test_dyadic_pool_is_order_free(shape):
    """the claim the exact GPU test rests on: with inputs k / 8, |k| <= 64, an fp32 running sum in any order is exact, so
    the pooled mean is one defined number"""
    x = R.eighths(sum(shape), shape)
    assert np.abs(x).max() <= 8.0 and (x * 8 == np.round(x * 8)).all()
    B, H, W, C = shape
    flat = x.reshape(B, H * W, C)
    want = R.pool(x)
    ints = (flat.astype(np.float64) * 8).astype(np.int64).sum(axis=1)            # exact integers
    assert (want == (ints / 8.0 / (H * W)).astype(np.float32)).all()
    back = flat[:, ::-1].astype(np.float32).cumsum(axis=1, dtype=np.float32)[:, -1]    # fp32, reversed order
    assert ((back.astype(np.float64) / (H * W)).astype(np.float32) == want).all()


def test_ridge_restatement_against_lstsq():
    x, y = R.blobs(seed=0)
    mu, W, ybar = R.ridge_fit(x, y, 3, l2=1e-3)
    xd = x.astype(np.float64)
    n, D = xd.shape
    Y = np.eye(3)[y]
    xc, yc = xd - xd.mean(0), Y - Y.mean(0)
    lam = 1e-3 * np.trace(xc.T @ xc / n) / D
    # ridge as ordinary least squares on the system augmented with sqrt(n lam) I rows
    A = np.vstack([xc, np.sqrt(n * lam) * np.eye(D)])
    b = np.vstack([yc, np.zeros((D, 3))])
    want = np.linalg.lstsq(A, b, rcond=None)[0]
    assert np.linalg.norm(W - want) <= 1e-10 * np.linalg.norm(want)
    assert np.allclose(mu, xd.mean(0), rtol=0, atol=1e-15 * np.abs(xd).max() * n) and (ybar == 1 / 3).all()
    for seed in (1, 2):
        xt, yt = R.blobs(seed=seed)
        assert (R.ridge_predict((mu, W, ybar), xt) == yt).all()
        assert (R.knn_predict(x, y, xt, 20, 3) == yt).all()


def test_ridge_solve_is_the_restatement():
    """features.ridge_solve (the host half of ridge_probe) from fp64 moments equals the restatement from the rows"""
    x, y = R.blobs(seed=3)
    xd = x.astype(np.float64)
    sums = np.stack([xd[y == c].sum(0) for c in range(3)])
    mu, W, ybar = F.ridge_solve(len(x), xd.sum(0), xd.T @ xd, sums, np.bincount(y), 1e-3)
    rm, rW, rb = R.ridge_fit(x, y, 3, 1e-3)
    assert np.linalg.norm(W - rW) <= 1e-10 * np.linalg.norm(rW) and np.allclose(mu, rm, rtol=1e-14) and (ybar == rb).all()
    with pytest.raises(ValueError, match="constant"):
        F.ridge_solve(4, np.ones(2) * 4, np.ones((2, 2)) * 4, np.ones((2, 2)) * 2, [2, 2], 1e-3)
    for l2 in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="l2"):
            F.ridge_solve(len(x), xd.sum(0), xd.T @ xd, sums, np.bincount(y), l2)


# ------------------------------------------------------------------------------------------------ the vote
VOTES = [([0, 0, 1], 0), ([1, 0, 0], 0), ([1, 0, 0, 1], 1), ([2, 1, 1, 2, 0], 2), ([2, 0, 1], 2), ([0], 0),
         ([1, 2, 2, 1, 0, 0], 1), ([3, 3, 3, 0, 0, 0, 0], 0)]


def test_vote_rules():
    """majority; a tied vote goes to the class of the nearest neighbour among the tied classes"""
    for row, want in VOTES:
        assert R.vote([row], 4).tolist() == [want], row
        assert F.knn_vote(torch.tensor([row]), 4).tolist() == [want], row
    table = torch.tensor([[1, 0, 0, 1], [0, 1, 1, 0], [2, 2, 1, 1], [3, 0, 0, 3]])
    assert F.knn_vote(table, 4).tolist() == R.vote(table.numpy(), 4).tolist() == [1, 0, 2, 3]
    # distance ties go to the lower index in the restatement's search, as ops.f32_knn gives them
    idx = R.knn_indices(np.array([[2.0, 0], [1.0, 0], [0, 1.0]]), np.array([[1.0, 0]]), 2)
    assert idx.tolist() == [[0, 1]]
    assert F._first_max(torch.tensor([[0.5, 0.5, 0.1], [0.1, 0.7, 0.7], [3.0, 1.0, 2.0]])).tolist() == [0, 1, 0]


# ------------------------------------------------------------------------------------------------ tap names
def test_tap_names():
    assert tap_positions(("enc0", "mid", "dec0", "dec12"), 8, 13) == {"enc0": 0, "mid": 7, "dec0": 8, "dec12": 20}
    assert list(tap_positions(["dec1", "enc2"], 3, 5)) == ["dec1", "enc2"]          # the order given is kept
    assert tap_positions("mid", 3, 5) == {"mid": 2}
    for bad in ((), [], ("enc8",), ("dec13",), ("enc",), ("mid0",), ("enc-1",), ("enc01",), ("enc1 ",), ("Enc1",),
                ("enc0", "enc0"), ("mid", "enc7"), (None,), (0,), None, 5, ("enc١",)):
        with pytest.raises(ValueError, match='"enc0" .. "enc7", "dec0" .. "dec12" or "mid"'):
            tap_positions(bad, 8, 13)


# ------------------------------------------------------------------------------------------------ command line
EXTRACT = ["--ckpt_path", "a.ckpt", "--dataset", "cifar10", "--data_dir", "d", "--out", "f.npy"]
PROBE = ["--probe", "--ckpt_path", "a.ckpt", "b.ckpt", "--dataset", "cifar10", "--data_dir", "d", "--report", "p.json"]


def _check(argv):
    F.check_args(F.build_parser().parse_args(argv))


def test_cli_accepts():
    _check(EXTRACT)
    _check(EXTRACT + ["--split", "test", "--taps", "enc5", "mid", "--sigma", "0.2", "--network_dtype", "f32", "--conditional",
                      "--labels_out", "l.json", "--num_images", "100", "--load_ema"])
    _check(["--ckpt_path", "a.ckpt", "--image_dir", "s", "--out", "f.npy"])
    _check(["--ckpt_path", "a.ckpt", "--image_dir", "s", "--out", "f.npy", "--conditional", "--labels_json", "l.json"])
    _check(PROBE)
    _check(PROBE + ["--sweep_sigmas", "0.05", "0.1", "--sweep_taps", "enc3", "mid", "--k", "5", "--l2", "0.01",
                    "--num_train", "1000", "--num_test", "500"])


REFUSALS = [
    (PROBE[:4] + ["--image_dir", "s", "--report", "p.json"], "--probe needs the labelled"),
    (["--ckpt_path", "a.ckpt", "--image_dir", "s", "--out", "f.npy", "--conditional"], "--conditional needs labels"),
    (EXTRACT + ["--network_dtype", "bf16"], "reference precision"),
    (EXTRACT[:-2], "needs --out"),
    (EXTRACT + ["--image_dir", "s"], "exactly one data source"),
    (["--ckpt_path", "a.ckpt", "--out", "f.npy"], "exactly one data source"),
    (["--ckpt_path", "a.ckpt", "--dataset", "mnist", "--out", "f.npy"], "--dataset needs --data_dir"),
    (["--ckpt_path", "a.ckpt", "--image_dir", "s", "--data_dir", "d", "--out", "f.npy"], "--data_dir goes with --dataset"),
    (["--ckpt_path", "a.ckpt", "--image_dir", "s", "--split", "test", "--out", "f.npy"], "--split goes with --dataset"),
    (EXTRACT + ["--labels_json", "l.json"], "--labels_json goes with --image_dir"),
    (["--ckpt_path", "a.ckpt", "--image_dir", "s", "--out", "f.npy", "--labels_out", "l.json"], "--labels_out has no labels"),
    (EXTRACT + ["--sigma", "0"], "finite and > 0"),
    (EXTRACT + ["--sigma", "nan"], "finite and > 0"),
    (EXTRACT + ["--sigma", "1e-60"], "finite and > 0"),
    (EXTRACT + ["--batch_size", "0"], "--batch_size"),
    (EXTRACT + ["--num_images", "0"], "--num_images"),
    (EXTRACT + ["--seed", "-1"], "--seed"),
    (EXTRACT + ["--taps", "mid", "mid"], "names a tap twice"),
    (EXTRACT + ["--ckpt_path", "a.ckpt", "b.ckpt"], "one --ckpt_path"),
    (EXTRACT + ["--sweep_sigmas", "0.1"], "--sweep_sigmas goes with --probe"),
    (EXTRACT + ["--report", "p.json"], "--report goes with --probe"),
    (EXTRACT + ["--num_train", "5"], "--num_train goes with --probe"),
    (PROBE + ["--out", "f.npy"], "--out belongs to extraction"),
    (PROBE + ["--split", "test"], "--split belongs to extraction"),
    (PROBE[:-2], "--probe needs --report"),
    (PROBE + ["--ckpt_path", "a.ckpt", "a.ckpt"], "names a checkpoint twice"),
    (PROBE + ["--sweep_sigmas", "0.1", "-1"], "finite and > 0"),
    (PROBE + ["--sweep_sigmas", "0.1", "0.1"], "lists a value twice"),
    (PROBE + ["--sweep_taps", "mid", "mid"], "lists a value twice"),
    (PROBE + ["--k", "0"], "--k must be"),
    (PROBE + ["--k", "33"], "--k must be"),
    (PROBE + ["--k", "20", "--num_train", "10"], "at least that many training images"),
    (PROBE + ["--l2", "0"], "--l2"),
]


@pytest.mark.parametrize("argv,message", REFUSALS, ids=[m for _, m in REFUSALS])
def test_cli_refuses(argv, message):
    """contradictory flags are refused before a checkpoint or the GPU is touched"""
    with pytest.raises(ValueError, match=message):
        _check(argv)


def test_cli_refusal_reaches_the_user(capsys):
    with pytest.raises(SystemExit) as e:
        F.main(EXTRACT + ["--network_dtype", "bf16"])
    assert e.value.code == 2 and "reference precision" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ the hand-over
def test_npy_round_trip(tmp_path):
    feats = np.random.default_rng(0).standard_normal((7, 5)).astype(np.float32)
    path = tmp_path / "feats.npy"
    F.write_features(str(path), torch.from_numpy(feats))
    back = N.read_features(str(path), "--features", "frechet")
    assert back.dtype == np.float32 and back.flags.c_contiguous and (back == feats).all()
    F.write_features(str(tmp_path / "noext"), feats)                      # the name is taken as given
    assert (tmp_path / "noext").exists() and not (tmp_path / "noext.npy").exists()
    for bad in (feats.astype(np.float64), feats[0], np.full((2, 2), np.nan, np.float32)):
        with pytest.raises(ValueError, match="float32"):
            F.write_features(str(tmp_path / "bad.npy"), bad)


def test_report_table():
    cells = [{"checkpoint": "a.ckpt", "sigma": 0.1, "tap": "mid", "dim": 256, "ridge_accuracy": 0.5, "knn_accuracy": 0.4},
             {"checkpoint": "b.ckpt", "sigma": 0.2, "tap": "enc5", "dim": 256, "ridge_accuracy": 0.75, "knn_accuracy": 0.3},
             {"checkpoint": "b.ckpt", "sigma": 0.4, "tap": "enc5", "dim": 256, "ridge_accuracy": 0.75, "knn_accuracy": 0.6}]
    assert F.best_cell(cells) is cells[1] and F.best_cell(cells, "knn_accuracy") is cells[2]
    text = F.format_table(cells)
    assert len(text.splitlines()) == 4 and "0.7500" in text and "enc5" in text
    json.dumps(cells)


# ------------------------------------------------------------------------------------------------ no CPU path
def test_cpu_tensors_raise():
    from tinyedm_amd import ops
    with pytest.raises(ValueError, match="expected a CUDA/HIP tensor -- tinyedm_amd has no CPU path"):
        ops.f32_pool_features(torch.zeros(1, 2, 2, 4))
    x, y = R.blobs()
    with pytest.raises(ValueError, match="tinyedm_amd has no CPU path"):
        F.ridge_probe(torch.from_numpy(x), y, 3)
    with pytest.raises(ValueError, match="tinyedm_amd has no CPU path"):
        F.knn_accuracy(torch.from_numpy(x), y, torch.from_numpy(x), y, 5, num_classes=3)
    import tinyedm_amd as T
    from oracle.make_golden import tiny_cfgs
    ecfg, dcfg = tiny_cfgs(num_classes=None)
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), dcfg.dropout_rate,
                     dcfg.sigma_data, dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    den.eval().set_eval_dtype("f32x3")
    with pytest.raises(RuntimeError, match="no CPU path"):
        den.forward_taps(torch.zeros(1, 3, 8, 8), torch.ones(1), torch.zeros(1, 64), ("mid",))
    with pytest.raises(ValueError, match="reference precision"):
        den.set_eval_dtype("bf16").forward_taps(torch.zeros(1, 3, 8, 8), torch.ones(1), torch.zeros(1, 64), ("mid",))
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                  steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01)
    ex = F.FeatureExtractor(model, taps=("enc1", "dec4"))
    assert ex.dim == 128 + 64 and ex.taps == ("enc1", "dec4") and ex.network_dtype == "f32x3" and ex.sigma == 0.1
    with pytest.raises(ValueError, match="on the GPU"):
        ex.extract(torch.zeros(2, 3, 8, 8))
    with pytest.raises(ValueError, match="conditional=True needs a class-conditional model"):
        F.FeatureExtractor(model, conditional=True)
    for kw in (dict(network_dtype="bf16"), dict(sigma=0), dict(sigma=float("inf")), dict(taps=("enc3",)), dict(taps=())):
        with pytest.raises(ValueError):
            F.FeatureExtractor(model, **kw)
