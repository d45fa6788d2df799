"""Host-side checks of the diffusion classifier (no GPU): every host function of tinyedm_amd/classify.py against the
restatements of tests/classify_ref.py, the tie rule, the refusal of non-finite scores, the shard merge, the statistics
of a hand-written matrix, the weights' closed forms, every argument error before anything is loaded, and the new entry
points in the header."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import classify_ref as R
from parity_log import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 3, 5, 4), (1, 1, 7, 2), (3, 4, 33, 10), (1, 2, 6, 1)]


def _C():
    import tinyedm_amd.classify as C
    return C


def _se(R_=2, L=3, n=5, C=4, seed=3):
    g = np.random.default_rng(seed)
    scale = np.array([1e-3, 1.0, 1e3, 7.0])[np.arange(L) % 4]
    return g.uniform(0.5, 40.0, size=(R_, L, n, C)) * scale[None, :, None, None]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("weighting", ["edm", "eps", "uniform"])
def test_host_functions_vs_restatement(shape, weighting):
    K = _C()
    se, chw = _se(*shape), 48
    sigmas = [0.05 * 4.0 ** l for l in range(shape[1])]
    w = K.class_weights(sigmas, weighting, 0.5)
    w_ref = R.class_weights(sigmas, weighting, 0.5)
    assert w.dtype == np.float64 and np.abs(w - w_ref).max() <= 1e-12 * np.abs(w_ref).max()
    sc, sc_ref = K.class_scores(se, chw, w), R.class_scores(se, chw, w_ref)
    assert sc.shape == (shape[2], shape[3]) and sc.dtype == np.float64
    err = float((np.abs(sc - sc_ref) / sc_ref).max())
    record(f"classify/scores_{'x'.join(map(str, shape))}_{weighting}_rel", err, 1e-12)
    assert err <= 1e-12
    pred, margin = K.predict(sc)
    p_ref, m_ref = R.predict(sc)
    assert pred.dtype == np.int64 and margin.dtype == np.float64
    assert np.array_equal(pred, p_ref) and np.array_equal(margin, m_ref)           # the same subtraction of the same numbers
    if shape[3] == 1:
        assert np.isinf(margin).all() and not pred.any()
    else:
        assert (margin >= 0).all()
    lp = K.level_predictions(se)
    assert lp.shape == (shape[1], shape[2]) and lp.dtype == np.int64 and np.array_equal(lp, R.level_predictions(se))
    labels = np.random.default_rng(1).integers(0, shape[3], size=shape[2])
    cm = K.confusion_matrix(pred, labels, shape[3])
    assert cm.dtype == np.int64 and np.array_equal(cm, R.confusion_matrix(pred, labels, shape[3]))
    assert cm.sum() == shape[2] and np.array_equal(cm.sum(axis=1), np.bincount(labels, minlength=shape[3]))
    st, st_ref = K.classification_stats(cm), R.classification_stats(cm)
    assert st["count"] == st_ref["count"] and st["per_class_accuracy"] == st_ref["per_class_accuracy"]
    assert abs(st["accuracy"] - st_ref["accuracy"]) <= 1e-15
    assert st["accuracy_stderr"] == pytest.approx(st_ref["accuracy_stderr"], rel=1e-12, abs=0.0)


def test_level_sum_is_sequential_in_level_order():
    """class_scores adds the levels one after the other: the bits of the left-to-right sum, not of a pairwise one"""
    K = _C()
    se = _se(1, 9, 6, 3, seed=8)
    w = K.class_weights([0.01 * 3.0 ** l for l in range(9)], "edm", 0.5)
    want = np.zeros((6, 3))
    for l in range(9):
        want = want + w[l] * (se[0, l] / 12.0)
    assert np.array_equal(K.class_scores(se, 12, w), want)


def test_exact_tie_goes_to_the_lower_index():
    K = _C()
    scores = np.array([[3.0, 1.0, 1.0, 2.0], [0.5, 0.5, 0.5, 0.5], [2.0, 4.0, 2.0, 1.5], [9.0, 8.0, 7.0, 7.0]])
    pred, margin = K.predict(scores)
    assert pred.tolist() == [1, 0, 3, 2] and margin.tolist() == [0.0, 0.0, 0.5, 0.0]
    se = np.zeros((2, 2, 1, 3))
    se[:, 0, 0] = [4.0, 2.0, 2.0]
    se[0, 1, 0], se[1, 1, 0] = [1.0, 5.0, 3.0], [3.0, 5.0, 1.0]        # the means over the draws tie: 2, 5, 2
    assert K.level_predictions(se).tolist() == [[1], [0]]
    assert R.predict(scores)[0].tolist() == [1, 0, 3, 2] and R.level_predictions(se).tolist() == [[1], [0]]


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_nonfinite_scores_are_refused(bad):
    K = _C()
    scores = np.ones((3, 4))
    scores[1, 2] = bad
    with pytest.raises(ValueError, match="finite"):
        K.predict(scores)
    se = np.ones((1, 2, 3, 4))
    se[0, 1, 2, 3] = bad
    with pytest.raises(ValueError, match="finite"):
        K.level_predictions(se)


def test_merging_two_shards_gives_the_whole():
    K = _C()
    g = np.random.default_rng(5)
    pred, labels = g.integers(0, 7, size=101), g.integers(0, 7, size=101)
    whole = K.confusion_matrix(pred, labels, 7)
    parts = [K.confusion_matrix(pred[r::2], labels[r::2], 7) for r in range(2)]        # ids = rank (mod 2)
    merged = K.merge_counts(parts)
    assert merged.dtype == np.int64 and np.array_equal(merged, whole) and np.array_equal(merged, R.merge_counts(parts))
    level_right = [np.array([3, 5, 1]), np.array([4, 0, 2])]
    assert K.merge_counts(level_right).tolist() == [7, 5, 3]
    assert K.classification_stats(merged) == K.classification_stats(whole)
    with pytest.raises(ValueError):
        K.merge_counts([])
    with pytest.raises(ValueError):
        K.merge_counts([whole, whole[:, :3]])
    with pytest.raises(ValueError):
        K.merge_counts([whole.astype(np.float64)])


def test_classification_stats_by_hand():
    K = _C()
    m = np.array([[3, 1, 0], [0, 0, 0], [2, 0, 4]], dtype=np.int64)        # class 1 has no image
    st = K.classification_stats(m)
    assert st["count"] == 10 and st["accuracy"] == 0.7
    assert abs(st["accuracy_stderr"] - math.sqrt(0.7 * 0.3 / 10)) <= 1e-15
    assert st["per_class_accuracy"] == [0.75, None, 4 / 6]
    one = K.classification_stats(np.array([[0, 1], [0, 0]]))
    assert one == {"accuracy": 0.0, "accuracy_stderr": None, "per_class_accuracy": [0.0, None], "count": 1}
    for bad in (np.zeros((2, 2), dtype=np.int64), np.ones((2, 3), dtype=np.int64), np.ones((2, 2)),
                np.array([[1, -1], [0, 1]])):
        with pytest.raises(ValueError):
            K.classification_stats(bad)


def test_class_weights_closed_forms():
    K = _C()
    assert K.class_weights([0.5], "edm", 0.5).tolist() == [8.0]                    # 2 / sigma_data^2 at sigma = sigma_data
    assert K.class_weights([0.25, 2.0], "eps", 0.5).tolist() == [16.0, 0.25]
    assert K.class_weights([0.25, 2.0, 80.0], "uniform", 0.5).tolist() == [1.0, 1.0, 1.0]
    w = K.class_weights([0.1, 3.0], "edm", 0.5)
    assert abs(w[0] - (1 / 0.25 + 1 / 0.01)) <= 1e-12 * w[0] and abs(w[1] - (4.0 + 1 / 9.0)) <= 1e-12 * w[1]
    for kw in (dict(weighting="snr"), dict(sigmas=[]), dict(sigmas=[0.0]), dict(sigmas=[math.nan]), dict(sigma_data=0.0),
               dict(sigmas="abc")):
        args = dict(sigmas=[1.0], weighting="edm", sigma_data=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            K.class_weights(**args)


def test_host_function_argument_errors():
    K = _C()
    se = _se()
    for fn in (lambda: K.class_scores(se[0], 12, [1, 1, 1]), lambda: K.class_scores(se, 0, [1, 1, 1]),
               lambda: K.class_scores(se, 12, [1, 1]), lambda: K.class_scores(se, 12, [1, math.nan, 1]),
               lambda: K.level_predictions(se[0]), lambda: K.predict(np.ones(4)), lambda: K.predict(np.ones((2, 0))),
               lambda: K.confusion_matrix([0, 1], [0], 2), lambda: K.confusion_matrix([0, 2], [0, 1], 2),
               lambda: K.confusion_matrix([0, 1], [0, -1], 2), lambda: K.confusion_matrix([0.5], [0], 2),
               lambda: K.confusion_matrix([0], [0], 0)):
        with pytest.raises(ValueError):
            fn()


# ------------------------------------------------------------------ constructor and command line
def test_constructor_errors():
    K = _C()
    ok = K.DiffusionClassifier()
    assert (ok.num_levels, ok.num_draws, ok.batch_size, ok.network_dtype, ok.weighting, ok.num_classes, ok.label_gain,
            ok.seed, ok.sigma_data) == (16, 1, 512, "bf16", "edm", None, False, 0, 0.5)
    assert K.DiffusionClassifier(sigmas=torch.tensor([0.5, 1.0]), num_classes=10, batch_size=10).sigmas == [0.5, 1.0]
    for kw in (dict(num_levels=0), dict(num_levels=65536), dict(num_levels=2.0), dict(num_levels=True),
               dict(sigmas=[]), dict(sigmas=[1.0, 1.0]), dict(sigmas=[2.0, 1.0]), dict(sigmas=[0.0, 1.0]),
               dict(sigmas=[1.0, math.inf]), dict(sigmas=[math.nan]), dict(sigmas=[1.0, 1.0 + 1e-12]),
               dict(P_std=0.0), dict(P_mean=math.nan), dict(seed=-1), dict(seed=1 << 64), dict(num_draws=0),
               dict(batch_size=0), dict(batch_size=65536), dict(network_dtype="fp16"), dict(sigma_data=0.0),
               dict(weighting="snr"), dict(num_classes=0), dict(num_classes=2.0), dict(num_classes=True),
               dict(label_gain=1), dict(num_classes=10, batch_size=9)):
        with pytest.raises(ValueError):
            K.DiffusionClassifier(**kw)
    with pytest.raises(ValueError, match="batch_size"):
        K.DiffusionClassifier(num_classes=10, batch_size=9)

    def model(x, s, c):
        return x
    # a plain callable needs num_classes; the training-distribution levels need a P_mean / P_std from somewhere
    with pytest.raises(ValueError, match="num_classes"):
        ok.classes_for(model)
    assert K.DiffusionClassifier(num_classes=7).classes_for(model) == 7
    with pytest.raises(ValueError, match="P_mean"):
        K.DiffusionClassifier(num_classes=7).levels.levels_for(model)

    class Emb:
        def __init__(self, k):
            self.num_classes = k

    class Net:
        def __init__(self, k):
            self.embedding = Emb(k)
    assert ok.classes_for(Net(10)) == 10
    with pytest.raises(ValueError, match="unconditional"):
        ok.classes_for(Net(None))
    with pytest.raises(ValueError, match="has 10 classes"):
        K.DiffusionClassifier(num_classes=7).classes_for(Net(10))
    with pytest.raises(ValueError, match="batch_size"):         # batch_size < C, known once the model is
        K.DiffusionClassifier(batch_size=9).classes_for(Net(10))
    # a CPU image never reaches the library
    with pytest.raises(ValueError, match="GPU"):
        K.DiffusionClassifier(sigmas=[1.0], num_classes=2).classify(model, torch.zeros(2, 3, 4, 4))
    from tinyedm_amd.callbacks import ClassifierAccuracy
    for kw in (dict(num_images=0), dict(every_n_epochs=0), dict(num_levels=0), dict(sigmas=[2.0, 1.0]),
               dict(weighting="snr"), dict(num_classes=10, batch_size=9)):
        with pytest.raises(ValueError):
            ClassifierAccuracy(**kw)
    cb = ClassifierAccuracy(num_images=8, num_levels=3)
    assert cb.images is None and cb.classifier.num_levels == 3


def test_ops_reject_cpu_operands_and_bad_class_counts_before_launch():
    from tinyedm_amd import _lib, ops
    x = torch.zeros(2, 3, 4, 4)
    calls = _lib.N_CALLS
    with pytest.raises(ValueError, match="no CPU path"):
        ops.eval_diffuse_classes(x, torch.zeros(2, dtype=torch.uint32), torch.zeros(2, dtype=torch.int32), torch.ones(1),
                                 torch.zeros(4, dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.eval_sqerr_classes(x.repeat_interleave(3, 0), x, 3)
    assert _lib.N_CALLS == calls


BASE = ["--ckpt_path", "/nonexistent/a.ckpt", "--report", "/nonexistent/out.json"]
DATA = ["--dataset", "cifar10", "--data_dir", "/nonexistent"]
CLI_ERRORS = [
    (BASE, "exactly one data source"),
    (BASE + DATA + ["--image_dir", "d", "--image_size", "8"], "exactly one data source"),
    (BASE + DATA + ["--sigmas", "0.5", "0.5", "2.0"], "strictly increasing"),
    (BASE + DATA + ["--sigmas", "2.0", "1.0"], "strictly increasing"),
    (BASE + DATA + ["--sigmas", "-1.0", "1.0"], "> 0"),
    (BASE + DATA + ["--num_levels", "0"], "num_levels"),
    (BASE + DATA + ["--labels_json", "l.json"], "--image_dir"),
    (BASE + ["--dataset", "mnist"], "--data_dir"),
    (BASE + ["--image_dir", "d"], "--image_size"),
    (BASE + ["--image_dir", "d", "--image_size", "8", "--mean", "0.5"], "--mean and --std"),
    (BASE + ["--image_dir", "d", "--image_size", "8", "--label_gain"], "--label_gain needs labels"),
    (BASE + DATA + ["--num_draws", "0"], "num_draws"),
    (BASE + DATA + ["--batch_size", "0"], "batch_size"),
    (BASE + DATA + ["--num_images", "0"], "--num_images"),
    (BASE + DATA + ["--seed", "-1"], "seed"),
    (["--ckpt_path", "/nonexistent/a.ckpt", "/nonexistent/a.ckpt", "--report", "r.json"] + DATA, "twice"),
]


@pytest.mark.parametrize("argv,needle", CLI_ERRORS, ids=[str(i) for i in range(len(CLI_ERRORS))])
def test_cli_argument_errors_before_anything_is_loaded(argv, needle, monkeypatch):
    """the checkpoint path does not exist and the GPU must not be touched: the refusal comes first"""
    K = _C()
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("the GPU was touched"))
    monkeypatch.setattr(torch, "load", lambda *a, **k: pytest.fail("a checkpoint was opened"))
    with pytest.raises(ValueError, match=needle):
        K.check_args(K.build_parser().parse_args(argv))
    with pytest.raises(SystemExit) as exc:
        K.main(argv)
    assert exc.value.code == 2


def test_cli_choices_are_argparse_errors(monkeypatch):
    K = _C()
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("the GPU was touched"))
    for extra in (["--weighting", "snr"], ["--network_dtype", "fp16"]):
        with pytest.raises(SystemExit) as exc:
            K.main(BASE + DATA + extra)
        assert exc.value.code == 2
    args = K.build_parser().parse_args(BASE + DATA)
    assert (args.num_images, args.num_levels, args.weighting, args.batch_size, args.network_dtype, args.label_gain) == (
        1000, 16, "edm", 512, "bf16", False)
    c = K.check_args(K.build_parser().parse_args(BASE + DATA + ["--weighting", "eps", "--label_gain", "--num_levels", "4"]))
    assert (c.weighting, c.label_gain, c.num_levels) == ("eps", True, 4)


def test_cli_module_alias_exits_with_status_2():
    r = subprocess.run([sys.executable, "-m", "tinyedm.classify", *BASE], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 2 and "exactly one data source" in r.stderr, r.stderr[-1500:]


def test_generate_labels_to_refuses_init_dir(monkeypatch):
    import tinyedm_amd.generate as G
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("the GPU was touched"))
    monkeypatch.setattr(torch, "load", lambda *a, **k: pytest.fail("a checkpoint was opened"))
    argv = ["--ckpt_path", "/nonexistent/a.ckpt", "--output_dir", "/nonexistent/out", "--num_samples", "4", "--image_size",
            "8", "--num_classes", "10", "--batch_size", "4", "--labels_to", "/nonexistent/l.json", "--init_dir", "d"]
    with pytest.raises(SystemExit) as exc:
        G.main(argv)
    assert exc.value.code == 2
    with pytest.raises(ValueError, match="--init_dir"):
        G.generate("/nonexistent/a.ckpt", False, "/nonexistent/out", 4, 8, 10, 4, init_dir="d",
                   labels_to="/nonexistent/l.json")
    G._check_labels_to(None, "d")
    G._check_labels_to("l.json", None)


def test_drawn_labels_are_the_datamodules():
    """--labels_to replays the labels on the host: they are the ones the sampling batches carry, rank by rank"""
    import tinyedm_amd.generate as G
    from tinyedm_amd.datamodules import RandomNoiseDataModule
    got = G._drawn_labels(4, 0, 8, 10, 10, 3, 5, 1)
    dm = RandomNoiseDataModule(4, 0, 8, 10, 10, in_channels=3, seed=5, device="cpu")
    want = [int(v) for b in dm.predict_dataloader() for v in b[1].flatten()]
    assert got == want and len(got) == 10 and all(0 <= v < 10 for v in got) and len(set(got)) > 1
    two = G._drawn_labels(4, 0, 8, 10, 10, 3, 5, 2)            # two ranks: 5 samples each, rank 1 under its own seed
    assert len(two) == 10 and two[:4] == got[:4]
    dm1 = RandomNoiseDataModule(4, 0, 8, 5, 10, in_channels=3, seed=5 + 1000003, device="cpu")
    assert two[5:] == [int(v) for b in dm1.predict_dataloader() for v in b[1].flatten()]


def test_abi_names_in_header_and_bindings():
    from tinyedm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    names = set(re.findall(r"\b(edm_[a-z0-9_]+)\s*\(", hdr))
    for name in ("edm_eval_diffuse_classes", "edm_eval_sqerr_classes"):
        assert name in names and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["edm_eval_diffuse_classes"]) == 13 and len(_lib.SIGNATURES["edm_eval_sqerr_classes"]) == 9
    # the pair they extend keeps its signature
    assert len(_lib.SIGNATURES["edm_eval_diffuse"]) == 12 and len(_lib.SIGNATURES["edm_eval_sqerr"]) == 8
