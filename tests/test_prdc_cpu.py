"""Precision, recall, density and coverage on the host: the int64 restatement (tests/prdc_ref.py) against the hand-checked
example of the definitions, and the pure host functions of tinyedm_amd/prdc.py (check_k, radii_from_knn,
metrics_from_counts, per_class, check_args, the report schema) against the restatement.  No GPU."""
import argparse

import numpy as np
import pytest

import prdc_ref as R
from tinyedm_amd import prdc as P

RATIOS = ("precision", "recall", "density", "coverage")
NUMERATORS = ("precision_count", "recall_count", "density_sum", "coverage_count")


def _ref_score(X, Y, ks):
    return {k: R.prdc(X, Y, k) for k in ks}


# ------------------------------------------------------------------------------------------------ the worked example
X1 = np.array([[0], [10], [20], [100]], dtype=np.uint8)
Y1 = np.array([[5], [40], [200], [201]], dtype=np.uint8)


def test_worked_example():
    hx, hy, near, rX, rY = R.counts(X1, Y1, 1)
    assert rX.tolist() == [100, 100, 100, 6400] and rY.tolist() == [1225, 1225, 1, 1]
    assert hx.tolist() == [2, 1, 0, 0]
    want = {"precision": 0.5, "density": 0.75, "recall": 0.75, "coverage": 0.75}
    ref = R.prdc(X1, Y1, 1)
    got = P.metrics_from_counts(hx, hy, near, rX, 1)
    for name, v in want.items():
        assert ref[name] == v and got[name] == v, name
    assert got == ref
    assert (got["precision_count"], got["density_sum"], got["recall_count"], got["coverage_count"]) == (2, 3, 3, 3)
    assert (got["num_real"], got["num_fake"], got["k"]) == (4, 4, 1)


def test_identical_sets():
    rng = np.random.default_rng(1)
    X = rng.integers(0, 256, (40, 12), dtype=np.uint8)
    for k in (1, 3):
        hx, hy, near, rX, _ = R.counts(X, X, k)
        m = P.metrics_from_counts(hx, hy, near, rX, k)
        assert m["precision"] == m["recall"] == m["coverage"] == 1.0 and m == R.prdc(X, X, k)
        assert (near == 0).all() and m["density"] >= 1.0        # each point lies in its own ball and in its neighbours'


def test_duplicates_give_radius_zero_and_a_closed_ball():
    X = np.array([[7, 7], [7, 7], [200, 0], [0, 200]], dtype=np.uint8)      # rows 0 and 1 are copies
    Y = np.array([[7, 7], [90, 90], [91, 90]], dtype=np.uint8)
    rX = R.radii(X, 1)
    assert rX[0] == 0 and rX[1] == 0 and rX[2] > 0
    hx = R.ball_count(Y, X, rX)
    assert hx[0] >= 2                                      # d2 = 0 <= radius 0: the closed ball still holds the copy
    assert R.ball_count(Y, X, np.maximum(rX - 1, 0))[0] >= 2 and R.ball_count(Y[:1], X[:2], [0, 0])[0] == 2
    m = P.metrics_from_counts(*R.counts(X, Y, 1)[:4], 1)
    assert m == R.prdc(X, Y, 1) and m["precision_count"] >= 1


# ------------------------------------------------------------------------------------------------ radii for several k
def test_radii_from_knn_equals_separate_computations():
    rng = np.random.default_rng(2)
    X = rng.integers(0, 256, (30, 9), dtype=np.uint8)
    d = R.dist_matrix(X, X)
    dist = np.stack([np.sort(np.delete(d[i], i))[:7] for i in range(30)])     # a self-search at k = 7
    got = P.radii_from_knn(dist, (7, 1, 3))
    assert sorted(got) == [1, 3, 7]
    for k in (1, 3, 7):
        assert np.array_equal(got[k], R.radii(X, k))
    assert np.array_equal(P.radii_from_knn(dist, 5)[5], R.radii(X, 5))
    with pytest.raises(ValueError):
        P.radii_from_knn(dist, 8)                           # beyond the search
    with pytest.raises(ValueError):
        P.radii_from_knn(dist[:, 0], 1)


# ------------------------------------------------------------------------------------------------ per class
def test_per_class_equals_scoring_the_subsets():
    rng = np.random.default_rng(3)
    X = rng.integers(0, 256, (50, 6), dtype=np.uint8)
    Y = rng.integers(0, 256, (33, 6), dtype=np.uint8)
    lx = np.arange(50) % 3
    ly = np.arange(33) % 3
    ly = np.where(np.arange(33) < 30, ly, 4)                # class 4: samples only, 3 of them
    lx = np.where(np.arange(50) < 48, lx, 5)                # class 5: reals only
    got = P.per_class(_ref_score, X, Y, lx, ly, (2, 4))
    assert sorted(got) == [2, 4]
    for k in (2, 4):
        want = R.prdc_per_class(X, Y, lx, ly, k)
        assert sorted(got[k]) == sorted(want) == [0, 1, 2, 4, 5]
        for c, w in want.items():
            if w is None:
                assert c in (4, 5) and "skipped" in got[k][c] and not any(r in got[k][c] for r in RATIOS)
                assert (got[k][c]["num_real"], got[k][c]["num_fake"]) == (int((lx == c).sum()), int((ly == c).sum()))
            else:
                assert got[k][c] == w
    # a class large enough for k = 2 but not for k = 4 is scored at one and skipped at the other
    ly2 = np.where(np.arange(33) < 4, 7, 0)
    lx2 = np.where(np.arange(50) < 10, 7, 0)
    got = P.per_class(_ref_score, X, Y, lx2, ly2, (2, 4))
    assert got[2][7] == R.prdc(X[lx2 == 7], Y[ly2 == 7], 2) and "skipped" in got[4][7]
    with pytest.raises(ValueError):
        P.per_class(_ref_score, X, Y, lx[:-1], ly, (2,))
    with pytest.raises(ValueError):
        P.per_class(_ref_score, X, Y, lx.astype(np.float32), ly, (2,))


# ------------------------------------------------------------------------------------------------ refusals
def test_check_k():
    assert P.check_k(5) == (5,) and P.check_k([10, 3, 5, 3]) == (3, 5, 10) and P.check_k((1, 32)) == (1, 32)
    assert P.check_k(3, 4, 4) == (3,) and P.check_k((1, 9), 10, 50) == (1, 9) and P.check_k(np.int64(2)) == (2,)
    for bad in (0, 33, -1, True, 2.0, "3", None, [], [1, 0], [1, 2.5]):
        with pytest.raises(ValueError):
            P.check_k(bad)
    for k, M, N in ((4, 4, 100), (4, 100, 4), ((1, 10), 50, 10), (1, 1, 5)):
        with pytest.raises(ValueError):
            P.check_k(k, M, N)


def test_metrics_from_counts_refusals():
    ok = ([1, 0], [1, 1, 0], [4, 5, 6], [4, 4, 4])
    P.metrics_from_counts(*ok, 1)
    with pytest.raises(ValueError):
        P.metrics_from_counts(*ok, 0)
    with pytest.raises(ValueError):
        P.metrics_from_counts(ok[0], ok[1], ok[2][:2], ok[3], 1)
    with pytest.raises(ValueError):
        P.metrics_from_counts([], ok[1], ok[2], ok[3], 1)
    with pytest.raises(ValueError):
        P.metrics_from_counts([-1, 0], ok[1], ok[2], ok[3], 1)


def _args(*argv):
    return P.build_parser().parse_args(list(argv))


DATA = ("--dataset", "cifar10", "--data_dir", "d")
BASE = ("--image_dir", "s", "--report", "r.json")


def test_check_args_accepts():
    P.check_args(_args(*BASE, *DATA))
    P.check_args(_args(*BASE, *DATA, "--k", "3", "5", "10", "--holdout", "--labels_json", "l.json", "--per_sample",
                       "--num_real", "1000", "--ref_chunk", "4096"))
    P.check_args(_args(*BASE, "--ref_image_dir", "x", "--holdout_image_dir", "h", "--k", "1"))
    assert _args(*BASE, *DATA).k == [5]


@pytest.mark.parametrize("argv", [
    ("--report", "r.json") + DATA,                                        # no samples
    BASE,                                                                 # no reals
    BASE + DATA + ("--ref_image_dir", "x"),                               # two sources of reals
    BASE + ("--dataset", "cifar10"),                                      # no --data_dir
    BASE + ("--ref_image_dir", "x", "--data_dir", "d"),
    BASE + DATA + ("--k", "0"),
    BASE + DATA + ("--k", "3", "33"),
    BASE + DATA + ("--num_real", "1"),
    BASE + DATA + ("--num_real", "5", "--k", "5"),                        # the fifth neighbour of 5 images
    BASE + ("--ref_image_dir", "x", "--holdout"),                         # no test split
    BASE + DATA + ("--holdout", "--holdout_image_dir", "h"),
    BASE + ("--ref_image_dir", "x", "--labels_json", "l.json"),           # no labelled reals
    BASE + DATA + ("--ref_chunk", "0"),
], ids=lambda a: " ".join(a[-3:]))
def test_check_args_refuses(argv):
    with pytest.raises(ValueError):
        P.check_args(_args(*argv))


def test_check_args_refuses_values_argparse_cannot_produce():
    a = _args(*BASE, *DATA)
    for field, bad in (("k", [True]), ("k", []), ("num_real", True), ("ref_chunk", 2.5)):
        b = argparse.Namespace(**{**vars(a), field: bad})
        with pytest.raises(ValueError):
            P.check_args(b)


def test_check_sets_and_main_refuse_before_the_device(tmp_path, monkeypatch):
    real = np.zeros((6, 3, 4, 4), np.uint8)
    P.check_sets((1, 5), real, {"samples": np.zeros((6, 3, 4, 4), np.uint8)})
    with pytest.raises(ValueError, match="samples"):
        P.check_sets((1, 5), real, {"samples": np.zeros((5, 3, 4, 4), np.uint8)})         # too few samples for k = 5
    with pytest.raises(ValueError, match="holdout"):
        P.check_sets((1,), real, {"samples": real, "holdout": np.zeros((6, 1, 4, 4), np.uint8)})
    # main: too few images, read from PNG directories, ends in the parser's error and never imports the device path
    from PIL import Image
    for name, n in (("real", 4), ("fake", 3)):
        (tmp_path / name).mkdir()
        for i in range(n):
            Image.fromarray(np.full((4, 4, 3), 10 * i, np.uint8)).save(tmp_path / name / f"{i}.png")

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(P, "ManifoldMetrics", no_device)
    with pytest.raises(SystemExit) as e:
        P.main(["--image_dir", str(tmp_path / "fake"), "--ref_image_dir", str(tmp_path / "real"), "--k", "3", "--report",
                str(tmp_path / "r.json")])
    assert e.value.code == 2 and not (tmp_path / "r.json").exists()
    with pytest.raises(SystemExit):
        P.main(["--image_dir", str(tmp_path / "fake"), "--ref_image_dir", str(tmp_path / "real"), "--k", "40", "--report",
                str(tmp_path / "r.json")])


# ------------------------------------------------------------------------------------------------ the report
def test_report_schema_and_table():
    m = P.metrics_from_counts(*R.counts(X1, Y1, 1)[:4], 1)
    assert set(m) == {"k", "num_real", "num_fake", *RATIOS, *NUMERATORS}
    assert all(isinstance(m[n], int) for n in NUMERATORS + ("k", "num_real", "num_fake"))
    assert all(isinstance(m[r], float) for r in RATIOS)
    assert m["precision"] == m["precision_count"] / m["num_fake"] and m["recall"] == m["recall_count"] / m["num_real"]
    assert m["density"] == m["density_sum"] / (m["k"] * m["num_fake"]) and m["coverage"] == m["coverage_count"] / m["num_real"]
    scores = {1: {**m, "per_class": {0: m, 3: {"skipped": "why", "num_real": 1, "num_fake": 0}}}}
    js = P._json_keys(scores)
    assert list(js) == ["1"] and list(js["1"]["per_class"]) == ["0", "3"]
    import json
    assert json.loads(json.dumps(js)) == js
    text = P.format_table({"samples": js, "holdout": P._json_keys({1: m})})
    lines = text.splitlines()
    assert lines[0].split() == ["set", "k", *RATIOS]
    assert lines[1].split() == ["samples", "1", "0.5000", "0.7500", "0.7500", "0.7500"]
    assert lines[2].split()[0] == "holdout" and "skipped: why" in lines[4] and lines[3].split()[:2] == ["class", "0"]


class _HostMetrics:
    """ManifoldMetrics with the restatement in place of the device: what main() hands over and what it writes"""
    calls = []

    def __init__(self, real, k=5, ref_chunk=None, device=None):
        self.real, self.ks, self.ref_chunk = real.reshape(len(real), -1), P.check_k(k, len(real)), ref_chunk

    def score(self, fake, real_labels=None, fake_labels=None, per_sample=False):
        fake = fake.reshape(len(fake), -1)
        _HostMetrics.calls.append((len(self.real), len(fake), real_labels is not None, per_sample, self.ref_chunk))
        out = _ref_score(self.real, fake, self.ks)
        if real_labels is not None:
            classes = P.per_class(_ref_score, self.real, fake, real_labels, fake_labels, self.ks)
            for k in self.ks:
                out[k]["per_class"] = classes[k]
        return out


def _write_mnist(root, stem, x, y):
    import struct
    raw = root / "MNIST" / "raw"
    raw.mkdir(parents=True, exist_ok=True)
    (raw / f"{stem}-images-idx3-ubyte").write_bytes(struct.pack(">IIII", 2051, *x.shape) + x.tobytes())
    (raw / f"{stem}-labels-idx1-ubyte").write_bytes(struct.pack(">II", 2049, len(y)) + y.astype(np.uint8).tobytes())


def test_main_report_with_dataset_labels_and_holdout(tmp_path, monkeypatch, capsys):
    import json
    import torch
    from PIL import Image
    rng = np.random.default_rng(5)
    train, test = rng.integers(0, 256, (14, 4, 4), dtype=np.uint8), rng.integers(0, 256, (9, 4, 4), dtype=np.uint8)
    ytrain, ytest = np.arange(14) % 2, np.arange(9) % 2
    _write_mnist(tmp_path, "train", train, ytrain)
    _write_mnist(tmp_path, "t10k", test, ytest)
    samples = rng.integers(0, 256, (8, 4, 4), dtype=np.uint8)
    (tmp_path / "s").mkdir()
    for i, a in enumerate(samples):
        Image.fromarray(a).save(tmp_path / "s" / f"{i}.png")
    drawn = [0, 0, 0, 0, 1, 1, 1, 0, 1, 1]                  # longer than the directory: the first 8 count
    (tmp_path / "drawn.json").write_text(json.dumps(drawn))
    monkeypatch.setattr(P, "ManifoldMetrics", _HostMetrics)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    _HostMetrics.calls.clear()
    argv = ["--image_dir", str(tmp_path / "s"), "--dataset", "mnist", "--data_dir", str(tmp_path), "--k", "2", "1", "--num_real",
            "12", "--holdout", "--labels_json", str(tmp_path / "drawn.json"), "--ref_chunk", "5", "--report",
            str(tmp_path / "r.json")]
    rep = P.main(argv)
    with open(tmp_path / "r.json") as f:
        assert json.load(f) == rep
    assert _HostMetrics.calls == [(12, 8, True, False, 5), (12, 9, False, False, 5)]
    X, Y = train[:12].reshape(12, -1), samples.reshape(8, -1)
    assert set(rep) == {"k", "num_real", "image_shape", "space", "num_samples", "samples", "num_holdout", "holdout"}
    assert (rep["k"], rep["num_real"], rep["num_samples"], rep["num_holdout"], rep["image_shape"]) == ([1, 2], 12, 8, 9, [1, 4, 4])
    for k in (1, 2):
        got = dict(rep["samples"][str(k)])
        classes = got.pop("per_class")
        assert got == R.prdc(X, Y, k) and rep["holdout"][str(k)] == R.prdc(X, test.reshape(9, -1), k)
        assert classes == {str(c): m for c, m in R.prdc_per_class(X, Y, ytrain[:12], np.array(drawn[:8]), k).items()}
    out = capsys.readouterr().out
    assert "holdout" in out and "class 1" in out and "wrote" in out
    for bad in ([0, 1], [0] * 7 + [-1], [0] * 7 + [True], {"a": 1}):
        (tmp_path / "drawn.json").write_text(json.dumps(bad))
        with pytest.raises(SystemExit):
            P.main(argv)


def test_shim_and_export():
    import tinyedm
    import tinyedm.prdc as S
    import tinyedm_amd
    assert S.main is P.main and S.ManifoldMetrics is P.ManifoldMetrics is tinyedm_amd.ManifoldMetrics is tinyedm.ManifoldMetrics
    assert S.check_k is P.check_k and S.metrics_from_counts is P.metrics_from_counts


def test_entry_is_declared_and_bound():
    import os
    import re
    from tinyedm_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tinyedm_hip.h")) as f:
        hdr = f.read()
    params = re.search(r"int edm_u8_ball_count_partial\((.*?)\);", hdr, re.S).group(1)
    assert len(params.split(",")) == len(_lib.SIGNATURES["edm_u8_ball_count_partial"]) == 13
