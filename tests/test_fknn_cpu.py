"""Feature-space neighbours, the parts that need no GPU: the fp64 restatement (tests/fknn_ref.py) against brute-force
Python, the float form of the host statistics and of metrics_from_counts (with the integer form unchanged), every refusal
of the feature form of the two command lines, and the dtype checks where a set is taken in."""
from fractions import Fraction

import numpy as np
import pytest

import fknn_ref as R
from tinyedm_amd import neighbors as N
from tinyedm_amd import prdc as P


# ------------------------------------------------------------------------------------------------ the restatement itself
def _brute(q, r, k, exclude_self):
    """exact rational arithmetic: dyadic inputs make every fp64 operation of the restatement exact, so it must agree"""
    out_d, out_i = [], []
    for i, a in enumerate(q.tolist()):
        keys = []
        for j, b in enumerate(r.tolist()):
            if exclude_self and i == j:
                continue
            keys.append((sum((Fraction(x) - Fraction(y)) ** 2 for x, y in zip(a, b)), j))
        keys.sort()
        out_d.append([float(d) for d, _ in keys[:k]])
        out_i.append([j for _, j in keys[:k]])
    return np.array(out_d), np.array(out_i)


@pytest.mark.parametrize("Q,Rn,D,k,excl", [(3, 7, 5, 1, False), (4, 9, 3, 4, False), (6, 6, 2, 5, True)])
def test_restatement_against_brute_force(Q, Rn, D, k, excl):
    r = R.dyadic(Q * 100 + Rn, Rn, D)
    r[1] = r[0]                                            # an exact duplicate: a tie at every query
    q = r if excl else R.dyadic(Q, Q, D)
    d, i = R.knn(q, r, k, exclude_self=excl)
    bd, bi = _brute(q, r, k, excl)
    assert d.dtype == np.float64 and np.array_equal(d, bd) and np.array_equal(i, bi)
    if excl:
        assert all(a not in i[a] for a in range(Q)) and i[0, 0] == 1 and i[1, 0] == 0 and d[0, 0] == 0.0
    # ball counts: the k-th neighbour radius holds exactly k references (ties aside) and the closed compare counts equality
    full = R.dist_matrix(q, r)
    rad = full.max(0)                                      # every query lies inside every ball, some exactly on the sphere
    assert R.ball_count(q, r, rad).tolist() == [Rn] * len(q)
    assert R.ball_count(q, r, np.zeros(Rn)).tolist() == (full == 0).sum(1).tolist()
    if excl:
        assert R.ball_count(q, r, rad, exclude_self=True).tolist() == [Rn - 1] * len(q)


def test_restatement_ratios():
    X = np.array([[0.0], [1.0], [10.0], [11.0]], np.float32)           # two clusters
    Y = np.array([[0.5], [0.25], [0.75]], np.float32)                  # samples of the first only
    m = R.prdc(X, Y, 1)
    assert m["precision"] == 1.0 and m["recall"] == 0.5 and m["coverage"] == 0.5
    assert m["density_sum"] == 6 and m["density"] == 2.0


# ------------------------------------------------------------------------------------------------ host arithmetic
def test_metrics_from_counts_float_form():
    hx, hy = [2, 0, 1], [1, 0]
    # 0.9 <= 0.5 is false in fp64; cast to integers it would be 0 <= 0, true
    m = P.metrics_from_counts(hx, hy, np.array([0.9, 0.25]), np.array([0.5, 0.25]), 1)
    assert m["coverage_count"] == 1 and m["coverage"] == 0.5
    assert m["precision_count"] == 2 and m["recall_count"] == 1 and m["density_sum"] == 3 and m["density"] == 1.0
    # values an fp32 or an integer compare would merge
    a = 1.0 + 2.0 ** -40
    assert P.metrics_from_counts(hx, hy, np.array([a, 1.0]), np.array([1.0, a]), 1)["coverage_count"] == 1
    for bad in ((np.array([0.5, np.nan]), np.array([0.5, 0.5])), (np.array([0.5, -0.5]), np.array([0.5, 0.5])),
                (np.array([0.5, 0.5]), np.array([1, 1])), (np.array([0.5, 0.5]), np.array([0.5, np.inf]))):
        with pytest.raises(ValueError):
            P.metrics_from_counts(hx, hy, *bad, 1)


def test_metrics_from_counts_integer_form_unchanged():
    want = {"k": 2, "num_real": 3, "num_fake": 2, "precision": 0.5, "recall": 2 / 3, "density": 0.75, "coverage": 2 / 3,
            "precision_count": 1, "recall_count": 2, "density_sum": 3, "coverage_count": 2}
    args = ([3, 0], [1, 0, 4], [5, 7, 2 ** 40], [5, 6, 2 ** 40])
    assert P.metrics_from_counts(*args, 2) == want
    assert P.metrics_from_counts(*(np.asarray(a, np.int64) for a in args), 2) == want
    assert P.metrics_from_counts(args[0], args[1], np.asarray(args[2], np.uint64), np.asarray(args[3], np.uint64), 2) == want


def test_statistics_take_float_distances():
    s = np.array([0.25, 2.5, 1.0 + 2.0 ** -40])
    h = np.array([1.0, 2.5, 0.125, 3.0])
    # pairs with holdout strictly farther: 0.25 -> 3, 2.5 -> 1 (+ one tie), 1 + 2^-40 -> 2
    assert N.closer_than_holdout(s, h) == (2 * 6 + 1) / (2 * 3 * 4)
    assert N.closer_than_holdout([1, 5], [1, 2, 9]) == (2 * 3 + 1) / (2 * 2 * 3)          # the integer form as before
    with pytest.raises(ValueError):
        N.closer_than_holdout(s, [1, 2])
    dist = np.array([[0.0, 0.5], [0.25, 0.75]])
    idx = np.array([[3, 1], [0, 2]])
    assert N.duplicates(dist, idx, 0.25) == [(0, 3, 0.0), (1, 0, 0.25)]
    assert N.duplicates(dist, idx, 0) == [(0, 3, 0.0)]
    got = N.duplicates(np.array([[0, 5]]), np.array([[1, 2]]), 0)
    assert got == [(0, 1, 0)] and isinstance(got[0][2], int)
    assert N.summarize(dist[:, 0])["min"] == 0.0 and N.summarize(dist[:, 0])["p50"] == 0.125
    rows = N.neighbour_rows(dist, idx, 4)
    assert rows[1][0] == {"index": 0, "d2": 0.25, "rms": 0.25} and isinstance(rows[0][0]["d2"], float)
    assert N.neighbour_rows(np.array([[65025 * 4]]), np.array([[7]]), 4) == [[{"index": 7, "d2": 260100, "rms": 1.0}]]
    assert N.rms(9.0, 4, 1.0) == 1.5


# ------------------------------------------------------------------------------------------------ command lines
@pytest.fixture()
def npy(tmp_path):
    rng = np.random.default_rng(0)
    files = {"a": rng.standard_normal((12, 6)).astype(np.float32), "b": rng.standard_normal((20, 6)).astype(np.float32),
             "d7": rng.standard_normal((20, 7)).astype(np.float32), "f64": rng.standard_normal((20, 6)),
             "flat": rng.standard_normal(20).astype(np.float32), "tiny": rng.standard_normal((3, 6)).astype(np.float32)}
    files["nan"] = files["b"].copy()
    files["nan"][3, 2] = np.nan
    files["inf"] = files["a"].copy()
    files["inf"][0, 0] = np.inf
    out = {}
    for name, a in files.items():
        out[name] = str(tmp_path / f"{name}.npy")
        np.save(out[name], a)
    return out


def _nn_args(*argv):
    return N.build_parser().parse_args(["--report", "r.json", *argv])


def _prdc_args(*argv):
    return P.build_parser().parse_args(["--report", "r.json", *argv])


def test_neighbors_check_args_feature_form(npy):
    a = _nn_args("--features", npy["a"], "--ref_features", npy["b"], "--holdout_features", npy["a"], "--k", "5", "--max_d2", "0.5")
    N.check_args(a)
    assert a.max_d2 == 0.5 and sorted(a.feature_sets) == ["features", "holdout_features", "ref_features"]
    assert a.feature_sets["ref_features"].dtype == np.float32 and a.feature_sets["ref_features"].shape == (20, 6)
    N.check_args(_nn_args("--features", npy["a"], "--self"))
    N.check_args(_nn_args("--ref_features", npy["b"], "--self", "--max_d2", "3"))
    refusals = [
        (["--features", npy["a"], "--ref_features", npy["b"], "--image_dir", "x"], "--image_dir"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--dataset", "mnist", "--data_dir", "x"], "--dataset"),
        (["--features", npy["a"], "--ref_image_dir", "x"], "--ref_image_dir"),
        (["--image_dir", "x", "--ref_image_dir", "y", "--holdout_features", npy["a"]], "--holdout_features"),
        (["--features", npy["a"]], "--ref_features"),
        (["--ref_features", npy["b"]], "--features"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--self"], "--self"),
        (["--features", npy["a"], "--self", "--holdout_features", npy["b"]], "--holdout_features"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--grid", "g.png"], "--grid"),
        (["--features", npy["a"], "--ref_features", npy["f64"]], "--ref_features"),
        (["--features", npy["flat"], "--ref_features", npy["b"]], "--features"),
        (["--features", npy["a"], "--ref_features", npy["d7"]], "differ in D"),
        (["--features", npy["a"], "--ref_features", npy["nan"]], "non-finite"),
        (["--features", npy["inf"], "--ref_features", npy["b"]], "non-finite"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--max_d2", "-0.5"], "--max_d2"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--max_d2", "nan"], "--max_d2"),
        (["--features", npy["a"], "--ref_features", npy["tiny"], "--k", "4"], "--k"),
        (["--features", npy["tiny"], "--self", "--k", "3"], "--k"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--k", "33"], "--k"),
    ]
    for argv, word in refusals:
        with pytest.raises(ValueError, match=word):
            N.check_args(_nn_args(*argv))
    # the pixel form keeps integer distances
    with pytest.raises(ValueError, match="--max_d2"):
        N.check_args(_nn_args("--image_dir", "x", "--ref_image_dir", "y", "--max_d2", "0.5"))
    N.check_args(_nn_args("--image_dir", "x", "--ref_image_dir", "y", "--max_d2", "5"))


def test_prdc_check_args_feature_form(npy, tmp_path):
    a = _prdc_args("--features", npy["a"], "--ref_features", npy["b"], "--holdout_features", npy["a"], "--k", "3", "5")
    P.check_args(a)
    assert sorted(a.feature_sets) == ["features", "holdout_features", "ref_features"]
    P.check_args(_prdc_args("--features", npy["a"], "--ref_features", npy["b"], "--labels_json", "l.json", "--ref_labels", "r.json"))
    refusals = [
        (["--features", npy["a"], "--ref_features", npy["b"], "--image_dir", "x"], "--image_dir"),
        (["--features", npy["a"], "--dataset", "cifar10", "--data_dir", "x"], "--dataset"),
        (["--image_dir", "x", "--ref_features", npy["b"]], "--ref_features"),
        (["--image_dir", "x", "--ref_image_dir", "y", "--holdout_features", npy["a"]], "--holdout_features"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--holdout"], "--holdout"),
        (["--features", npy["a"]], "--ref_features"),
        (["--ref_features", npy["b"]], "--features"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--labels_json", "l.json"], "--ref_labels"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--ref_labels", "l.json"], "--labels_json"),
        (["--image_dir", "x", "--ref_image_dir", "y", "--ref_labels", "l.json"], "--ref_labels"),
        (["--features", npy["a"], "--ref_features", npy["f64"]], "--ref_features"),
        (["--features", npy["flat"], "--ref_features", npy["b"]], "--features"),
        (["--features", npy["a"], "--ref_features", npy["d7"]], "differ in D"),
        (["--features", npy["nan"], "--ref_features", npy["b"]], "non-finite"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--holdout_features", npy["inf"]], "non-finite"),
        (["--features", npy["tiny"], "--ref_features", npy["b"], "--k", "3"], "k = 3"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--k", "12"], "k = 12"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--num_real", "21"], "--num_real"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--k", "5", "--num_real", "5"], "k = 5"),
        (["--features", npy["a"], "--ref_features", npy["b"], "--ref_chunk", "0"], "--ref_chunk"),
    ]
    for argv, word in refusals:
        with pytest.raises(ValueError, match=word):
            P.check_args(_prdc_args(*argv))


def test_main_ends_in_the_parser_error(npy, capsys):
    """a refusal reaches the user as a usage error that names the flags, before the device is touched"""
    for mod, argv in ((N, ["--features", npy["a"], "--ref_features", npy["nan"]]),
                      (P, ["--features", npy["a"], "--ref_features", npy["nan"]]),
                      (N, ["--features", npy["a"], "--ref_features", npy["b"], "--grid", "g.png"])):
        with pytest.raises(SystemExit) as e:
            mod.main(["--report", "r.json", *argv])
        err = capsys.readouterr().err
        assert e.value.code == 2 and ("--ref_features" in err or "--grid" in err)


# ------------------------------------------------------------------------------------------------ dtype dispatch
def test_sets_are_checked_where_they_are_taken_in():
    f = np.zeros((8, 4), np.float32)
    bad = [f.astype(np.float64), f.astype(np.float16), f.astype(np.int32), f.reshape(8, 2, 2), f[:, 0]]
    nan = f.copy()
    nan[2, 1] = np.nan
    inf = f.copy()
    inf[0, 0] = -np.inf
    for x in bad + [nan, inf]:
        with pytest.raises(ValueError):
            N.NearestNeighbors(x, k=1, device="cuda")
        with pytest.raises(ValueError):
            P.ManifoldMetrics(x, k=1, device="cuda")
    with pytest.raises(ValueError, match="float"):
        N.as_set(f.astype(np.float64), "t")
    assert N.as_set(f, "t").dtype.is_floating_point and N.as_set(np.zeros((3, 2, 2), np.uint8), "t").dim() == 3
