"""Nearest-neighbour search, the parts that need no GPU: the numpy reference against brute-force Python, the host statistics
of tinyedm_amd/neighbors.py, every command-line refusal, the PNG reader and the header's declarations."""
import os
import re

import numpy as np
import pytest

import neighbors_ref as R
from tinyedm_amd import neighbors as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference itself
def _brute(q, r, k, exclude_self):
    out_d, out_i = [], []
    for i, a in enumerate(q.tolist()):
        keys = []
        for j, b in enumerate(r.tolist()):
            if exclude_self and i == j:
                continue
            keys.append((sum((x - y) ** 2 for x, y in zip(a, b)), j))
        keys.sort()
        out_d.append([d for d, _ in keys[:k]])
        out_i.append([j for _, j in keys[:k]])
    return np.array(out_d), np.array(out_i)


@pytest.mark.parametrize("Q,Rn,D,k", [(3, 7, 5, 1), (4, 9, 3, 4), (5, 5, 2, 5)])
def test_reference_against_brute_force(Q, Rn, D, k):
    rng = np.random.default_rng(Q * 100 + Rn)
    q = rng.integers(0, 256, (Q, D), dtype=np.uint8)
    r = rng.integers(0, 4, (Rn, D), dtype=np.uint8) * 85          # few levels: ties in distance
    r[1] = r[0]
    d, i = R.knn(q, r, k)
    bd, bi = _brute(q, r, k, False)
    assert np.array_equal(d, bd) and np.array_equal(i, bi)


def test_reference_exclude_self_and_extremes():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 3, (6, 4), dtype=np.uint8) * 100
    x[4] = x[2]
    d, i = R.knn(x, x, 3, exclude_self=True)
    bd, bi = _brute(x, x, 3, True)
    assert np.array_equal(d, bd) and np.array_equal(i, bi)
    assert all(a not in i[a] for a in range(6)) and i[2, 0] == 4 and i[4, 0] == 2 and d[2, 0] == 0
    z = np.zeros((1, 8), np.uint8)
    f = np.full((1, 8), 255, np.uint8)
    assert R.dist_matrix(z, f)[0, 0] == 65025 * 8


# ------------------------------------------------------------------------------------------------ host statistics
def test_rms():
    assert N.rms(0, 10) == 0.0
    assert N.rms(65025 * 12, 12) == pytest.approx(1.0, abs=1e-15)
    d2 = np.array([[3, 48], [75, 0]])
    assert np.array_equal(N.rms(d2, 3), R.rms(d2, 3))
    with pytest.raises(ValueError):
        N.rms(1, 0)


def test_summarize():
    rng = np.random.default_rng(0)
    for n in (1, 2, 7, 100):
        a = rng.integers(0, 10 ** 6, n)
        got, want = N.summarize(a), R.summarize(a)
        assert set(got) == {"n", "min", "p1", "p5", "p25", "p50", "p75", "p95", "mean"}
        for key in want:
            assert got[key] == pytest.approx(want[key], rel=1e-12), key
    s = N.summarize([4, 0, 2, 1, 3])
    assert (s["min"], s["p50"], s["mean"], s["p25"], s["p75"]) == (0.0, 2.0, 2.0, 1.0, 3.0)
    with pytest.raises(ValueError):
        N.summarize([])


def test_closer_than_holdout_hand_cases():
    assert N.closer_than_holdout([1, 2, 3], [10, 11]) == 1.0          # every sample closer
    assert N.closer_than_holdout([10, 11], [1, 2, 3]) == 0.0
    assert N.closer_than_holdout([5, 7, 9], [5, 7, 9]) == 0.5          # identical lists
    assert N.closer_than_holdout([4, 4], [4]) == 0.5                    # all ties
    # (1 vs 1: tie, 1 vs 2: closer, 3 vs 1: no, 3 vs 2: no) -> (0.5 + 1) / 4
    assert N.closer_than_holdout([1, 3], [1, 2]) == 0.375
    rng = np.random.default_rng(1)
    s, h = rng.integers(0, 20, 31), rng.integers(0, 20, 17)
    assert N.closer_than_holdout(s, h) == R.closer_than_holdout(s, h)
    with pytest.raises(ValueError):
        N.closer_than_holdout([], [1])


def test_duplicates():
    dist = np.array([[0, 5, 9], [2, 2, 30], [7, 8, 9]])
    idx = np.array([[4, 1, 2], [0, 3, 5], [6, 7, 8]])
    assert N.duplicates(dist, idx, 2) == [(0, 4, 0), (1, 0, 2), (1, 3, 2)] == R.duplicates(dist, idx, 2)
    assert N.duplicates(dist, idx, 0) == [(0, 4, 0)]
    assert N.duplicates(dist + 1, idx, 0) == []
    with pytest.raises(ValueError):
        N.duplicates(dist, idx[:, :2], 1)
    with pytest.raises(ValueError):
        N.duplicates(dist, idx, -1)


# ------------------------------------------------------------------------------------------------ command line refusals
def _args(*argv):
    return N.build_parser().parse_args(["--report", "r.json", *argv])


def test_cli_accepts():
    N.check_args(_args("--image_dir", "s", "--dataset", "cifar10", "--data_dir", "d", "--holdout", "--k", "32"))
    N.check_args(_args("--image_dir", "s", "--ref_image_dir", "r", "--holdout_image_dir", "h", "--max_d2", "0"))
    N.check_args(_args("--self", "--ref_image_dir", "r", "--max_d2", "10"))
    N.check_args(_args("--self", "--dataset", "mnist", "--data_dir", "d"))


@pytest.mark.parametrize("argv", [
    ("--image_dir", "s"),                                                              # no reference source
    ("--image_dir", "s", "--dataset", "cifar10", "--data_dir", "d", "--ref_image_dir", "r"),   # two of them
    ("--image_dir", "s", "--dataset", "cifar10"),                                      # --dataset without --data_dir
    ("--image_dir", "s", "--ref_image_dir", "r", "--data_dir", "d"),                   # --data_dir without --dataset
    ("--self", "--image_dir", "s", "--ref_image_dir", "r"),                            # --self with --image_dir
    ("--ref_image_dir", "r"),                                                          # neither samples nor --self
    ("--image_dir", "s", "--ref_image_dir", "r", "--k", "0"),
    ("--image_dir", "s", "--ref_image_dir", "r", "--k", "33"),
    ("--image_dir", "s", "--ref_image_dir", "r", "--max_d2", "-1"),
    ("--image_dir", "s", "--ref_image_dir", "r", "--holdout"),                         # no test split of a PNG directory
    ("--image_dir", "s", "--dataset", "mnist", "--data_dir", "d", "--holdout", "--holdout_image_dir", "h"),
    ("--self", "--ref_image_dir", "r", "--holdout_image_dir", "h"),
    ("--self", "--ref_image_dir", "r", "--grid", "g.png"),
    ("--image_dir", "s", "--ref_image_dir", "r", "--grid", "g.png", "--grid_rows", "0"),
])
def test_cli_refusals(argv):
    with pytest.raises(ValueError):
        N.check_args(_args(*argv))


def test_cli_refusal_exits_before_anything_is_loaded(capsys):
    with pytest.raises(SystemExit) as e:
        N.main(["--report", "r.json", "--image_dir", "/nonexistent", "--ref_image_dir", "/nonexistent", "--k", "40"])
    assert e.value.code == 2 and "--k" in capsys.readouterr().err


def test_alias_module():
    import tinyedm.neighbors as A
    assert A.main is N.main and A.NearestNeighbors is N.NearestNeighbors


# ------------------------------------------------------------------------------------------------ the PNG reader
def test_load_images_u8_round_trip(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(5)
    for C in (3, 1):
        d = tmp_path / f"c{C}"
        d.mkdir()
        x = rng.integers(0, 256, (12, C, 6, 6), dtype=np.uint8)
        for i in (10, 2, 0, 1, 11, 3, 9, 4, 8, 5, 7, 6):                # written out of order; 10 sorts after 9
            a = x[i].transpose(1, 2, 0)
            Image.fromarray(a[:, :, 0] if C == 1 else a).save(d / f"{i}.png")
        got = N.load_images_u8(str(d), 6, C)
        assert got.dtype == np.uint8 and got.shape == (12, C, 6, 6) and np.array_equal(got, x)
        assert np.array_equal(N.load_images_u8(str(d)), x)               # size and channels from the first image
        with pytest.raises(ValueError):
            N.load_images_u8(str(d), 8, C)
    wide = tmp_path / "wide"                                             # H != W
    wide.mkdir()
    y = rng.integers(0, 256, (3, 3, 4, 7), dtype=np.uint8)
    for i in range(3):
        Image.fromarray(y[i].transpose(1, 2, 0)).save(wide / f"{i}.png")
    assert np.array_equal(N.load_images_u8(str(wide), (4, 7), 3), y) and np.array_equal(N.load_images_u8(str(wide)), y)
    with pytest.raises(ValueError):
        N.load_images_u8(str(wide), 4, 3)
    Image.fromarray(np.zeros((6, 6, 3), np.uint8)).save(tmp_path / "c3" / "extra.png")
    with pytest.raises(ValueError, match="not named"):
        N.load_images_u8(str(tmp_path / "c3"), 6, 3)
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no PNG"):
        N.load_images_u8(str(tmp_path / "empty"), 6, 3)


# ------------------------------------------------------------------------------------------------ declarations
def test_header_declares_the_entries():
    from tinyedm_amd import _lib
    with open(os.path.join(ROOT, "include", "tinyedm_hip.h")) as f:
        header = f.read()
    for name in ("edm_u8_knn_splits", "edm_u8_norms", "edm_u8_knn_partial", "edm_knn_merge"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
    with open(os.path.join(ROOT, "tinyedm_amd", "csrc", "neighbors.hip")) as f:
        src = f.read()
    for name in ("edm_u8_knn_splits", "edm_u8_norms", "edm_u8_knn_partial", "edm_knn_merge"):
        assert re.search(r'extern "C" int ' + name + r"\(", src), name
    assert "mfma_i32_16x16x64_i8" in src
