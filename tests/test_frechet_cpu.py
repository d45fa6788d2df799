"""The host side of the Frechet distance and KID (tinyedm_amd/frechet.py) and the operand checks of ops.moments and
ops.poly_kernel_sums that precede a device call: closed forms, numpy.cov, a brute-force MMD^2, every refusal.  No GPU."""
import argparse

import numpy as np
import pytest
import torch

import frechet_ref as R
from tinyedm_amd import frechet as F


def _stats_of_cov(cov, n=1000, mean=None):
    """FeatureStats of a float set whose covariance (ddof 1) is exactly `cov` and whose mean is `mean`"""
    D = cov.shape[0]
    mean = np.zeros(D) if mean is None else mean
    return F.FeatureStats(n, n * mean, (n - 1) * cov + n * np.outer(mean, mean), "f32")


def _basis(D, seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(D, D)))
    return q


# ------------------------------------------------------------------------------------------------ frechet_distance
@pytest.mark.parametrize("D", [1, 75])
def test_fd_shared_eigenbasis_closed_form(D):
    rng = np.random.default_rng(D)
    q = _basis(D, 3)
    a, b = rng.uniform(0.1, 2.0, D), rng.uniform(0.1, 2.0, D)
    ma, mb = rng.normal(size=D), rng.normal(size=D)
    got = F.frechet_distance(_stats_of_cov((q * a) @ q.T, mean=ma), _stats_of_cov((q * b) @ q.T, mean=mb))
    want_trace = a.sum() + b.sum() - 2 * np.sqrt(a * b).sum()
    want_mean = ((ma - mb) ** 2).sum()
    # eigenvalues are bounded away from 0 here, so the terms are good to a modest multiple of D 2^-53 times their operands
    tol = 1e3 * D * R.EPS * (a.sum() + b.sum() + (ma ** 2).sum() + (mb ** 2).sum())
    assert abs(got["trace_term"] - want_trace) <= tol and abs(got["mean_term"] - want_mean) <= tol
    assert got["fd"] == got["mean_term"] + got["trace_term"]
    assert got["clipped_eigenvalues"] == 0 and got["rank_deficient"] is False


def test_fd_of_a_set_with_itself_and_the_rank_flag():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (200, 48), dtype=np.uint8)            # n > D: full rank
    s = R.stats(x)
    got = F.frechet_distance(s, s)
    tr = np.trace(s.cov())
    assert got["mean_term"] == 0.0 and abs(got["fd"]) <= 1e-9 * tr and got["rank_deficient"] is False
    few = R.stats(x[:48])                                          # n <= D
    assert F.frechet_distance(few, s)["rank_deficient"] is True and F.frechet_distance(s, few)["rank_deficient"] is True
    assert F.frechet_distance(R.stats(x[:49]), s)["rank_deficient"] is False


def test_fd_counts_clipped_eigenvalues_of_an_indefinite_product():
    q = _basis(6, 1)
    a = _stats_of_cov((q * np.array([1.0, 2, 3, 4, 5, 6])) @ q.T)
    b = _stats_of_cov((q * np.array([1.0, -2, 3, -4, 5, 6])) @ q.T)        # not a covariance: two negative directions
    got = F.frechet_distance(a, b)
    assert got["clipped_eigenvalues"] == 2
    want = 21 + 9 - 2 * (1 + 3 + 5 + 6)
    assert abs(got["trace_term"] - want) <= 1e-12 * 30
    assert F.frechet_distance(b, a)["clipped_eigenvalues"] >= 2           # the root of the indefinite one clips as well


def test_fd_refusals():
    s = R.stats(np.random.default_rng(0).integers(0, 256, (5, 4), dtype=np.uint8))
    with pytest.raises(ValueError, match="two FeatureStats"):
        F.frechet_distance(s, None)
    with pytest.raises(ValueError, match="4 and 3 features"):
        F.frechet_distance(s, F.FeatureStats(5, np.zeros(3), np.eye(3), "u8"))
    with pytest.raises(ValueError, match="2 rows in each set"):
        F.frechet_distance(s, F.FeatureStats(1, np.zeros(4), np.eye(4), "u8"))


# ------------------------------------------------------------------------------------------------ FeatureStats
def test_stats_merge_of_two_halves_is_the_whole_u8():
    x = np.random.default_rng(2).integers(0, 256, (301, 3, 4, 4), dtype=np.uint8)
    whole, m = R.stats(x), R.stats(x[:120]).merge(R.stats(x[120:]))
    assert m.n == 301 and np.array_equal(m.sum, whole.sum) and np.array_equal(m.gram, whole.gram)
    assert np.array_equal(whole.gram, np.round(whole.gram)) and m.kind == "u8" and m.shift is None


def test_stats_mean_and_cov_against_numpy():
    x = np.random.default_rng(3).integers(0, 256, (77, 20), dtype=np.uint8)
    s = R.stats(x)
    f = x.astype(np.float64) / 255
    assert np.allclose(s.mean(), f.mean(0), rtol=1e-13, atol=0)
    assert np.allclose(s.cov(), np.cov(f, rowvar=False), rtol=1e-11, atol=1e-15)
    assert np.allclose(s.cov(ddof=0), np.cov(f, rowvar=False, ddof=0), rtol=1e-11, atol=1e-15)
    with pytest.raises(ValueError, match="ddof"):
        F.FeatureStats(1, np.zeros(2), np.eye(2), "u8").cov()


def test_stats_float_shift_and_merge():
    rng = np.random.default_rng(4)
    x = (rng.normal(size=(90, 7)) * 0.01 + 100.0).astype(np.float32).astype(np.float64)    # a large mean, a small spread
    parts = []
    for lo, hi in ((0, 40), (40, 90)):
        mu = x[lo:hi].mean(0)
        y = x[lo:hi] - mu
        parts.append(F.FeatureStats(hi - lo, y.sum(0), y.T @ y, "f32", mu))
    m = parts[0].merge(parts[1])
    assert m.n == 90 and np.array_equal(m.shift, parts[0].shift)
    assert np.allclose(m.mean(), x.mean(0), rtol=1e-14, atol=0)
    assert np.allclose(m.cov(), np.cov(x, rowvar=False), rtol=1e-9, atol=1e-18)


def test_stats_save_load_round_trip(tmp_path):
    x = np.random.default_rng(6).integers(0, 256, (30, 12), dtype=np.uint8)
    s = R.stats(x)
    s.save(tmp_path / "ref.npz")
    t = F.FeatureStats.load(tmp_path / "ref.npz")
    assert (t.n, t.kind, t.shift) == (30, "u8", None) and np.array_equal(t.sum, s.sum) and np.array_equal(t.gram, s.gram)
    f = F.FeatureStats(9, np.arange(3.0), np.eye(3) * 5, "f32", np.array([0.5, 1.5, 2.5]))
    f.save(tmp_path / "f.npz")
    g = F.FeatureStats.load(tmp_path / "f.npz")
    assert g.kind == "f32" and np.array_equal(g.shift, f.shift) and np.array_equal(g.gram, f.gram) and g.n == 9
    np.savez(tmp_path / "bad.npz", n=3)
    with pytest.raises(ValueError, match="lacks"):
        F.FeatureStats.load(tmp_path / "bad.npz")


def test_stats_refusals():
    with pytest.raises(ValueError, match="kind"):
        F.FeatureStats(3, np.zeros(2), np.eye(2), "f16")
    with pytest.raises(ValueError, match="n must be"):
        F.FeatureStats(0, np.zeros(2), np.eye(2), "u8")
    with pytest.raises(ValueError, match=r"sum \[D\] and gram \[D, D\]"):
        F.FeatureStats(3, np.zeros(2), np.eye(3), "u8")
    with pytest.raises(ValueError, match="shift"):
        F.FeatureStats(3, np.zeros(2), np.eye(2), "u8", np.zeros(2))
    with pytest.raises(ValueError, match="non-finite"):
        F.FeatureStats(3, np.array([0.0, np.nan]), np.eye(2), "f32")
    with pytest.raises(ValueError, match="same kind"):
        F.FeatureStats(3, np.zeros(2), np.eye(2), "u8").merge(F.FeatureStats(3, np.zeros(2), np.eye(2), "f32"))


# ------------------------------------------------------------------------------------------------ subsets and KID
def test_subset_indices():
    ix, iy = F.subset_indices(50, 40, 7, 30, seed=11)
    jx, jy = F.subset_indices(50, 40, 7, 30, seed=11)
    assert np.array_equal(ix, jx) and np.array_equal(iy, jy) and ix.dtype == np.int64 and ix.shape == iy.shape == (7, 30)
    assert not np.array_equal(ix, F.subset_indices(50, 40, 7, 30, seed=12)[0])
    for row in list(ix) + list(iy):
        assert len(set(row.tolist())) == 30                          # without replacement inside a subset
    assert ix.min() >= 0 and ix.max() < 50 and iy.min() >= 0 and iy.max() < 40
    rng = np.random.default_rng(11)                                  # the documented order of draws
    assert np.array_equal(ix[0], rng.choice(50, 30, replace=False)) and np.array_equal(iy[0], rng.choice(40, 30, replace=False))
    with pytest.raises(ValueError, match="exceeds the smaller set"):
        F.subset_indices(50, 40, 7, 41, seed=0)
    with pytest.raises(ValueError, match="num_subsets"):
        F.subset_indices(50, 40, 0, 10, seed=0)
    with pytest.raises(ValueError, match="subset_size"):
        F.subset_indices(50, 40, 2, 1, seed=0)


def test_kid_from_sums_against_brute_force_mmd():
    rng = np.random.default_rng(8)
    x, y = rng.normal(size=(12, 5)), rng.normal(size=(12, 5)) + 0.5

    def k(u, v):
        return (u @ v / 5 + 1.0) ** 3
    sxx = sum(k(x[i], x[j]) for i in range(12) for j in range(12) if i != j)
    syy = sum(k(y[i], y[j]) for i in range(12) for j in range(12) if i != j)
    sxy = sum(k(x[i], y[j]) for i in range(12) for j in range(12))
    want = sxx / (12 * 11) + syy / (12 * 11) - 2 * sxy / 144
    got = F.kid_from_sums([sxx, sxx], [syy, syy], [sxy, sxy + 144.0], 12)
    assert np.isclose(got["per_subset"][0], want, rtol=1e-13) and np.isclose(got["per_subset"][1], want - 2.0, rtol=1e-13)
    assert np.isclose(got["kid"], want - 1.0, rtol=1e-13) and np.isclose(got["std"], 1.0, rtol=1e-12)
    uneven = F.kid_from_sums([sxx], [6.0], [sxy], (12, 3))             # the full-set form: two sizes
    assert np.isclose(uneven["kid"], sxx / 132 + 1.0 - 2 * sxy / 36, rtol=1e-13) and uneven["std"] == 0.0
    with pytest.raises(ValueError, match="one length"):
        F.kid_from_sums([1.0], [1.0, 2.0], [1.0], 5)
    with pytest.raises(ValueError, match="m must be"):
        F.kid_from_sums([1.0], [1.0], [1.0], 1)


def test_kid_refuses_bad_kernels_before_the_device():
    x = torch.zeros(4, 3, dtype=torch.uint8)
    for kw, msg in ((dict(degree=5), "degree"), (dict(degree=True), "degree"), (dict(gamma=0.0), "gamma"),
                    (dict(gamma=float("nan")), "gamma"), (dict(coef0=float("inf")), "coef0")):
        with pytest.raises(ValueError, match=msg):
            F.kid(x, x, **kw)
    with pytest.raises(ValueError, match="differ in kind or row shape"):
        F.kid(x, x.float())
    with pytest.raises(ValueError, match="exceeds the smaller set"):
        F.kid(x, x, num_subsets=2, subset_size=5)


# ------------------------------------------------------------------------------------------------ command line
def _args(**kw):
    base = dict(image_dir=None, dataset=None, data_dir=None, ref_image_dir=None, features=None, ref_features=None, holdout=False,
                labels_json=None, num_subsets=100, subset_size=1000, degree=3, seed=0, no_kid=False, ref_stats=None,
                save_ref_stats=None, report="r.json")
    base.update(kw)
    return argparse.Namespace(**base)


def test_check_args_accepts_both_forms_and_the_parser_defaults():
    F.check_args(_args(image_dir="s", dataset="cifar10", data_dir="d", holdout=True, labels_json="l.json"))
    F.check_args(_args(image_dir="s", ref_image_dir="r", save_ref_stats="o.npz"))
    F.check_args(_args(features="a.npy", ref_features="b.npy", num_subsets=0, ref_stats="i.npz"))
    a = F.build_parser().parse_args(["--features", "a.npy", "--ref_features", "b.npy", "--report", "o.json"])
    F.check_args(a)
    assert (a.num_subsets, a.subset_size, a.degree, a.seed) == (100, 1000, 3, 0)


@pytest.mark.parametrize("kw, msg", [
    (dict(image_dir="s", dataset="mnist", data_dir="d", features="a.npy"), "not both"),
    (dict(features="a.npy"), "both --features and --ref_features"),
    (dict(ref_features="b.npy"), "both --features and --ref_features"),
    (dict(features="a.npy", ref_features="b.npy", holdout=True), "go with --dataset"),
    (dict(features="a.npy", ref_features="b.npy", labels_json="l"), "go with --dataset"),
    (dict(), "give the samples"),
    (dict(dataset="mnist", data_dir="d"), "give the samples"),
    (dict(image_dir="s"), "exactly one source"),
    (dict(image_dir="s", dataset="mnist", data_dir="d", ref_image_dir="r"), "exactly one source"),
    (dict(image_dir="s", dataset="mnist"), "--dataset needs --data_dir"),
    (dict(image_dir="s", ref_image_dir="r", data_dir="d"), "--data_dir goes with --dataset"),
    (dict(image_dir="s", ref_image_dir="r", holdout=True), "--holdout takes the test split"),
    (dict(image_dir="s", ref_image_dir="r", labels_json="l"), "--labels_json needs"),
    (dict(image_dir="s", ref_image_dir="r", ref_stats="a", save_ref_stats="b"), "not both"),
    (dict(image_dir="s", ref_image_dir="r", num_subsets=-1), "--num_subsets"),
    (dict(image_dir="s", ref_image_dir="r", subset_size=1), "--subset_size"),
    (dict(image_dir="s", ref_image_dir="r", degree=0), "degree"),
    (dict(image_dir="s", ref_image_dir="r", degree=5), "degree"),
    (dict(image_dir="s", ref_image_dir="r", seed=-1), "--seed"),
])
def test_check_args_refusals(kw, msg):
    with pytest.raises(ValueError, match=msg):
        F.check_args(_args(**kw))


def test_check_sets_and_feature_files(tmp_path):
    refs = np.zeros((10, 6), np.float32)
    F.check_sets(refs, {"samples": np.zeros((8, 6), np.float32)}, 3, 8)
    F.check_sets(refs, {"samples": np.zeros((8, 6), np.float32)}, 0, 1000)       # the full-set form has no subset size
    with pytest.raises(ValueError, match="rows are"):
        F.check_sets(refs, {"samples": np.zeros((8, 5), np.float32)}, 3, 8)
    with pytest.raises(ValueError, match="exceeds the smaller"):
        F.check_sets(refs, {"samples": np.zeros((8, 6), np.float32)}, 3, 9)
    with pytest.raises(ValueError, match="2 rows"):
        F.check_sets(refs, {"samples": np.zeros((1, 6), np.float32)}, 0, 2)
    np.save(tmp_path / "d.npy", np.zeros((4, 3)))
    with pytest.raises(ValueError, match="float32"):
        F._read_features(tmp_path / "d.npy", "--features")
    bad = np.zeros((4, 3), np.float32)
    bad[1, 1] = np.inf
    np.save(tmp_path / "i.npy", bad)
    with pytest.raises(ValueError, match="non-finite"):
        F._read_features(tmp_path / "i.npy", "--features")


def test_main_ends_in_the_parsers_error_before_the_device(tmp_path, capsys):
    np.save(tmp_path / "a.npy", np.zeros((5, 3), np.float32))
    np.save(tmp_path / "b.npy", np.zeros((5, 4), np.float32))
    with pytest.raises(SystemExit) as e:
        F.main(["--features", str(tmp_path / "a.npy"), "--ref_features", str(tmp_path / "b.npy"), "--num_subsets", "0",
                "--report", str(tmp_path / "o.json")])
    assert e.value.code != 0 and "rows are (3,)" in capsys.readouterr().err and not (tmp_path / "o.json").exists()


def test_alias_package_exports():
    import tinyedm.frechet as S
    import tinyedm_amd
    for name in ("DistributionDistance", "FeatureStats", "frechet_distance", "kid", "kid_from_sums", "subset_indices"):
        assert getattr(S, name) is getattr(F, name) and getattr(tinyedm_amd, name) is getattr(F, name)
    assert S.main is F.main


# ------------------------------------------------------------------------------------------------ ops: checks before the device
def test_ops_moments_refusals_on_the_host():
    from tinyedm_amd import ops
    u = torch.zeros(6, 5, dtype=torch.uint8)
    with pytest.raises(TypeError, match=r"\.float\(\)"):
        ops.moments(u.double())
    with pytest.raises(TypeError, match=r"\.float\(\)"):
        ops.moments(u.to(torch.float16))
    with pytest.raises(TypeError, match="expected a tensor"):
        ops.moments(np.zeros((6, 5), np.uint8))
    with pytest.raises(ValueError, match="non-empty"):
        ops.moments(torch.zeros(6, dtype=torch.uint8))
    with pytest.raises(ValueError, match="non-empty"):
        ops.moments(torch.zeros(6, 0, dtype=torch.uint8))               # D >= 1
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.moments(u)                                                  # a well-formed host tensor: CUDA tensors only
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.moments(u.float())


def test_ops_poly_kernel_sums_refusals_on_the_host():
    from tinyedm_amd import ops
    u = torch.zeros(6, 5, dtype=torch.uint8)
    for deg in (0, 5, 2.0, True, None):
        with pytest.raises(ValueError, match="degree"):
            ops.poly_kernel_sums(u, None, u, None, 1.0, 1.0, deg)
    with pytest.raises(ValueError, match="finite"):
        ops.poly_kernel_sums(u, None, u, None, float("nan"), 1.0, 3)
    with pytest.raises(ValueError, match="finite"):
        ops.poly_kernel_sums(u, None, u, None, 1.0, float("inf"), 3)
    with pytest.raises(TypeError, match=r"\.float\(\)"):
        ops.poly_kernel_sums(u.double(), None, u, None, 1.0, 1.0, 3)
    with pytest.raises(TypeError, match=r"\.float\(\)"):
        ops.poly_kernel_sums(u.to(torch.int32), None, u, None, 1.0, 1.0, 3)
    with pytest.raises(ValueError, match="non-empty"):
        ops.poly_kernel_sums(torch.zeros(0, 5, dtype=torch.uint8), None, u, None, 1.0, 1.0, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.poly_kernel_sums(u, None, u, None, 1.0, 1.0, 3)
