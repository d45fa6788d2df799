"""The fp64 moments and polynomial-kernel sums on the GPU (csrc/moments.hip through ops.moments and ops.poly_kernel_sums),
DistributionDistance and the command line, against the numpy restatement tests/frechet_ref.py.  uint8 results are exact
integers and compared bit for bit; float32 results against the bounds derived in frechet_ref.

The uint8 moment cases carry a few columns of constant 255 and of constant 0.  A gram entry of N rows is at most 65025 N, so
it can only exceed 2^24 (where an fp32 accumulator stops being exact) from N = 259 rows on: the (33100, 48) case asserts
that, and 2^31 for an int32 accumulator, on its own rows; every smaller case is run again through an index of 523 repeated
rows, out of order, whose reference asserts an entry above 2^24 as well."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import frechet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as o
    return o


def _dev(x, off=0):
    """a contiguous device copy whose base sits `off` bytes past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    if off == 0:
        d = t.to(DEV)
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(t.numel() * t.element_size() + 16, dtype=torch.uint8, device=DEV)
    d = buf[off:off + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
    d.copy_(t)
    assert d.data_ptr() % 16 == off and d.is_contiguous()
    return d


def _same_bits(got, want, what):
    g = got.cpu().numpy()
    assert g.dtype == np.float64 and g.shape == want.shape
    bad = np.argwhere(g != want)
    assert bad.size == 0, f"{what}: {len(bad)} entries differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {want[tuple(bad[0])]}"


# ------------------------------------------------------------------------------------------------ moments, uint8
# (N, D, misalign): N tail of the k = 4 step, partial D tile, element loads; vector loads with a partial last tile; full
# tiles and one row past a staged step; the element path by alignment alone; many rows, entries past 2^31
U8_SHAPES = [(37, 75, 0), (130, 784, 0), (257, 3072, 0), (40, 3072, 1), (33100, 48, 0)]
_u8 = {}


def _u8_case(shape):
    if shape not in _u8:
        N, D, off = shape
        rng = np.random.default_rng(N * 7 + D)
        x = rng.integers(0, 256, (N, D), dtype=np.uint8)
        x[:, [1, D // 2, D - 1]] = 255
        x[:, [0, D // 3, D - 2]] = 0
        s, g = R.moments(x)
        assert g.max() == 65025.0 * N and g.min() == 0.0
        if N >= 259:
            assert g.max() > 2 ** 24, "no entry an fp32 accumulator would lose"
        if N == 33100:
            assert g.max() > 2 ** 31, "no entry an int32 accumulator would lose"
        _u8[shape] = (x, _dev(x, off), s, g)
    return _u8[shape]


@pytest.mark.parametrize("shape", U8_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_moments_u8_exact(ops, shape):
    x, xd, s, g = _u8_case(shape)
    N, D, _ = shape
    for splits in (1, 3, None):
        gs, gg = ops.moments(xd, splits=splits)
        _same_bits(gs, s, f"sum, splits {splits}")
        _same_bits(gg, g, f"gram, splits {splits}")          # the full matrix: a missing mirror fails here
    assert 1 <= ops.moments_splits(N, D) <= 1024
    ss, none = ops.moments(xd, sums_only=True)
    assert none is None
    _same_bits(ss, s, "sums only")


@pytest.mark.parametrize("shape", U8_SHAPES[:4], ids=lambda s: "x".join(map(str, s)))
def test_moments_u8_index_repeats_out_of_order(ops, shape):
    x, xd, _, _ = _u8_case(shape)
    idx = np.random.default_rng(3).integers(0, len(x), 523)
    idx[:4] = [len(x) - 1, 0, len(x) - 1, 5]
    assert len(set(idx.tolist())) < 523 and (np.diff(idx) < 0).any()
    s, g = R.moments(x, idx)
    assert g.max() > 2 ** 24, "no entry an fp32 accumulator would lose"
    for splits in (1, 3):
        gs, gg = ops.moments(xd, index=torch.from_numpy(idx).to(DEV), splits=splits)
        _same_bits(gs, s, "sum")
        _same_bits(gg, g, "gram")


def test_moments_more_splits_than_rows(ops):
    x, xd, s, g = _u8_case(U8_SHAPES[0])
    gs, gg = ops.moments(xd, splits=50)                      # 37 rows: some shares are empty and write zeros
    _same_bits(gs, s, "sum")
    _same_bits(gg, g, "gram")


# ------------------------------------------------------------------------------------------------ moments, float32
# (301, 2048), (53, 100): the vector path; (53, 99): the element path of float rows
F32_SHAPES = [(301, 2048), (53, 100), (53, 99)]


@pytest.mark.parametrize("shape", F32_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("shifted", [False, True], ids=["raw", "shift"])
def test_moments_f32_within_the_sum_bound(ops, shape, shifted):
    N, D = shape
    rng = np.random.default_rng(N + D)
    x = (rng.normal(size=(N, D)) * rng.uniform(0.1, 3.0, D) + rng.normal(size=D) * 4).astype(np.float32)
    shift = x.astype(np.float64).mean(0) if shifted else None
    s, g = R.moments(x, shift=shift)
    bs, bg = R.moments_bound(x, shift=shift)
    xd = _dev(x)
    sd = None if shift is None else torch.from_numpy(shift).to(DEV)
    for splits in (1, 3, None):
        gs, gg = ops.moments(xd, shift=sd, splits=splits)
        es, eg = np.abs(gs.cpu().numpy() - s), np.abs(gg.cpu().numpy() - g)
        print(f"splits {splits}: worst sum error / bound {(es / bs).max():.3g}, gram {(eg / bg).max():.3g}")
        assert (es <= bs).all() and (eg <= bg).all()
        again = ops.moments(xd, shift=sd, splits=splits)
        assert torch.equal(again[0], gs) and torch.equal(again[1], gg)          # same arguments, same bits
        assert torch.equal(gg, gg.T)


# ------------------------------------------------------------------------------------------------ kernel sums
def _subset_case(kind, S, m, nx, ny, D, seed):
    """two sets, the subset index lists, and a duplicate planted inside subset 0 of the first set"""
    from tinyedm_amd.frechet import subset_indices
    rng = np.random.default_rng(seed)
    if kind == "u8":
        x, y = rng.integers(0, 256, (nx, D), dtype=np.uint8), rng.integers(0, 256, (ny, D), dtype=np.uint8)
    else:                       # non-negative, as pooled features are
        x, y = np.abs(rng.normal(size=(nx, D))).astype(np.float32), np.abs(rng.normal(size=(ny, D))).astype(np.float32)
    ix, iy = subset_indices(nx, ny, S, m, seed)
    x[ix[0, 1]] = x[ix[0, 0]]
    assert ix[0, 0] != ix[0, 1] and (x[ix[0, 0]] == x[ix[0, 1]]).all()        # equal rows, different indices: must count
    return x, y, ix, iy


SUM_CASES = [("u8", 3, 37, 90, 120, 75), ("u8", 2, 130, 150, 140, 784), ("u8", 2, 128, 128, 130, 3072),
             ("f32", 2, 64, 70, 64, 2048)]


@pytest.mark.parametrize("case", SUM_CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("degree", [1, 3])
def test_poly_kernel_sums_subsets(ops, case, degree):
    kind, S, m, nx, ny, D = case
    x, y, ix, iy = _subset_case(kind, S, m, nx, ny, D, seed=S * 100 + m)
    gamma = 1.0 / D / (255.0 ** 2 if kind == "u8" else 1.0)
    xd, yd = _dev(x), _dev(y)
    ixd, iyd = torch.from_numpy(ix).to(DEV), torch.from_numpy(iy).to(DEV)
    for name, (a, ia, b, ib, excl), (ad, iad, bd, ibd) in (
            ("xx", (x, ix, x, ix, True), (xd, ixd, xd, ixd)), ("yy", (y, iy, y, iy, True), (yd, iyd, yd, iyd)),
            ("xy", (x, ix, y, iy, False), (xd, ixd, yd, iyd))):
        want, mags, terms = R.poly_sums(a, ia, b, ib, gamma, 1.0, degree, excl)
        bound = R.poly_bound(mags, terms, D)
        got = ops.poly_kernel_sums(ad, iad, bd, ibd, gamma, 1.0, degree, excl)
        assert got.dtype == torch.float64 and tuple(got.shape) == (S,)
        err = np.abs(got.cpu().numpy() - want)
        print(f"{name} degree {degree}: worst error / bound {(err / bound).max():.3g}")
        assert (err <= bound).all(), (name, err, bound)
        assert torch.equal(ops.poly_kernel_sums(ad, iad, bd, ibd, gamma, 1.0, degree, excl), got)
    # exclusion goes by index: with it off the sum grows by exactly the m diagonal terms of every subset
    if kind == "u8" and degree == 1:
        for a, ia, ad, iad, excl in ((x, ix, xd, ixd, True), (x, ix, xd, ixd, False), (y, iy, yd, iyd, True)):
            want, _, _ = R.poly_sums(a, ia, a, ia, 1.0, 0.0, 1, excl)           # integers: exact in any order
            assert want.max() < 2 ** 53
            _same_bits(ops.poly_kernel_sums(ad, iad, ad, iad, 1.0, 0.0, 1, excl), want, "integer sums")
        want, _, _ = R.poly_sums(x, ix, y, iy, 1.0, 0.0, 1, False)
        _same_bits(ops.poly_kernel_sums(xd, ixd, yd, iyd, 1.0, 0.0, 1, False), want, "integer cross sums")


@pytest.mark.parametrize("degree", [1, 3])
def test_poly_kernel_sums_full_sets(ops, degree):
    rng = np.random.default_rng(9)
    x, y = rng.integers(0, 256, (37, 75), dtype=np.uint8), rng.integers(0, 256, (301, 75), dtype=np.uint8)
    y[17] = y[200]                                                    # a duplicate image still counts
    xd, yd = _dev(x, 1), _dev(y)                                      # (one set off the 16-byte grid)
    gamma = 1.0 / 75 / 255.0 ** 2
    for a, b, ad, bd, excl in ((x, x, xd, xd, True), (y, y, yd, yd, True), (x, y, xd, yd, False)):
        want, mags, terms = R.poly_sums(a, None, b, None, gamma, 1.0, degree, excl)
        got = ops.poly_kernel_sums(ad, None, bd, None, gamma, 1.0, degree, excl)
        assert tuple(got.shape) == (1,)
        assert (np.abs(got.cpu().numpy() - want) <= R.poly_bound(mags, terms, 75)).all()
        exact, _, _ = R.poly_sums(a, None, b, None, 1.0, 0.0, 1, excl)
        _same_bits(ops.poly_kernel_sums(ad, None, bd, None, 1.0, 0.0, 1, excl), exact, "integer sums")


def test_ops_refusals_on_the_device(ops):
    u = torch.zeros(6, 8, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="contiguous"):
        ops.moments(torch.zeros(6, 16, dtype=torch.uint8, device=DEV)[:, ::2])
    for bad in (torch.tensor([0, 6], device=DEV), torch.tensor([-1], device=DEV)):
        with pytest.raises(ValueError, match=r"\[0, 6\)"):
            ops.moments(u, index=bad)
    with pytest.raises(ValueError, match="int64"):
        ops.moments(u, index=torch.tensor([0], dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="index"):
        ops.moments(u, index=torch.tensor([0]))                                   # on the host
    with pytest.raises(ValueError, match="shift"):
        ops.moments(u.float(), shift=torch.zeros(8, device=DEV))                   # float32, not fp64
    with pytest.raises(ValueError, match="shift"):
        ops.moments(u.float(), shift=torch.zeros(7, dtype=torch.float64, device=DEV))
    for splits in (0, 1025, 2.0, True):
        with pytest.raises(ValueError, match="splits"):
            ops.moments(u, splits=splits)
    ok = torch.zeros(1, 3, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="8 elements, rows of b 4"):
        ops.poly_kernel_sums(u, None, u[:, :4].contiguous(), None, 1.0, 1.0, 3)
    with pytest.raises(ValueError, match=r"\[0, 6\)"):
        ops.poly_kernel_sums(u, ok + 6, u, ok, 1.0, 1.0, 3)
    with pytest.raises(ValueError, match="2 dimension"):
        ops.poly_kernel_sums(u, ok[0], u, ok, 1.0, 1.0, 3)
    with pytest.raises(ValueError, match="same number of subsets"):
        ops.poly_kernel_sums(u, ok, u, torch.zeros(2, 3, dtype=torch.int64, device=DEV), 1.0, 1.0, 3)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def sets():
    rng = np.random.default_rng(31)
    refs = rng.integers(0, 246, (500, 3, 8, 8), dtype=np.uint8)
    samples = np.clip(rng.integers(0, 256, (300, 3, 8, 8)) * 0.8 + 30, 0, 255).astype(np.uint8)
    return refs, samples


def test_distribution_distance_matches_the_reference(ops, sets):
    from tinyedm_amd.frechet import DistributionDistance
    refs, samples = sets
    dd = DistributionDistance(refs)
    got = dd.score(samples, num_subsets=4, subset_size=100, seed=5)
    assert got["fd"] == R.fd(samples, refs)                           # exact moments, shared host arithmetic: equal bits
    assert got["fd"]["fd"] > 0 and got["fd"]["rank_deficient"] is False and got["num_refs"] == 500
    want, bound = R.kid(samples, refs, 4, 100, seed=5)
    assert abs(got["kid"]["kid"] - want["kid"]) <= bound
    assert np.allclose(got["kid"]["per_subset"], want["per_subset"], rtol=0, atol=4 * bound)
    assert got["kid"]["kid"] > 10 * bound                             # the sets differ by far more than the rounding
    full = dd.score(samples, num_subsets=0)["kid"]
    want, bound = R.kid(samples, refs, 0, None)
    assert abs(full["kid"] - want["kid"]) <= bound and full["subset_size"] is None and full["std"] == 0.0
    assert "kid" not in dd.score(samples, kid=False)
    # statistics saved by one run serve the next
    again = DistributionDistance(refs, ref_stats=R.stats(refs)).score(samples, kid=False)
    assert again["fd"] == got["fd"]
    with pytest.raises(ValueError, match="not the statistics"):
        DistributionDistance(refs, ref_stats=R.stats(refs[:-1]))


def test_per_class_table_and_skipped_classes(ops, sets):
    from tinyedm_amd.frechet import DistributionDistance
    refs, samples = sets
    rl = np.arange(500) % 3
    sl = np.arange(300) % 2
    sl[7] = 2                                                          # class 2: one sample only
    got = DistributionDistance(refs).score(samples, labels=sl, ref_labels=rl, kid=False)["per_class"]
    assert sorted(got) == [0, 1, 2]
    assert got[2]["skipped"] and got[2]["num_samples"] == 1 and "fd" not in got[2]
    for c in (0, 1):
        want = R.fd(samples[sl == c], refs[rl == c])
        assert {k: got[c][k] for k in want} == want and got[c]["num_refs"] == int((rl == c).sum())
    with pytest.raises(ValueError, match="both labels and ref_labels"):
        DistributionDistance(refs).score(samples, labels=sl)


def test_planted_shift_is_all_mean_term(ops, sets):
    """Samples = references + 10 grey levels: mean_term is D (10 / 255)^2 -- every element of the mean difference is the
    correctly rounded 10 / 255 (one division of exact integers), so the term equals the closed form up to the rounding of
    a D-term sum of squares, (D + 4) 2^-53 relative -- and the covariances agree up to rounding, so trace_term is 0 within
    frechet_ref.trace_term_bound of the two numpy covariances (n = 500 > D = 192)."""
    from tinyedm_amd.frechet import DistributionDistance
    refs, _ = sets
    moved = refs + 10
    assert moved.dtype == np.uint8 and moved.max() == 255
    got = DistributionDistance(refs).score(moved, kid=False)["fd"]
    D = 192
    assert got == R.fd(moved, refs)
    assert abs(got["mean_term"] - D * (10 / 255) ** 2) <= (D + 4) * R.EPS * D * (10 / 255) ** 2
    ca = np.cov(moved.reshape(500, -1).astype(np.float64) / 255, rowvar=False)
    cb = np.cov(refs.reshape(500, -1).astype(np.float64) / 255, rowvar=False)
    bound = R.trace_term_bound(ca, cb)
    print(f"trace_term {got['trace_term']:.3g}, bound {bound:.3g}, clipped {got['clipped_eigenvalues']}")
    assert bound < 1e-3 * np.trace(cb) and abs(got["trace_term"]) <= bound and got["rank_deficient"] is False


def test_float_features_two_pass(ops):
    from tinyedm_amd.frechet import DistributionDistance, FeatureStats, frechet_distance
    rng = np.random.default_rng(12)
    a = (np.abs(rng.normal(size=(400, 100))) + 50).astype(np.float32)          # a mean far above the spread
    b = (np.abs(rng.normal(size=(350, 100))) * 1.2 + 50).astype(np.float32)
    got = DistributionDistance(a).score(b, num_subsets=0)

    def stats(x):
        x = x.astype(np.float64)
        mu = x.mean(0)
        return FeatureStats(len(x), (x - mu).sum(0), (x - mu).T @ (x - mu), "f32", mu)
    want = frechet_distance(stats(b), stats(a))
    # the shifted moments agree to the sum bound, so the covariances do to ~N 2^-53 of their size; the distance is a
    # difference of traces of size ~100, and 1e-9 of that is four orders above the rounding and six below the distance
    assert abs(got["fd"]["fd"] - want["fd"]) <= 1e-9 * 100 and want["fd"] > 1.0
    assert np.isfinite(got["kid"]["kid"])
    bad = a.copy()
    bad[3, 5] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        DistributionDistance(bad)


# ------------------------------------------------------------------------------------------------ command line
def test_cli_pixels_and_features(ops, sets, tmp_path):
    from PIL import Image
    refs, samples = sets
    refs, samples = refs[:60, :, :4, :4], samples[:50, :, :4, :4]
    for name, x in (("samples", samples), ("refs", refs)):
        (tmp_path / name).mkdir()
        for n, a in enumerate(x):
            Image.fromarray(a.transpose(1, 2, 0)).save(tmp_path / name / f"{n}.png")
    report, saved = tmp_path / "fd.json", tmp_path / "ref.npz"
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    cmd = [sys.executable, "-m", "tinyedm.frechet", "--image_dir", str(tmp_path / "samples"), "--ref_image_dir",
           str(tmp_path / "refs"), "--num_subsets", "3", "--subset_size", "40", "--seed", "2", "--save_ref_stats", str(saved),
           "--report", str(report)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(report) as f:
        rep = json.load(f)
    assert rep["num_refs"] == 60 and rep["feature_dim"] == 48 and rep["samples"]["num_samples"] == 50
    assert rep["samples"]["fd"] == R.fd(samples, refs)
    want, bound = R.kid(samples, refs, 3, 40, seed=2)
    assert abs(rep["samples"]["kid"]["kid"] - want["kid"]) <= bound
    assert "samples" in r.stdout and f"{rep['samples']['fd']['fd']:12.6g}" in r.stdout
    from tinyedm_amd.frechet import FeatureStats
    st = FeatureStats.load(saved)
    assert st.n == 60 and np.array_equal(st.gram, R.stats(refs).gram)

    # the feature form, on the same numbers as float32 features u / 255
    fa, fb = tmp_path / "a.npy", tmp_path / "b.npy"
    np.save(fa, (samples.reshape(50, -1) / 255.0).astype(np.float32))
    np.save(fb, (refs.reshape(60, -1) / 255.0).astype(np.float32))
    rep2 = tmp_path / "fd2.json"
    r = subprocess.run([sys.executable, "-m", "tinyedm.frechet", "--features", str(fa), "--ref_features", str(fb),
                        "--num_subsets", "0", "--report", str(rep2)], capture_output=True, text=True, env=env, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(rep2) as f:
        rep2 = json.load(f)
    # float32 rounding of u / 255 moves every feature by 2^-24 relative: the distance agrees to ~1e-6 of the traces (~8)
    assert abs(rep2["samples"]["fd"]["fd"] - rep["samples"]["fd"]["fd"]) <= 1e-5 * 8
    assert rep2["samples"]["kid"]["num_subsets"] == 0 and rep2["feature_dim"] == 48

    # a bad invocation: the message, a non-zero exit, and no traceback
    bad = subprocess.run(cmd[:-1] + [str(tmp_path / "no.json"), "--subset_size", "51"], capture_output=True, text=True,
                         env=env, timeout=600, cwd=ROOT)
    assert bad.returncode != 0 and "exceeds the smaller" in bad.stderr and "Traceback" not in bad.stderr
    assert not (tmp_path / "no.json").exists()
