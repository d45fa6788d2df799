"""Feature-space nearest neighbours and ball counts on the GPU (csrc/neighbors_f32.hip through ops.f32_knn,
ops.f32_ball_count, NearestNeighbors, ManifoldMetrics and the two command lines) against the fp64 numpy restatement
(tests/fknn_ref.py).

Exact tier: dyadic inputs (small integers / 8), for which every product and sum is exact in fp64 whatever the order, so
dist and idx are compared bit for bit and the tie rule is exercised.  Float tier: normal inputs, with the tolerance
    |d2_gpu - d2_true| <= (D + 2) u (|q| + |r|)^2,  u = 2^-53
(at most D roundings in each of |q|^2, |r|^2 and q.r, each of a partial sum bounded by |q|^2, |r|^2 and |q||r|, and two
in the epilogue); the test allows twice that and first asserts, on the reference alone, that the neighbours are farther
apart than that, so the indices must agree.  End to end: the classes and the command lines on features."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fknn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as o
    return o


def _dev(x, off=0):
    """x on the device, contiguous; off: floats past a 16-byte boundary at which the rows start (a slice of a larger buffer)"""
    x = np.ascontiguousarray(x)
    if not off:
        t = torch.from_numpy(x).to(DEV)
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(x.size + off, dtype=torch.float32, device=DEV)
    t = buf[off:].view(x.shape)
    t.copy_(torch.from_numpy(x))
    assert t.data_ptr() % 16 == 4 * off and t.is_contiguous()
    return t


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_knn(got, want, what=""):
    """bit for bit: dist fp64 [Q, k], idx int64 [Q, k]"""
    (gd, gi), (wd, wi) = got, want
    assert gd.dtype == torch.float64 and gi.dtype == torch.int64 and tuple(gd.shape) == wd.shape == tuple(gi.shape)
    gd, gi = gd.cpu().numpy(), gi.cpu().numpy()
    assert np.array_equal(gi, wi), f"{what}: idx differs at {np.argwhere(gi != wi)[:4].tolist()}"
    assert np.array_equal(_bits(gd), _bits(wd)), f"{what}: dist differs at {np.argwhere(_bits(gd) != _bits(wd))[:4].tolist()}"


def _same_counts(got, want, what=""):
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
    g = got.cpu().numpy()
    assert np.array_equal(g, want), f"{what}: counts differ at {np.argwhere(g != want)[:5].ravel().tolist()}"


# ------------------------------------------------------------------------------------------------ exact tier
# (Q, R, D, k, off): one row; k = R = 32 at D < 4; a row short of a tile with a K tail of 31; one row past a tile at one
# whole K step; one past in Q with a K step and one element; several tiles both ways, k = 32, odd D; ten K steps, D % 4 == 0
# on the vector path; and D % 4 == 0 with both sets 4 bytes off a 16-byte boundary (element path by alignment alone)
SHAPES = [(1, 1, 1, 1, 0), (1, 32, 3, 32, 0), (63, 64, 31, 5, 0), (64, 65, 32, 5, 0), (65, 127, 33, 7, 0),
          (130, 517, 67, 32, 0), (70, 129, 300, 1, 0), (66, 130, 64, 5, 1)]
_cases = {}


def _case(shape):
    """(q, r, q on the device, r on the device, the reference distance matrix): made once per shape"""
    if shape not in _cases:
        Q, Rn, D, k, off = shape
        q, r = R.dyadic(Q * 1000 + Rn, Q, D), R.dyadic(Q * 1000 + Rn + 1, Rn, D)
        _cases[shape] = (q, r, _dev(q, off), _dev(r, off), R.dist_matrix(q, r))
    return _cases[shape]


def _ids(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_exact_shapes(ops, shape):
    q, r, qd, rd, d = _case(shape)
    k = shape[3]
    _same_knn(ops.f32_knn(qd, rd, k), R.knn(q, r, k, d=d), _ids(shape))


def test_exact_case_has_distance_ties():
    """on the reference alone: these cases hold exact ties among a query's candidates, so the index half of the key decides
    there"""
    for shape in (SHAPES[4], SHAPES[5]):
        d = _case(shape)[4]
        assert sum(len(row) - len(np.unique(row)) for row in d) > 50, shape


def test_exact_mixed_alignment(ops):
    q, r, qd, rd, d = _case(SHAPES[-1])
    want = R.knn(q, r, 5, d=d)
    _same_knn(ops.f32_knn(_dev(q), rd, 5), want, "aligned queries, misaligned refs")
    _same_knn(ops.f32_knn(qd, _dev(r), 5), want, "misaligned queries, aligned refs")
    _same_knn(ops.f32_knn(_dev(q), _dev(r), 5), want, "both aligned")


def test_exact_invariance(ops):
    shape = SHAPES[5]
    q, r, qd, rd, d = _case(shape)                     # 517 references: 9 tiles
    for k in (32, 3):
        want = R.knn(q, r, k, d=d)
        for splits in (1, 2, 9, 40):
            _same_knn(ops.f32_knn(qd, rd, k, splits=splits), want, f"splits {splits}")
        for chunk in (64, 100, 517):
            _same_knn(ops.f32_knn(qd, rd, k, ref_chunk=chunk), want, f"ref_chunk {chunk}")
        _same_knn(ops.f32_knn(qd, rd, k, splits=3, ref_chunk=100), want, "splits and ref_chunk")
    # rank 4 against the flattened form
    a, b = R.dyadic(5, 40, 48), R.dyadic(6, 90, 48)
    want = R.knn(a, b, 4)
    _same_knn(ops.f32_knn(_dev(a).view(40, 3, 4, 4), _dev(b).view(90, 3, 4, 4), 4), want, "rank 4")
    _same_knn(ops.f32_knn(_dev(a), _dev(b), 4), want, "rank 2")


def test_exact_norms(ops):
    """|x|^2 is exact for dyadic rows, so the norm kernel has a unique answer at every shape and on both load paths"""
    for n, D, off in ((1, 1, 0), (63, 31, 0), (65, 32, 0), (130, 300, 0), (129, 64, 1)):
        x = R.dyadic(n + D, n, D)
        got = ops.f32_norms(_dev(x, off))
        assert got.dtype == torch.float64 and tuple(got.shape) == (n,)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits((x.astype(np.float64) ** 2).sum(1)))


def test_exact_exclude_self_with_duplicates(ops):
    x = R.dyadic(7, 200, 45)
    x[17] = x[3]
    x[150] = x[3]
    x[199] = x[64]                                      # a duplicate pair across tiles, one of them the last row
    xd = _dev(x)
    for k, kw in ((5, {}), (32, {}), (5, {"splits": 4}), (5, {"ref_chunk": 64})):
        dist, idx = ops.f32_knn(xd, xd, k, exclude_self=True, **kw)
        _same_knn((dist, idx), R.knn(x, x, k, exclude_self=True), f"k {k} {kw}")
        dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
        assert all(i not in idx[i] for i in range(200))
        # the duplicate is a neighbour at +0.0 exactly (the bit pattern, not just the value), lower index first
        assert idx[3, :2].tolist() == [17, 150] and idx[17, :2].tolist() == [3, 150] and idx[199, 0] == 64
        assert _bits(dist[3, :2]).tolist() == [0, 0] and _bits(dist[199, :1]).tolist() == [0] and dist[3, 2] > 0
    # without the flag every row finds itself first, at +0.0
    dist, idx = ops.f32_knn(xd, xd, 2)
    assert not _bits(dist[:, 0].cpu().numpy()).any()
    first = idx[:, 0].cpu().numpy()
    assert first[17] == 3 and first[150] == 3 and first[199] == 64 and first[5] == 5


def test_exact_against_the_integer_kernels(ops):
    rng = np.random.default_rng(192)
    x = rng.integers(0, 256, (70, 3, 8, 8), dtype=np.uint8)
    y = rng.integers(0, 4, (150, 3, 8, 8), dtype=np.uint8) * 85              # few levels: ties in distance
    y[40] = y[7]
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    for k in (1, 5, 32):
        di, ii = ops.u8_knn(xd, yd, k)
        df, jf = ops.f32_knn(xd.float(), yd.float(), k)
        assert torch.equal(ii, jf) and torch.equal(di.double(), df) and df.dtype == torch.float64
    rad = ops.u8_knn(yd, yd, 5, exclude_self=True)[0][:, 4]
    want = ops.u8_ball_count(xd, yd, rad)
    assert int(want.min()) < int(want.max())
    assert torch.equal(ops.f32_ball_count(xd.float(), yd.float(), rad.double()), want)
    assert torch.equal(ops.f32_ball_count(yd.float(), yd.float(), rad.double(), exclude_self=True),
                       ops.u8_ball_count(yd, yd, rad, exclude_self=True))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_exact_ball_counts(ops, shape):
    """radii: the distance of a randomly chosen query to each reference (a query exactly on every sphere), every 5th radius
    0 and every 7th above every distance"""
    Q, Rn, D, k, off = shape
    q, r, qd, rd, d = _case(shape)
    rng = np.random.default_rng(Q + Rn)
    rad = d[rng.integers(0, Q, Rn), np.arange(Rn)].copy()
    rad[2::5] = 0.0
    rad[3::7] = d.max() + 0.125
    want = R.ball_count(q, r, rad, d=d)
    assert (d == rad[None, :]).any() and (Q < 2 or want.min() < want.max())      # a vacuous case fails here
    radd = torch.from_numpy(rad).to(DEV)
    tiles = (Rn + 63) // 64
    for kw in ({}, {"splits": 1}, {"splits": 2}, {"splits": tiles + 3}, {"ref_chunk": 64}, {"ref_chunk": 100, "splits": 2}):
        _same_counts(ops.f32_ball_count(qd, rd, radd, **kw), want, f"{_ids(shape)} {kw}")
    # an all-zero radius list counts the exact duplicates only, a huge one everything
    _same_counts(ops.f32_ball_count(qd, rd, torch.zeros_like(radd)), (d == 0).sum(1).astype(np.int64))
    _same_counts(ops.f32_ball_count(qd, rd, torch.full_like(radd, float(d.max()))), np.full(Q, Rn, np.int64))


def test_exact_ball_counts_exclude_self(ops):
    x = R.dyadic(11, 200, 45)
    x[17] = x[3]
    x[199] = x[64]
    xd = _dev(x)
    for k in (1, 5):
        dist = ops.f32_knn(xd, xd, k, exclude_self=True)[0]
        rad = R.radii(x, k)
        assert np.array_equal(_bits(dist[:, k - 1].cpu().numpy()), _bits(rad)) and (k > 1 or rad[3] == 0.0)
        want = R.ball_count(x, x, rad, exclude_self=True)
        assert want.min() < want.max()
        for kw in ({}, {"splits": 2}, {"splits": 9}, {"ref_chunk": 128}):
            _same_counts(ops.f32_ball_count(xd, xd, dist[:, k - 1].contiguous(), exclude_self=True, **kw), want, str(kw))
            # a point is always inside its own closed ball: without the flag every count is exactly one higher
            _same_counts(ops.f32_ball_count(xd, xd, dist[:, k - 1].contiguous(), **kw), want + 1, str(kw))


# ------------------------------------------------------------------------------------------------ float tier
FLOAT_CASES = [("normal", 301), ("normal", 67), ("mean3", 301), ("mean3", 67)]
_float = {}


def _float_case(case):
    """Q = 130 queries, R = 517 references; 'mean3': abs(normal) / 2 + 3, non-negative with a large common mean, where the
    expansion cancels the most.  -> (q, r, devices, reference d, allowance [Q, R])"""
    if case not in _float:
        kind, D = case
        rng = np.random.default_rng(D + (0 if kind == "normal" else 1000))
        q, r = rng.standard_normal((130, D)).astype(np.float32), rng.standard_normal((517, D)).astype(np.float32)
        if kind == "mean3":
            q, r = np.abs(q) * np.float32(0.5) + np.float32(3), np.abs(r) * np.float32(0.5) + np.float32(3)
        nq = np.sqrt((q.astype(np.float64) ** 2).sum(1))
        nr = np.sqrt((r.astype(np.float64) ** 2).sum(1))
        allow = 2.0 * (D + 2) * U * (nq[:, None] + nr[None, :]) ** 2
        _float[case] = (q, r, _dev(q), _dev(r), R.dist_matrix(q, r), allow)
    return _float[case]


def _assert_gaps(d, allow, n, what):
    """every gap between consecutive distances among each row's n nearest exceeds twice the allowance (an assert on the
    reference alone, not a filter: nothing is skipped)"""
    s = np.sort(d, axis=1)[:, :n]
    gaps = np.diff(s, axis=1)
    worst = allow.max(1, keepdims=True)
    assert (gaps > 2.0 * worst).all(), f"{what}: a gap of {gaps.min():.3e} against an allowance of {worst.max():.3e}"
    return float((gaps / worst).min())


@pytest.mark.parametrize("case", FLOAT_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_float_knn(ops, case):
    q, r, qd, rd, d, allow = _float_case(case)
    margin = _assert_gaps(d, allow, 33, "queries against references")
    wd, wi = R.knn(q, r, 32, d=d)
    gd, gi = ops.f32_knn(qd, rd, 32)
    gd, gi = gd.cpu().numpy(), gi.cpu().numpy()
    err = np.abs(gd - wd) / np.take_along_axis(allow, wi, 1)
    print(f"{case}: smallest gap {margin:.3g} allowances, worst error {err.max():.3g} of the allowance")
    assert np.array_equal(gi, wi)
    assert (err <= 1.0).all(), f"worst error {err.max():.3g} of the allowance"
    assert (gd >= 0).all() and (np.diff(gd, axis=1) >= 0).all()
    # and invariance holds for rounded sums too: the bits of a distance depend on its two rows only
    for kw in ({"splits": 1}, {"splits": 5}, {"ref_chunk": 100}):
        hd, hi = ops.f32_knn(qd, rd, 32, **kw)
        assert np.array_equal(hi.cpu().numpy(), gi) and np.array_equal(_bits(hd.cpu().numpy()), _bits(gd)), kw
    off = ops.f32_knn(_dev(q, 1), _dev(r, 3), 32)
    assert np.array_equal(off[1].cpu().numpy(), gi) and np.array_equal(_bits(off[0].cpu().numpy()), _bits(gd))


@pytest.mark.parametrize("case", FLOAT_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_float_knn_and_ball_count_agree_to_the_bit(ops, case):
    """the k-th neighbour radius of a search is the very number the ball count compares against: with no ties, every ball
    holds exactly its k neighbours, and one differing bit in either kernel changes the total"""
    _, x, _, xd, _, _ = _float_case(case)
    d = R.dist_matrix(x, x)
    nx = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    allow = 2.0 * (case[1] + 2) * U * (nx[:, None] + nx[None, :]) ** 2
    np.fill_diagonal(d, np.inf)
    _assert_gaps(d, allow, 11, "the set against itself")
    for k in (1, 5, 10):
        radii = ops.f32_knn(xd, xd, k, exclude_self=True)[0][:, k - 1].contiguous()
        for kw in ({}, {"splits": 3}, {"ref_chunk": 200}):
            counts = ops.f32_ball_count(xd, xd, radii, exclude_self=True, **kw)
            assert int(counts.sum()) == k * len(x), (k, kw)
        assert int(ops.f32_ball_count(xd, xd, radii).sum()) == (k + 1) * len(x)
    # the float reference agrees on who is inside (the gaps leave no room for a rounding to decide)
    rad5 = ops.f32_knn(xd, xd, 5, exclude_self=True)[0][:, 4].contiguous()
    np.fill_diagonal(d, 0.0)
    _same_counts(ops.f32_ball_count(xd, xd, rad5, exclude_self=True), R.ball_count(x, x, R.radii(x, 5, d=d), exclude_self=True, d=d))


# ------------------------------------------------------------------------------------------------ end to end
_struct = {}


def _structured():
    """two clusters of dyadic features (D = 24), 120 reals; samples from both clusters, and from the first only"""
    if not _struct:
        rng = np.random.default_rng(24)
        centres = rng.integers(-16, 17, (2, 24))
        centres[1] += 40

        def draw(n, modes):
            lab = rng.integers(0, modes, n)
            return ((centres[lab] + rng.integers(-6, 7, (n, 24))) / 8).astype(np.float32), lab
        (X, lx), (Ya, la), (Yb, lb) = draw(120, 2), draw(90, 2), draw(90, 1)
        _struct.update(X=X, lx=lx, both=(Ya, la), first=(Yb, lb),
                       ref={n: {k: R.prdc(X, Y, k) for k in (3, 5)} for n, Y in (("both", Ya), ("first", Yb))})
    return _struct


def test_manifold_metrics_on_features(ops):
    from tinyedm_amd.prdc import ManifoldMetrics
    s = _structured()
    ref = s["ref"]
    for k in (3, 5):     # on the reference alone: a dropped cluster lowers recall and coverage while precision holds
        assert ref["first"][k]["recall"] < 0.7 * ref["both"][k]["recall"]
        assert ref["first"][k]["coverage"] < 0.7 * ref["both"][k]["coverage"]
        assert ref["first"][k]["precision"] > 0.8 and ref["both"][k]["precision"] > 0.8
    mm = ManifoldMetrics(s["X"], k=(3, 5))
    assert mm.ks == (3, 5) and mm.real.dtype == torch.float32
    for k in (3, 5):
        assert mm.r_x[k].dtype == torch.float64
        assert np.array_equal(_bits(mm.r_x[k].cpu().numpy()), _bits(R.radii(s["X"], k)))
    for name in ("both", "first"):
        assert mm.score(s[name][0]) == ref[name], name
    got = ManifoldMetrics(_dev(s["X"]), k=5, ref_chunk=64).score(torch.from_numpy(s["first"][0]), per_sample=True)
    hx, hy, _, _, _ = R.counts(s["X"], s["first"][0], 5)
    per = got[5].pop("per_sample")
    assert got == {5: ref["first"][5]}
    assert per["hits_x"] == hx.tolist() and per["real_reached"] == (hy > 0).tolist() and not all(per["real_reached"])
    # the two kinds do not mix, and a set is checked where it is taken in
    with pytest.raises(ValueError, match="uint8"):
        mm.score(np.zeros((20, 24), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        ManifoldMetrics(np.zeros((20, 24), np.uint8), k=3).score(s["both"][0])
    with pytest.raises(ValueError):
        mm.score(s["both"][0][:, :23].copy())
    bad = s["both"][0].copy()
    bad[5, 5] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        mm.score(bad)


def test_manifold_metrics_per_class_on_features(ops):
    from tinyedm_amd.prdc import ManifoldMetrics
    s = _structured()
    X, lx = s["X"], s["lx"]
    Y, ly = s["both"]
    ly = ly.copy()
    ly[:4] = 2                                           # class 2: 4 samples and no reals: skipped at every k
    got = ManifoldMetrics(X, k=(3, 5)).score(Y, real_labels=lx, fake_labels=ly)
    for k in (3, 5):
        classes = got[k].pop("per_class")
        assert got[k] == s["ref"]["both"][k]
        want = R.prdc_per_class(X, Y, lx, ly, k)
        assert sorted(classes) == sorted(want) == [0, 1, 2] and want[2] is None and want[0] is not None
        for c, w in want.items():
            if w is None:
                assert "skipped" in classes[c] and classes[c]["num_fake"] == int((ly == c).sum())
            else:
                assert classes[c] == w


def test_nearest_neighbors_on_features(ops):
    from tinyedm_amd.neighbors import NearestNeighbors
    s = _structured()
    X, Y = s["X"], s["both"][0]
    nn = NearestNeighbors(X, k=5)
    assert nn.features and nn.refs.dtype == torch.float32
    _same_knn(nn.search(Y), R.knn(Y, X, 5))
    _same_knn(nn.search(Y, k=1), R.knn(Y, X, 1))
    _same_knn(nn.search(nn.refs, exclude_self=True), R.knn(X, X, 5, exclude_self=True))
    _same_knn(NearestNeighbors(_dev(X), k=5, ref_chunk=50).search(_dev(Y)), R.knn(Y, X, 5))
    with pytest.raises(ValueError, match="uint8"):
        nn.search(np.zeros((4, 24), np.uint8))
    with pytest.raises(ValueError, match="float32"):
        NearestNeighbors(np.zeros((8, 24), np.uint8), k=2).search(Y)
    with pytest.raises(ValueError):
        nn.search(Y.astype(np.float64))


def _run(module, argv, tmp_path):
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    return subprocess.run([sys.executable, "-m", module, *argv], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)


def _cli_files(tmp_path):
    """samples (the first cluster only, one row copied from the reals), reals and a held-out set as .npy, labels as JSON"""
    s = _structured()
    X, lx = s["X"], s["lx"]
    Y, ly = s["first"]
    H = s["both"][0]
    Y = Y.copy()
    Y[7] = X[31]                                         # a copied row: a nearest neighbour at distance 0
    for name, a in (("A", Y), ("B", X), ("C", H)):
        np.save(tmp_path / f"{name}.npy", a)
    for name, lab in (("drawn", ly), ("ref_labels", lx)):
        with open(tmp_path / f"{name}.json", "w") as f:
            json.dump([int(v) for v in lab], f)
    return (X, lx, Y, ly, H) + tuple(str(tmp_path / f"{n}.npy") for n in "ABC")


def test_prdc_command_line_on_features(ops, tmp_path):
    X, lx, Y, ly, H, A, B, C = _cli_files(tmp_path)
    r = _run("tinyedm.prdc", ["--features", A, "--ref_features", B, "--holdout_features", C, "--labels_json",
                              str(tmp_path / "drawn.json"), "--ref_labels", str(tmp_path / "ref_labels.json"), "--k", "3", "5",
                              "--report", str(tmp_path / "prdc.json")], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "prdc.json") as f:
        rep = json.load(f)
    assert rep["k"] == [3, 5] and rep["num_real"] == 120 and rep["num_samples"] == 90 and rep["num_holdout"] == 90
    assert rep["space"] == "features as given (float32)" and rep["feature_dim"] == 24 and "image_shape" not in rep
    for k in (3, 5):
        got = rep["samples"][str(k)]
        classes = got.pop("per_class")
        assert got == R.prdc(X, Y, k) and rep["holdout"][str(k)] == R.prdc(X, H, k)
        want = R.prdc_per_class(X, Y, lx, ly, k)
        assert sorted(classes) == ["0", "1"] and classes["0"] == want[0] and "skipped" in classes["1"]
    assert "samples" in r.stdout and "holdout" in r.stdout and "class 0" in r.stdout


def test_neighbors_command_line_on_features(ops, tmp_path):
    """samples against references with a held-out set"""
    X, lx, Y, ly, H, A, B, C = _cli_files(tmp_path)
    r = _run("tinyedm.neighbors", ["--features", A, "--ref_features", B, "--holdout_features", C, "--k", "5", "--max_d2",
                                   "0.5", "--report", str(tmp_path / "nn.json")], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "nn.json") as f:
        rep = json.load(f)
    wd, wi = R.knn(Y, X, 5)
    hd = R.knn(H, X, 1)[0][:, 0]
    from tinyedm_amd import neighbors as N
    assert rep["space"] == "features as given (float32)" and rep["feature_dim"] == 24 and rep["num_references"] == 120
    assert rep["num_samples"] == 90 and rep["num_holdout"] == 90 and rep["k"] == 5 and rep["max_d2"] == 0.5
    assert [[n["index"] for n in row] for row in rep["neighbours"]] == wi.tolist()
    assert [[n["d2"] for n in row] for row in rep["neighbours"]] == wd.tolist()          # JSON round-trips fp64 exactly
    assert rep["neighbours"][7][0] == {"index": 31, "d2": 0.0, "rms": 0.0}
    assert rep["nearest"] == N.summarize(wd[:, 0]) and rep["holdout_nearest"] == N.summarize(hd)
    assert rep["closer_than_holdout"] == N.closer_than_holdout(wd[:, 0], hd)
    want = [{"sample": i, "index": int(wi[i, 0]), "d2": float(wd[i, 0])} for i in np.nonzero(wd[:, 0] <= 0.5)[0].tolist()]
    assert [{n: e[n] for n in ("sample", "index", "d2")} for e in rep["at_or_under_max_d2"]] == want and len(want) >= 1


def test_neighbors_command_line_self_on_features(ops, tmp_path):
    """--self: duplicates inside one set (the refusals of both command lines are tested in process, test_fknn_cpu.py)"""
    from tinyedm_amd import neighbors as N
    Z = _structured()["X"].copy()
    Z[100] = Z[12]
    np.save(tmp_path / "Z.npy", Z)
    r = _run("tinyedm.neighbors", ["--features", str(tmp_path / "Z.npy"), "--self", "--k", "3", "--report",
                                   str(tmp_path / "self.json")], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "self.json") as f:
        rep = json.load(f)
    assert rep["max_d2"] == 0 and rep["duplicate_pairs"] == [{"i": 12, "j": 100, "d2": 0.0, "rms": 0.0}]
    assert rep["nearest"] == N.summarize(R.knn(Z, Z, 1, exclude_self=True)[0][:, 0])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ops):
    from tinyedm_amd import _lib
    q = torch.zeros(4, 48, dtype=torch.float32, device=DEV)
    r = torch.zeros(6, 48, dtype=torch.float32, device=DEV)
    rad = torch.zeros(6, dtype=torch.float64, device=DEV)
    for bad in (q.double(), q.half(), q.to(torch.uint8)):
        with pytest.raises(TypeError, match="float"):
            ops.f32_knn(bad, r, 1)
        with pytest.raises(TypeError):
            ops.f32_ball_count(bad, r, rad)
        with pytest.raises(TypeError):
            ops.f32_norms(bad)
    with pytest.raises(TypeError):
        ops.f32_knn(q, r.to(torch.uint8), 1)
    for fn in (lambda a, b: ops.f32_knn(a, b, 1), lambda a, b: ops.f32_ball_count(a, b, rad)):
        with pytest.raises(ValueError):
            fn(q.cpu(), r)                                  # the two sets on different devices
        with pytest.raises(ValueError):
            fn(q, r.cpu())
        with pytest.raises(ValueError):
            fn(q, torch.zeros(6, 49, dtype=torch.float32, device=DEV))
        with pytest.raises(ValueError):
            fn(q.view(4, 3, 16), r)
        with pytest.raises(ValueError):
            fn(torch.zeros(4, 96, dtype=torch.float32, device=DEV)[:, ::2], r)
        with pytest.raises(ValueError):
            fn(q.view(-1), r)
    with pytest.raises(RuntimeError):
        ops.f32_knn(q.cpu(), r.cpu(), 1)
    big = torch.zeros(2, 32769, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        ops.f32_knn(big, big, 1)
    for k in (0, 33, 7, True, 2.0):                         # 7 > R = 6
        with pytest.raises(ValueError):
            ops.f32_knn(q, r, k)
    with pytest.raises(ValueError):
        ops.f32_knn(r, r, 6, exclude_self=True)             # k = R with exclude_self
    ops.f32_knn(r, r, 5, exclude_self=True)
    ops.f32_knn(q, r, 6)
    for kw in ({"splits": 0}, {"splits": 1025}, {"splits": True}, {"ref_chunk": 0}, {"ref_chunk": 2.5}):
        with pytest.raises(ValueError):
            ops.f32_knn(q, r, 1, **kw)
        with pytest.raises(ValueError):
            ops.f32_ball_count(q, r, rad, **kw)
    nan = rad.clone()
    nan[2] = float("nan")
    for bad in (rad[:5], rad.view(6, 1), rad.float(), rad.long(), rad.cpu(), [0.0] * 6, rad - 1, rad + float("inf"), nan):
        with pytest.raises(ValueError):
            ops.f32_ball_count(q, r, bad)
    for Q, Rn in ((ops.FKNN_MAX_Q + 1, 6), (4, ops.FKNN_MAX_R + 1)):          # limits no tensor here can reach
        with pytest.raises(ValueError):
            ops.fknn_check(Q, Rn, 48, 1)
    ops.fknn_check(ops.FKNN_MAX_Q, ops.FKNN_MAX_R, 48, 1)
    # the library refuses on its own what ops would not let through to it
    norms = torch.zeros(10, dtype=torch.float64, device=DEV)
    kd = torch.zeros(4 * 32, dtype=torch.uint64, device=DEV)
    ki = torch.zeros(4 * 32, dtype=torch.int32, device=DEV)
    counts = torch.zeros(4, dtype=torch.int32, device=DEV)
    for Q, Rn, D, k, excl, base, splits in ((4, 6, 48, 0, 0, 0, 1), (4, 6, 48, 33, 0, 0, 1), (4, 6, 48, 7, 0, 0, 1),
                                            (6, 6, 48, 6, 1, 0, 1), (4, 6, 0, 1, 0, 0, 1), (4, 6, 32769, 1, 0, 0, 1),
                                            (0, 6, 48, 1, 0, 0, 1), (4, 0, 48, 1, 0, 0, 1), (4, 6, 48, 1, 0, -1, 1),
                                            (4, 6, 48, 1, 0, 2 ** 31 - 64 - 5, 1), (4, 6, 48, 1, 0, 0, 0),
                                            (4, 6, 48, 1, 0, 0, 1025), (65535 * 64 + 1, 6, 48, 1, 0, 0, 1)):
        with pytest.raises(_lib.HipKernelError):
            _lib.call("edm_f32_knn_partial", ops._p(q), ops._p(r), Q, Rn, D, k, excl, base, 0, splits, ops._p(norms),
                      ops._p(norms[4:]), ops._p(kd), ops._p(ki), None)
        if k == 1:
            with pytest.raises(_lib.HipKernelError):
                _lib.call("edm_f32_ball_count_partial", ops._p(q), ops._p(r), Q, Rn, D, ops._p(rad), excl, base, splits,
                          ops._p(norms), ops._p(norms[4:]), ops._p(counts), None)
    with pytest.raises(_lib.HipKernelError):
        _lib.call("edm_f32_knn_partial", ops._p(q), ops._p(r), 4, 6, 48, 1, 0, 0, 0, 1, None, ops._p(norms[4:]), ops._p(kd),
                  ops._p(ki), None)
    for n_rows, D in ((0, 48), (4, 0), (4, 32769), (2 ** 31 - 63, 48)):
        with pytest.raises(_lib.HipKernelError):
            _lib.call("edm_f32_norms", ops._p(q), n_rows, D, ops._p(norms), None)
    for n_lists, Q, k in ((0, 4, 1), (1, 0, 1), (1, 4, 0), (1, 4, 33)):
        with pytest.raises(_lib.HipKernelError):
            _lib.call("edm_fknn_merge", ops._p(kd), ops._p(ki), n_lists, Q, k, ops._p(norms), ops._p(ki), None)
    torch.cuda.synchronize()
