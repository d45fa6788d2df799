"""Ball counts and precision / recall / density / coverage on the GPU (csrc/neighbors.hip k_u8_ball_count through
ops.u8_ball_count, ManifoldMetrics and the command line): integer equality with the int64 numpy restatement
(tests/prdc_ref.py) at the shapes of test_neighbors_gpu.py, each of which guards a path of the shared distance tile.  No
tolerance anywhere: a count is an integer sum."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import prdc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
RATIOS = ("precision", "recall", "density", "coverage")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as o
    return o


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _eq(got, want):
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
    g = got.cpu().numpy()
    assert np.array_equal(g, want), f"counts differ at {np.argwhere(g != want)[:5].ravel().tolist()}: {g[g != want][:5]} != {want[g != want][:5]}"


# ------------------------------------------------------------------------------------------------ shapes
# (Q, R, D, misalign): element loads, K tail, partial tiles both ways; 16-byte path with D % 64 == 16 and one row past a
# tile in Q and R; full tiles; the element path by alignment alone
SHAPES = [(37, 301, 75, 0), (130, 257, 784, 0), (128, 512, 3072, 0), (5, 40, 3072, 1)]
_cases = {}


def _case(shape):
    """(q, r, radii int64, q device, r device, radii device, reference counts): made once per shape.  Radii: the distance of
    a randomly chosen query to each reference (so every reference has a query exactly on its sphere), then every 17th
    radius 0, another residue class 2^31 and another 2^32 - 1."""
    if shape not in _cases:
        Q, Rn, D, off = shape
        rng = np.random.default_rng(Q * 1000 + Rn)
        q = rng.integers(0, 256, (Q, D), dtype=np.uint8)
        r = rng.integers(0, 256, (Rn, D), dtype=np.uint8)
        d = R.dist_matrix(q, r)
        rad = d[rng.integers(0, Q, Rn), np.arange(Rn)].copy()
        rad[0::17] = 0
        rad[5::17] = 2 ** 31
        rad[11::17] = 2 ** 32 - 1
        want = R.ball_count(q, r, rad)
        # a vacuous case fails here, on the reference alone
        assert want.min() < want.max(), "every count is the same"
        assert (d == rad[None, :]).any(), "no distance equals its radius"
        assert (rad >= 2 ** 31).any(), "no radius at or above 2^31"
        buf = torch.empty(Q * D + off, dtype=torch.uint8, device=DEV)
        qd = buf[off:].view(Q, D)
        qd.copy_(torch.from_numpy(q))
        assert qd.data_ptr() % 16 == off and qd.is_contiguous()
        _cases[shape] = (q, r, rad, qd, _dev(r), _dev(rad), want)
    return _cases[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes(ops, shape):
    q, r, rad, qd, rd, radd, want = _case(shape)
    _eq(ops.u8_ball_count(qd, rd, radd), want)
    _eq(ops.u8_ball_count(qd, rd, radd.to(torch.uint32)), want)        # the kernel's own radius type


# ------------------------------------------------------------------------------------------------ independence
def test_splits_chunks_and_rank_do_not_matter(ops):
    q, r, rad, qd, rd, radd, want = _case(SHAPES[1])
    for splits in (1, 2, 3, 7, None):                  # 7 > the three reference tiles: empty shares must write zeros
        _eq(ops.u8_ball_count(qd, rd, radd, splits=splits), want)
    for chunk in (64, 101, None):
        _eq(ops.u8_ball_count(qd, rd, radd, ref_chunk=chunk), want)
        _eq(ops.u8_ball_count(qd, rd, radd, splits=2, ref_chunk=chunk), want)
    _eq(ops.u8_ball_count(qd.view(-1, 1, 28, 28), rd.view(-1, 1, 28, 28), radd), want)


def test_empty_shares_write_zeros(ops):
    """the library entry on a poisoned buffer: 7 shares of 3 reference tiles, every element written, the empty ones 0"""
    from tinyedm_amd import _lib
    q, r, rad, qd, rd, radd, want = _case(SHAPES[1])
    Q, Rn, D, _ = SHAPES[1]
    qn, rn = ops.u8_norms(qd), ops.u8_norms(rd)
    pad = 2
    buf = torch.full((7 + 2 * pad, Q), -77, dtype=torch.int32, device=DEV)
    _lib.call("edm_u8_ball_count_partial", ops._p(qd), ops._p(rd), Q, Rn, D, ops._p(radd.to(torch.uint32)), 0, 0, 7,
              ops._p(qn), ops._p(rn), ops._p(buf[pad:]), None)
    b = buf.cpu().numpy().astype(np.int64)
    assert (b[:pad] == -77).all() and (b[pad + 7:] == -77).all()
    assert (b[pad:pad + 7] >= 0).all() and np.array_equal(b[pad:pad + 7].sum(0), want)
    empty = [s for s in range(7) if 3 * s // 7 == 3 * (s + 1) // 7]
    assert len(empty) == 4 and (b[pad:pad + 7][empty] == 0).all()


# ------------------------------------------------------------------------------------------------ exclude_self
def test_exclude_self(ops):
    rng = np.random.default_rng(300)
    x = rng.integers(0, 256, (300, 784), dtype=np.uint8)
    x[203] = x[17]                                      # a planted exact duplicate pair: radius 0 at k = 1
    xd = _dev(x)
    for k in (1, 5):
        rad = R.radii(x, k)
        dist = ops.u8_knn(xd, xd, k, exclude_self=True)[0]
        assert np.array_equal(dist[:, k - 1].cpu().numpy(), rad)
        want = R.ball_count(x, x, rad, exclude_self=True)
        assert want.min() < want.max()
        for splits, chunk in ((None, None), (2, None), (None, 128)):
            got = ops.u8_ball_count(xd, xd, dist[:, k - 1], exclude_self=True, splits=splits, ref_chunk=chunk)
            _eq(got, want)
            # a point is always inside its own closed ball: without the flag every count is exactly one higher
            _eq(ops.u8_ball_count(xd, xd, dist[:, k - 1], splits=splits, ref_chunk=chunk), want + 1)
    assert R.radii(x, 1)[17] == 0 and R.radii(x, 1)[203] == 0


# ------------------------------------------------------------------------------------------------ range
def test_largest_distance_and_largest_radius(ops):
    D = 32768
    q = np.stack([np.zeros(D, np.uint8), np.full(D, 255, np.uint8)])
    r = np.stack([np.zeros(D, np.uint8), np.full(D, 255, np.uint8), np.full(D, 128, np.uint8)])
    top = 65025 * 32768
    assert top == 2130739200 and R.dist_matrix(q, r).max() == top
    qd, rd = _dev(q), _dev(r)
    for rad in ([top, top, top], [top - 1, top - 1, top - 1], [2 ** 32 - 1] * 3, [0, 0, 0], [2 ** 31, top - 1, 2 ** 32 - 1],
                [top - 1, 2 ** 31, 128 * 128 * D - 1]):
        want = R.ball_count(q, r, rad)
        _eq(ops.u8_ball_count(qd, rd, torch.tensor(rad, dtype=torch.int64, device=DEV)), want)
    assert R.ball_count(q, r, [top] * 3).tolist() == [3, 3] and R.ball_count(q, r, [top - 1] * 3).tolist() == [2, 2]
    assert R.ball_count(q, r, [2 ** 32 - 1] * 3).tolist() == [3, 3]    # a signed compare would empty these balls


# ------------------------------------------------------------------------------------------------ ManifoldMetrics
def _structured():
    """6 base images of D = 48; reals: 200 draws of base + uniform noise +-20; samples (a) 150 draws from all 6 modes,
    (b) from 3 modes, (c) all modes with noise +-60"""
    rng = np.random.default_rng(48)
    base = rng.integers(60, 196, (6, 48))

    def draw(n, modes, amp):
        lab = rng.integers(0, modes, n)
        return np.clip(base[lab] + rng.integers(-amp, amp + 1, (n, 48)), 0, 255).astype(np.uint8), lab
    return draw(200, 6, 20), draw(150, 6, 20), draw(150, 3, 20), draw(150, 6, 60)


_struct = {}


def _structured_ref():
    if not _struct:
        (X, lx), a, b, c = _structured()
        _struct.update(X=X, lx=lx, sets={"a": a, "b": b, "c": c},
                       ref={n: {k: R.prdc(X, Y, k) for k in (3, 5)} for n, (Y, _) in (("a", a), ("b", b), ("c", c))})
    return _struct


def test_manifold_metrics_structured(ops):
    from tinyedm_amd.prdc import ManifoldMetrics
    s = _structured_ref()
    ref = s["ref"]
    # orderings the reference itself satisfies: dropped modes lower recall and coverage, noise lowers precision
    for k in (3, 5):
        assert ref["b"][k]["recall"] < ref["a"][k]["recall"] and ref["b"][k]["coverage"] < ref["a"][k]["coverage"]
        assert ref["c"][k]["precision"] < ref["a"][k]["precision"]
    mm = ManifoldMetrics(s["X"], k=(3, 5))
    assert mm.ks == (3, 5)
    for k in (3, 5):
        assert np.array_equal(mm.r_x[k].cpu().numpy(), R.radii(s["X"], k))
    for name, (Y, _) in s["sets"].items():
        assert mm.score(Y) == ref[name], name
    got = ManifoldMetrics(_dev(s["X"]).view(-1, 3, 4, 4), k=5, ref_chunk=64).score(s["sets"]["b"][0].reshape(-1, 3, 4, 4),
                                                                                  per_sample=True)
    hx, hy, _, _, _ = R.counts(s["X"], s["sets"]["b"][0], 5)
    per = got[5].pop("per_sample")
    assert got == {5: ref["b"][5]}
    assert per["hits_x"] == hx.tolist() and per["real_reached"] == (hy > 0).tolist() and not all(per["real_reached"])


def test_manifold_metrics_per_class(ops):
    from tinyedm_amd.prdc import ManifoldMetrics
    s = _structured_ref()
    X, lx = s["X"], s["lx"].copy()
    Y, ly = s["sets"]["b"]                               # samples of classes 0..2 only
    ly = ly.copy()
    ly[:4] = 5                                           # class 5: 4 samples, enough for k = 3 and not for k = 5
    got = ManifoldMetrics(X, k=(3, 5)).score(Y, real_labels=lx, fake_labels=ly)
    for k in (3, 5):
        classes = got[k].pop("per_class")
        assert got[k] == s["ref"]["b"][k]
        want = R.prdc_per_class(X, Y, lx, ly, k)
        assert sorted(classes) == sorted(want) == [0, 1, 2, 3, 4, 5]
        for c, w in want.items():
            if w is None:
                assert "skipped" in classes[c] and classes[c]["num_fake"] == int((ly == c).sum())
            else:
                assert classes[c] == w
        assert want[3] is None and want[4] is None and (want[5] is None) == (k == 5)
    with pytest.raises(ValueError):
        ManifoldMetrics(X, k=5).score(Y, real_labels=lx)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ops):
    q = torch.zeros(4, 48, dtype=torch.uint8, device=DEV)
    r = torch.zeros(6, 48, dtype=torch.uint8, device=DEV)
    rad = torch.zeros(6, dtype=torch.int64, device=DEV)
    assert ops.u8_ball_count(q, r, rad).tolist() == [6] * 4
    with pytest.raises(TypeError):
        ops.u8_ball_count(q.float(), r, rad)
    with pytest.raises(RuntimeError):
        ops.u8_ball_count(q.cpu(), r, rad)
    for bad in (rad[:5], rad.view(6, 1), rad.int(), rad.float(), rad.cpu(), [0] * 6, rad - 1, rad + 2 ** 32):
        with pytest.raises(ValueError):
            ops.u8_ball_count(q, r, bad)
    with pytest.raises(ValueError):
        ops.u8_ball_count(q, torch.zeros(6, 49, dtype=torch.uint8, device=DEV), rad)
    with pytest.raises(ValueError):
        ops.u8_ball_count(q, r, rad, splits=0)
    with pytest.raises(ValueError):
        ops.u8_ball_count(q, r, rad, ref_chunk=0)
    # the library refuses on its own what ops would not let through to it
    from tinyedm_amd import _lib
    counts = torch.empty(1, 4, dtype=torch.int32, device=DEV)
    norms = torch.zeros(10, dtype=torch.int32, device=DEV)
    rad32 = rad.to(torch.uint32)
    for Q, Rn, D, base, splits in ((0, 6, 48, 0, 1), (ops.KNN_MAX_Q + 1, 6, 48, 0, 1), (4, 0, 48, 0, 1), (4, 6, 0, 0, 1),
                                   (4, 6, 32769, 0, 1), (4, 6, 48, -1, 1), (4, 6, 48, 2 ** 31 - 133, 1),
                                   (4, 2 ** 31 - 127, 48, 0, 1), (4, 6, 48, 0, 0), (4, 6, 48, 0, 1025)):
        with pytest.raises(_lib.HipKernelError):
            _lib.call("edm_u8_ball_count_partial", ops._p(q), ops._p(r), Q, Rn, D, ops._p(rad32), 0, base, splits,
                      ops._p(norms), ops._p(norms[4:]), ops._p(counts), None)
    with pytest.raises(_lib.HipKernelError):
        _lib.call("edm_u8_ball_count_partial", ops._p(q), ops._p(r), 4, 6, 48, None, 0, 0, 1, ops._p(norms), ops._p(norms[4:]),
                  ops._p(counts), None)
    torch.cuda.synchronize()
    ops.check_health(q.device, "after the refusals")


# ------------------------------------------------------------------------------------------------ command line
def test_cli_end_to_end(ops, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(21)
    base = rng.integers(40, 216, (4, 3, 4, 4))

    def draw(n, amp):
        return np.clip(base[rng.integers(0, 4, n)] + rng.integers(-amp, amp + 1, (n, 3, 4, 4)), 0, 255).astype(np.uint8)
    refs, samples, hold = draw(40, 25), draw(30, 40), draw(30, 25)
    for name, x in (("samples", samples), ("refs", refs), ("hold", hold)):
        (tmp_path / name).mkdir()
        for n, a in enumerate(x):
            Image.fromarray(a.transpose(1, 2, 0)).save(tmp_path / name / f"{n}.png")
    report = tmp_path / "prdc.json"
    cmd = [sys.executable, "-m", "tinyedm.prdc", "--image_dir", str(tmp_path / "samples"), "--ref_image_dir",
           str(tmp_path / "refs"), "--holdout_image_dir", str(tmp_path / "hold"), "--k", "1", "3", "--per_sample", "--report",
           str(report)]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(report) as f:
        rep = json.load(f)
    assert rep["k"] == [1, 3] and rep["num_real"] == 40 and rep["num_samples"] == 30 and rep["num_holdout"] == 30
    assert rep["image_shape"] == [3, 4, 4]
    for k in (1, 3):
        got = rep["samples"][str(k)]
        per = got.pop("per_sample")
        assert got == R.prdc(refs, samples, k) and rep["holdout"][str(k)] == R.prdc(refs, hold, k)
        hx, hy, _, _, _ = R.counts(refs, samples, k)
        assert per["hits_x"] == hx.tolist() and per["real_reached"] == (hy > 0).tolist()
    want = R.prdc(refs, samples, 3)
    assert f"{'samples':10s} {'3':>3s} " + " ".join(f"{want[n]:10.4f}" for n in RATIOS) in r.stdout and "holdout" in r.stdout
    # a bad invocation: the message, a non-zero exit, and no traceback
    bad = subprocess.run(cmd[:-2] + ["--k", "30", "--report", str(tmp_path / "no.json")], capture_output=True, text=True,
                         env=env, timeout=600, cwd=ROOT)
    assert bad.returncode != 0 and "needs at least 31 images" in bad.stderr and "Traceback" not in bad.stderr
    assert not (tmp_path / "no.json").exists()
