"""Exact nearest neighbours of uint8 images on the GPU (csrc/neighbors.hip through ops.u8_knn, NearestNeighbors and the
command line): distances AND indices bit for bit against the int64 numpy restatement (tests/neighbors_ref.py), at the smallest
shapes at which each path of the kernel can go wrong.  No tolerance anywhere: the key (d2, index) is total, so the answer
is unique."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import neighbors_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
KS = (1, 5, 32)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as o
    return o


def _eq(got, want):
    (gd, gi), (wd, wi) = got, want
    assert gd.dtype == torch.int64 and gi.dtype == torch.int64
    gd, gi = gd.cpu().numpy(), gi.cpu().numpy()
    assert gd.shape == wd.shape and gi.shape == wi.shape
    assert np.array_equal(gd, wd), f"distances differ at {np.argwhere(gd != wd)[:5].tolist()}"
    assert np.array_equal(gi, wi), f"indices differ at {np.argwhere(gi != wi)[:5].tolist()}"


# ------------------------------------------------------------------------------------------------ shapes
# (Q, R, D, misalign): odd D -> misaligned rows, element path, K tail, partial tiles both ways; MNIST -> 16-byte path with
# D % 64 == 16 and one row past a tile in Q and R; CIFAR -> full tiles; the last -> element path by alignment alone
SHAPES = [(37, 301, 75, 0), (130, 257, 784, 0), (128, 512, 3072, 0), (5, 40, 3072, 1)]
_cases = {}


def _case(shape):
    """(q numpy, r numpy, q device, r device, reference at k = 32): made once per shape; a k-nearest list is a prefix of it"""
    if shape not in _cases:
        Q, Rn, D, off = shape
        rng = np.random.default_rng(Q * 1000 + Rn)
        q = rng.integers(0, 256, (Q, D), dtype=np.uint8)
        r = rng.integers(0, 256, (Rn, D), dtype=np.uint8)
        buf = torch.empty(Q * D + off, dtype=torch.uint8, device=DEV)
        qd = buf[off:].view(Q, D)
        qd.copy_(torch.from_numpy(q))
        assert qd.data_ptr() % 16 == (off if off else 0) and qd.is_contiguous()
        _cases[shape] = (q, r, qd, torch.from_numpy(r).to(DEV), R.knn(q, r, 32))
    return _cases[shape]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes(ops, shape, k):
    q, r, qd, rd, (wd, wi) = _case(shape)
    _eq(ops.u8_knn(qd, rd, k), (wd[:, :k], wi[:, :k]))


def test_rank_4_inputs_are_rows(ops):
    q, r, qd, rd, (wd, wi) = _case(SHAPES[2])
    _eq(ops.u8_knn(qd.view(-1, 3, 32, 32), rd.view(-1, 3, 32, 32), 5), (wd[:, :5], wi[:, :5]))


# ------------------------------------------------------------------------------------------------ range
def test_largest_distance_does_not_wrap(ops):
    D = 32768
    q = np.stack([np.zeros(D, np.uint8), np.full(D, 255, np.uint8)])
    r = np.stack([np.zeros(D, np.uint8), np.full(D, 255, np.uint8), np.full(D, 128, np.uint8)])
    d, i = ops.u8_knn(torch.from_numpy(q).to(DEV), torch.from_numpy(r).to(DEV), 3)
    _eq((d, i), R.knn(q, r, 3))
    d = d.cpu().numpy()
    assert d[0, 0] == 0 and d[1, 0] == 0 and d[0, 2] == 65025 * 32768 == 2130739200 and d[1, 2] == 2130739200
    assert d[0, 1] == 128 * 128 * D and d[1, 1] == 127 * 127 * D


@pytest.mark.parametrize("k", KS)
def test_d_12288(ops, k):
    rng = np.random.default_rng(12288)
    q = rng.integers(0, 256, (9, 12288), dtype=np.uint8)
    r = rng.integers(0, 256, (150, 12288), dtype=np.uint8)
    _eq(ops.u8_knn(torch.from_numpy(q).to(DEV), torch.from_numpy(r).to(DEV), k), R.knn(q, r, k))


# ------------------------------------------------------------------------------------------------ ties
def test_ties_across_tiles_and_splits(ops):
    rng = np.random.default_rng(7)
    base = rng.integers(0, 256, (7, 80), dtype=np.uint8)
    r = base[np.arange(1000) % 7]                       # 143 copies of each image: equal distances in every tile
    q = np.concatenate([base, rng.integers(0, 256, (13, 80), dtype=np.uint8)])
    want = R.knn(q, r, 32)
    assert all((want[0][a] == 0).all() and (np.diff(want[1][a]) == 7).all() for a in range(7))
    qd, rd = torch.from_numpy(q).to(DEV), torch.from_numpy(r).to(DEV)
    for splits in (None, 1, 3, 8):
        _eq(ops.u8_knn(qd, rd, 32, splits=splits), want)


# ------------------------------------------------------------------------------------------------ independence
def test_split_count_does_not_matter(ops):
    q, r, qd, rd, (wd, wi) = _case(SHAPES[1])
    assert ops.u8_knn_splits(130, 257) >= 1
    for k in (5, 32):
        for splits in (1, 2, 3, None, 7):               # 7 > the three reference tiles: empty shares
            _eq(ops.u8_knn(qd, rd, k, splits=splits), (wd[:, :k], wi[:, :k]))


@pytest.mark.parametrize("chunk", [64, 100, None])
def test_reference_chunks_do_not_matter(ops, chunk):
    from tinyedm_amd.neighbors import NearestNeighbors
    q, r, qd, rd, (wd, wi) = _case(SHAPES[1])
    _eq(ops.u8_knn(qd, rd, 32, ref_chunk=7 if chunk is None else chunk + 1), (wd, wi))      # chunks smaller than k
    for k in (5, 32):
        _eq(NearestNeighbors(rd, k=k, ref_chunk=chunk).search(qd), (wd[:, :k], wi[:, :k]))
    _eq(NearestNeighbors(r, k=3, ref_chunk=chunk).search(q), (wd[:, :3], wi[:, :3]))      # numpy in, moved to the device
    _eq(NearestNeighbors(rd, k=32, ref_chunk=chunk).search(qd, k=1), (wd[:, :1], wi[:, :1]))
    _eq(ops.u8_knn(qd, rd, 5, splits=2, ref_chunk=chunk), (wd[:, :5], wi[:, :5]))


# ------------------------------------------------------------------------------------------------ exclude_self
def test_exclude_self(ops):
    from tinyedm_amd.neighbors import NearestNeighbors
    rng = np.random.default_rng(300)
    x = rng.integers(0, 256, (300, 784), dtype=np.uint8)
    x[203] = x[17]                                      # a planted exact duplicate pair
    xd = torch.from_numpy(x).to(DEV)
    d, i = ops.u8_knn(xd, xd, 5)
    _eq((d, i), R.knn(x, x, 5))
    d, i = d.cpu().numpy(), i.cpu().numpy()
    assert (d[:, 0] == 0).all()
    assert all(i[a, 0] == (17 if a == 203 else a) for a in range(300))    # 203's copy at index 17 wins the tie
    want = R.knn(x, x, 5, exclude_self=True)
    for splits in (None, 1, 2):
        got = ops.u8_knn(xd, xd, 5, exclude_self=True, splits=splits)
        _eq(got, want)
    gi, gd = got[1].cpu().numpy(), got[0].cpu().numpy()
    assert all(a not in gi[a] for a in range(300))
    assert (gi[17, 0], gd[17, 0], gi[203, 0], gd[203, 0]) == (203, 0, 17, 0)
    assert (np.delete(gd[:, 0], [17, 203]) > 0).all()
    _eq(NearestNeighbors(xd, k=5, ref_chunk=128).search(xd, exclude_self=True), want)


# ------------------------------------------------------------------------------------------------ planted answers
def test_planted_distances(ops):
    from tinyedm_amd.neighbors import duplicates
    rng = np.random.default_rng(11)
    r = rng.integers(0, 256, (200, 192), dtype=np.uint8)
    src = [3, 150, 77, 199, 0, 128]
    ms = [0, 0, 1, 1, 17, 17]
    q = r[src].copy()
    for a, m in enumerate(ms):
        for p in rng.choice(192, m, replace=False):
            q[a, p] = q[a, p] + 1 if q[a, p] == 0 or (q[a, p] < 255 and rng.integers(2)) else q[a, p] - 1
    d, i = ops.u8_knn(torch.from_numpy(q).to(DEV), torch.from_numpy(r).to(DEV), 5)
    _eq((d, i), R.knn(q, r, 5))
    d, i = d.cpu().numpy(), i.cpu().numpy()
    assert i[:, 0].tolist() == src and d[:, 0].tolist() == ms
    assert duplicates(d, i, 1) == [(0, 3, 0), (1, 150, 0), (2, 77, 1), (3, 199, 1)]


# ------------------------------------------------------------------------------------------------ outputs
def test_outputs_land_in_a_slice_and_nowhere_else(ops):
    q, r, qd, rd, (wd, wi) = _case(SHAPES[0])
    Q, k, pad = q.shape[0], 5, 3
    big_d = torch.full((Q + 2 * pad, k), 0xDEADBEEF, dtype=torch.uint32, device=DEV)
    big_i = torch.full((Q + 2 * pad, k), -77, dtype=torch.int32, device=DEV)
    d, i = ops.u8_knn(qd, rd, k, out=(big_d[pad:pad + Q], big_i[pad:pad + Q]))
    assert d.dtype == torch.uint32 and i.dtype == torch.int32 and d.data_ptr() == big_d[pad].data_ptr()
    bd, bi = big_d.cpu().numpy().astype(np.int64), big_i.cpu().numpy().astype(np.int64)
    assert np.array_equal(bd[pad:pad + Q], wd[:, :k]) and np.array_equal(bi[pad:pad + Q], wi[:, :k])
    for edge in (slice(0, pad), slice(pad + Q, None)):
        assert (bd[edge] == 0xDEADBEEF).all() and (bi[edge] == -77).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ops):
    q = torch.zeros(4, 48, dtype=torch.uint8, device=DEV)
    r = torch.zeros(6, 48, dtype=torch.uint8, device=DEV)
    with pytest.raises(TypeError):
        ops.u8_knn(q.float(), r, 1)
    with pytest.raises(TypeError):
        ops.u8_knn(q, r.float(), 1)
    with pytest.raises(RuntimeError):
        ops.u8_knn(q.cpu(), r, 1)
    with pytest.raises(RuntimeError):
        ops.u8_knn(q, r.cpu(), 1)
    with pytest.raises(ValueError):
        ops.u8_knn(q, torch.zeros(6, 49, dtype=torch.uint8, device=DEV), 1)
    big = torch.zeros(2, 32769, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.u8_knn(big, big, 1)
    for k in (0, 33, 7):                                   # 7 > R = 6
        with pytest.raises(ValueError):
            ops.u8_knn(q, r, k)
    with pytest.raises(ValueError):
        ops.u8_knn(r, r, 6, exclude_self=True)             # k = R with exclude_self
    ops.u8_knn(r, r, 5, exclude_self=True)
    ops.u8_knn(r, r, 6)
    with pytest.raises(ValueError):
        ops.u8_knn(torch.zeros(4, 96, dtype=torch.uint8, device=DEV)[:, ::2], r, 1)
    with pytest.raises(ValueError):
        ops.u8_knn(q, torch.zeros(48, 6, dtype=torch.uint8, device=DEV).t(), 1)
    with pytest.raises(ValueError):
        ops.u8_knn(q, r, 1, splits=0)
    with pytest.raises(ValueError):
        ops.u8_knn(q, r, 1, ref_chunk=0)
    for Q, Rn in ((ops.KNN_MAX_Q + 1, 6), (4, ops.KNN_MAX_R + 1), (4, 2 ** 31 - 1)):   # limits no tensor here can reach
        with pytest.raises(ValueError):
            ops.knn_check(Q, Rn, 48, 1)
    ops.knn_check(ops.KNN_MAX_Q, ops.KNN_MAX_R, 48, 1)
    # the library refuses on its own what ops would not let through to it
    from tinyedm_amd import _lib
    keys = torch.empty(1, 4, 7, dtype=torch.uint64, device=DEV)
    norms = torch.empty(10, dtype=torch.int32, device=DEV)
    for Q, Rn, D, k, excl, base, splits in ((4, 6, 48, 7, 0, 0, 1), (4, 6, 48, 6, 1, 0, 1), (4, 6, 0, 1, 0, 0, 1),
                                           (4, 6, 32769, 1, 0, 0, 1), (4, 6, 48, 0, 0, 0, 1), (4, 6, 48, 33, 0, 0, 1),
                                           (4, 6, 48, 1, 0, 0, 0), (4, 6, 48, 1, 0, 0, 1025), (ops.KNN_MAX_Q + 1, 6, 48, 1, 0, 0, 1),
                                           (4, 2 ** 31 - 127, 48, 1, 0, 0, 1), (4, 6, 48, 1, 0, 2 ** 31 - 133, 1)):
        with pytest.raises(_lib.HipKernelError):
            _lib.call("edm_u8_knn_partial", ops._p(q), ops._p(r), Q, Rn, D, k, excl, base, 0, splits, ops._p(norms),
                      ops._p(norms[4:]), ops._p(keys), None)
    for n_rows, D in ((0, 48), (4, 0), (4, 32769)):
        with pytest.raises(_lib.HipKernelError):
            _lib.call("edm_u8_norms", ops._p(q), n_rows, D, ops._p(norms), None)
    torch.cuda.synchronize()
    ops.check_health(q.device, "after the refusals")


# ------------------------------------------------------------------------------------------------ command line
def test_cli_end_to_end(ops, tmp_path):
    from PIL import Image
    from tinyedm_amd.neighbors import closer_than_holdout, summarize
    rng = np.random.default_rng(21)
    refs = rng.integers(0, 256, (200, 3, 8, 8), dtype=np.uint8)
    samples = rng.integers(0, 256, (20, 3, 8, 8), dtype=np.uint8)
    samples[4] = refs[120]                                  # a copy, and a near copy
    samples[9] = refs[33]
    samples[9, 0, 0, 0] ^= 1
    hold = rng.integers(0, 256, (15, 3, 8, 8), dtype=np.uint8)
    hold[2] = refs[5]
    for name, x in (("samples", samples), ("refs", refs), ("hold", hold)):
        (tmp_path / name).mkdir()
        for n, a in enumerate(x):
            Image.fromarray(a.transpose(1, 2, 0)).save(tmp_path / name / f"{n}.png")
    report, grid = tmp_path / "nn.json", tmp_path / "nn.png"
    cmd = [sys.executable, "-m", "tinyedm.neighbors", "--image_dir", str(tmp_path / "samples"), "--ref_image_dir",
           str(tmp_path / "refs"), "--holdout_image_dir", str(tmp_path / "hold"), "--k", "3", "--max_d2", "1", "--report",
           str(report), "--grid", str(grid), "--grid_rows", "4"]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(report) as f:
        rep = json.load(f)
    wd, wi = R.knn(samples, refs, 3)
    assert rep["k"] == 3 and rep["num_references"] == 200 and rep["num_samples"] == 20 and rep["image_shape"] == [3, 8, 8]
    assert [[n["index"] for n in row] for row in rep["neighbours"]] == wi.tolist()
    assert [[n["d2"] for n in row] for row in rep["neighbours"]] == wd.tolist()
    assert rep["neighbours"][9][0]["rms"] == pytest.approx(float(R.rms(1, 192)), rel=1e-12)
    hd = R.knn(hold, refs, 1)[0][:, 0]
    assert rep["nearest"] == summarize(wd[:, 0]) and rep["holdout_nearest"] == summarize(hd) and rep["num_holdout"] == 15
    assert rep["closer_than_holdout"] == closer_than_holdout(wd[:, 0], hd) == R.closer_than_holdout(wd[:, 0], hd)
    assert [(e["sample"], e["index"], e["d2"]) for e in rep["at_or_under_max_d2"]] == [(4, 120, 0), (9, 33, 1)]
    with Image.open(grid) as im:
        assert im.size == ((3 + 1) * 8, 4 * 8) and im.mode == "RGB"
        top = np.asarray(im)[:8]
    assert np.array_equal(top[:, :8], samples[4].transpose(1, 2, 0)) and np.array_equal(top[:, 8:16], refs[120].transpose(1, 2, 0))
    # --self: the reference set against itself
    refs2 = tmp_path / "refs2"
    refs2.mkdir()
    dup = refs[:30].copy()
    dup[22] = dup[6]
    for n, a in enumerate(dup):
        Image.fromarray(a.transpose(1, 2, 0)).save(refs2 / f"{n}.png")
    cmd = [sys.executable, "-m", "tinyedm.neighbors", "--self", "--ref_image_dir", str(refs2), "--k", "2", "--report", str(report)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(report) as f:
        rep = json.load(f)
    assert [(p["i"], p["j"], p["d2"]) for p in rep["duplicate_pairs"]] == [(6, 22, 0)]
    assert rep["nearest"] == summarize(R.knn(dup, dup, 1, exclude_self=True)[0][:, 0])
