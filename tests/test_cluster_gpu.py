"""Feature clustering on the GPU (csrc/kmeans.hip through ops.f32_cluster_sums, lloyd_step, kmeans_plus_plus, KMeans, the
command line and the datamodules' label files) against the numpy restatement (tests/cluster_ref.py).

ops.f32_cluster_sums is compared BIT FOR BIT on arbitrary finite inputs: the restatement performs the same IEEE fp64
additions in the stated order, so there is no tolerance.  Three kinds of input: normal float32 data, dyadic data (exact in
any order) and data spread over 60 binades (cluster_ref.wide), the one on which nearly every addition rounds -- sums of a
few thousand float32 values of one magnitude are exact in fp64 and would not notice a wrong order.

lloyd_step trajectories: the restatement assigns by the direct distance form and first asserts, on its own numbers, that
every row's nearest and second-nearest centroid are farther apart than f32_knn's float-tier bound (tests/test_fknn_gpu.py:
2 (D + 2) 2^-53 (|q| + |r|)^2) and that no cluster runs empty; the labels must then agree, and with equal labels the
centroid and count bits are a consequence of the order rule.  The distance bits are those of f32_knn (checked against the
direct form within that bound); the cluster inertia is the restatement's ordered sum of the device's distance vector, bit
for bit.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cluster_ref as C
import fknn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
B = C.BLOCK


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as o
    assert o.cluster_block() == B
    return o


@pytest.fixture(scope="module")
def cluster(ops):
    from tinyedm_amd import cluster as c
    return c


def _dev(x, off=0):
    """x on the device, contiguous; off: floats past a 16-byte boundary at which the rows start"""
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


def _same_sums(got, want, what=""):
    (gs, gc, gd), (ws, wc, wd) = got, want
    assert gs.dtype == torch.float64 and gc.dtype == torch.int64 and tuple(gs.shape) == ws.shape
    assert np.array_equal(gc.cpu().numpy(), wc), f"{what}: counts differ"
    g = gs.cpu().numpy()
    assert np.array_equal(_bits(g), _bits(ws)), f"{what}: sums differ at {np.argwhere(_bits(g) != _bits(ws))[:4].tolist()}"
    assert (gd is None) == (wd is None)
    if wd is not None:
        assert gd.dtype == torch.float64 and np.array_equal(_bits(gd.cpu().numpy()), _bits(wd)), f"{what}: d2sums differ"


def _one_big(n, K=4, k=2):
    """labels with all n rows in cluster k of K, the others empty"""
    return np.full(n, k, np.int64)


def _data(kind, seed, n, D):
    if kind == "normal":
        return np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)
    return R.dyadic(seed, n, D) if kind == "dyadic" else C.wide(seed, n, D)


def _skewed(n, K, seed):
    """one cluster holds half the rows, the rest are spread over the others; scrambled order"""
    r = np.random.default_rng(seed)
    labels = np.where(np.arange(n) < (n + 1) // 2, 1, r.integers(0, K, n))
    return r.permutation(labels).astype(np.int64)


# (n, D, K, labels): the kernel's seams, with B = EDM_CLUSTER_BLOCK
def _shapes():
    r = np.random.default_rng(0)
    s = [(1, 1, 1, np.zeros(1, np.int64)),
         (5, 3, 5, r.permutation(5).astype(np.int64)),                     # every row its own cluster
         (7, 3, 9, np.array([8, 0, 3, 3, 8, 1, 0], np.int64))]            # K > n, empty clusters
    s += [(m, 8, 4, _one_big(m)) for m in (B - 1, B, B + 1, 3 * B + 1)]    # chunk seams, the other clusters empty
    s += [(150, D, 6, r.integers(0, 6, 150)) for D in (1, 3, 4, 67, 300)]  # element path, vector path, a second column block
    s += [(2051, 12, 7, _skewed(2051, 7, 1))]                              # one cluster at half the rows
    return s


SHAPES = _shapes()


@pytest.mark.parametrize("kind", ["normal", "dyadic", "wide"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[f"n{s[0]}-D{s[1]}-K{s[2]}" for s in SHAPES])
def test_cluster_sums_bit_for_bit(ops, i, kind):
    n, D, K, labels = SHAPES[i]
    x = _data(kind, 100 + i, n, D)
    d2 = np.abs(_data(kind, 200 + i, n, 1)[:, 0]).astype(np.float64) * (1.0 + 2.0 ** -40)     # fp64 values, not float32 ones
    want = C.cluster_sums(x, labels, K, d2)
    got = ops.f32_cluster_sums(_dev(x), torch.from_numpy(labels).to(DEV), K, _dev(d2))
    _same_sums(got, want, f"{kind} {(n, D, K)}")
    if kind == "dyadic":
        exact = np.zeros((K, D))
        np.add.at(exact, labels, x.astype(np.float64))
        assert np.array_equal(got[0].cpu().numpy(), exact)
    empty = np.flatnonzero(want[1] == 0)
    g = got[0].cpu().numpy()
    assert not g[empty].any() and not np.signbit(g[empty]).any(), "an empty cluster is +0.0"
    # without the distance vector: the same sums, no third result
    s2, c2, none = ops.f32_cluster_sums(_dev(x), torch.from_numpy(labels).to(DEV), K)
    assert none is None and torch.equal(c2, got[1]) and np.array_equal(_bits(s2.cpu().numpy()), _bits(want[0]))


def test_cluster_sums_wider_rows_and_nd_input(ops):
    """D = 2048 (eight column blocks) and an input of rank 4 taken as [n, D]"""
    x = C.wide(7, 70, 2048)
    labels = np.random.default_rng(7).integers(0, 3, 70)
    _same_sums(ops.f32_cluster_sums(_dev(x).view(70, 2, 32, 32), torch.from_numpy(labels).to(DEV), 3),
               C.cluster_sums(x, labels, 3), "D = 2048")


def test_cluster_sums_element_path_by_alignment(ops):
    """D = 64 with the set 4 bytes off a 16-byte boundary: the element loads, with the bits of the aligned copy"""
    n, D, K = 3 * B + 5, 64, 5
    x = C.wide(3, n, D)
    labels = _skewed(n, K, 3)
    lab = torch.from_numpy(labels).to(DEV)
    d2 = _dev(np.abs(C.wide(4, n, 1)[:, 0]).astype(np.float64))
    off = ops.f32_cluster_sums(_dev(x, off=1), lab, K, d2)
    aligned = ops.f32_cluster_sums(_dev(x), lab, K, d2)
    _same_sums(off, C.cluster_sums(x, labels, K, d2.cpu().numpy()), "4 bytes off")
    assert torch.equal(off[0].view(torch.int64), aligned[0].view(torch.int64))
    assert torch.equal(off[2].view(torch.int64), aligned[2].view(torch.int64))


def test_cluster_sums_do_not_depend_on_K_or_the_run(ops):
    n, D, K = 1000, 20, 6
    x, labels = _dev(C.wide(9, n, D)), torch.from_numpy(_skewed(n, 6, 9)).to(DEV)
    d2 = _dev(np.abs(C.wide(10, n, 1)[:, 0]).astype(np.float64))
    a = ops.f32_cluster_sums(x, labels, K, d2)
    b = ops.f32_cluster_sums(x, labels, K, d2)
    c = ops.f32_cluster_sums(x, labels, K + 37, d2)
    for i in (0, 2):
        assert torch.equal(a[i].view(torch.int64), b[i].view(torch.int64)), "two calls, the same bits"
        assert torch.equal(a[i].view(torch.int64), c[i][:K].view(torch.int64)), "K enlarged: the old clusters keep their bits"
    assert torch.equal(a[1], c[1][:K]) and not bool(c[1][K:].any()) and not bool(c[0][K:].any())


def test_cluster_sums_refusals(ops):
    x = torch.zeros(4, 3, device=DEV)
    lab = torch.tensor([0, 1, 1, 0], device=DEV)
    d64 = torch.zeros(4, device=DEV, dtype=torch.float64)
    good = np.array([2, 2], np.int64)
    for error, bad in (
            (TypeError, lambda: ops.f32_cluster_sums(x.double(), lab, 2)),
            (TypeError, lambda: ops.f32_cluster_sums(x.cpu().numpy(), lab, 2)),
            (RuntimeError, lambda: ops.f32_cluster_sums(x.cpu(), lab.cpu(), 2)),      # _chk's "no CPU path", as in f32_knn
            (ValueError, lambda: ops.f32_cluster_sums(x, lab, 0)),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab, True)),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab, 2.0)),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab, ops.CLUSTER_MAX_K + 1)),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab, 1)),                    # a label out of range
            (ValueError, lambda: ops.f32_cluster_sums(x, lab - 1, 2)),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab[:3], 2)),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab.int(), 2)),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab.cpu(), 2)),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab.view(2, 2), 2)),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab, 2, d64.float())),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab, 2, d64[:3])),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab, 2, d64.cpu())),
            (ValueError, lambda: ops.f32_cluster_sums(x.t(), lab[:3], 2)),            # not contiguous
            (ValueError, lambda: ops.f32_cluster_sums(x, lab, 2, counts=[2, 2])),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab, 2, counts=good[:1])),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab, 2, counts=np.array([3, 2], np.int64))),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab, 2, counts=np.array([5, -1], np.int64))),
            (ValueError, lambda: ops.f32_cluster_sums(x, lab.int(), 2, counts=good))):
        with pytest.raises(error) as info:
            bad()
        assert type(info.value) is error, "the wrapper's own refusal, not a subclass raised further down"
    a = ops.f32_cluster_sums(x + 1.0, lab, 2, d64 + 1.0)
    b = ops.f32_cluster_sums(x + 1.0, lab, 2, d64 + 1.0, counts=good)       # the caller's counts: the same results
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and b[1].tolist() == [2, 2]


# ------------------------------------------------------------------------------------------------ Lloyd trajectories
@pytest.mark.parametrize("case", C.LLOYD_CASES)
def test_lloyd_trajectory(cluster, case):
    x, init = C.lloyd_inputs(*case)
    want = C.lloyd(x, init, require_gap=True)                  # asserts the gap and the occupancy on its own numbers
    xd, c = _dev(x), _dev(init)
    for it, (labels, d2, new, counts, _) in enumerate(want):
        gl, gd2, gnew, gcounts, ginertia = cluster.lloyd_step(xd, c)
        assert gl.dtype == torch.int64 and gd2.dtype == torch.float64 and gnew.dtype == torch.float32
        assert np.array_equal(gl.cpu().numpy(), labels), f"step {it}: labels"
        assert np.array_equal(gcounts.cpu().numpy(), counts), f"step {it}: counts"
        assert np.array_equal(gnew.cpu().numpy().view(np.uint32), new.view(np.uint32)), f"step {it}: centroid bits"
        dev_d2 = gd2.cpu().numpy()
        bound = C.gap_bound(x, c.cpu().numpy())[np.arange(len(x)), labels]
        assert (np.abs(dev_d2 - d2) <= bound).all(), f"step {it}: distances"
        inertia = C.cluster_sums(x, labels, len(init), dev_d2)[2]
        assert np.array_equal(_bits(ginertia.cpu().numpy()), _bits(inertia)), f"step {it}: inertia bits"
        c = gnew
    assert np.array_equal(want[-1][0], want[-2][0]), "the reference reached its fixed point"


# ------------------------------------------------------------------------------------------------ empty clusters
def test_duplicate_init_row_runs_empty_and_is_refilled(cluster):
    x, init = C.lloyd_inputs(400, 5, 4, 11)
    init = init.copy()
    init[3] = init[1]                                          # ties go to cluster 1: cluster 3 is empty at step 1
    d = R.dist_matrix(x, init)
    assert (np.argmin(d, 1) != 3).all()
    two = np.partition(d[:, :3], 1, axis=1)[:, :2]             # the three distinct centroids are told apart safely
    assert ((two[:, 1] - two[:, 0]) > C.gap_bound(x, init).max(1)).all()
    labels, d2, new, counts, inertia, left = C.lloyd_step(x, init)
    assert left == [] and counts[3] == 1
    gl, gd2, gnew, gcounts, ginertia = cluster.lloyd_step(_dev(x), _dev(init))
    assert np.array_equal(gl.cpu().numpy(), labels) and np.array_equal(gcounts.cpu().numpy(), counts)
    assert np.array_equal(gnew.cpu().numpy().view(np.uint32), new.view(np.uint32))
    moved = int(np.flatnonzero(labels == 3)[0])
    assert float(gd2[moved]) == 0.0 and np.array_equal(gnew[3].cpu().numpy(), x[moved])


def test_more_clusters_than_distinct_rows(cluster):
    base = R.dyadic(4, 3, 6)
    x = _dev(base[np.random.default_rng(4).integers(0, 3, 40)])
    km = cluster.KMeans(5, n_init=2, seed=1).fit(x)
    assert len(km.empty_clusters) == 2 and km.converged and km.inertia == 0.0
    assert int((km.counts == 0).sum()) == 2 and int(km.counts.sum()) == 40
    assert torch.equal(km.predict(x)[0], km.labels_)


# ------------------------------------------------------------------------------------------------ seeding
def test_kmeans_plus_plus(cluster):
    x = C.lloyd_inputs(500, 9, 1, 21)[0]
    xd = _dev(x)
    a = cluster.kmeans_plus_plus(xd, 12, 3)
    assert a.dtype == np.int64 and a.shape == (12,) and len(set(a.tolist())) == 12 and a.min() >= 0 and a.max() < 500
    assert np.array_equal(a, cluster.kmeans_plus_plus(xd, 12, 3))
    assert not np.array_equal(a, cluster.kmeans_plus_plus(xd, 12, 4))
    # duplicated rows: 10 distinct rows, 30 copies each; 10 draws never take two copies of one row
    base = R.dyadic(6, 10, 7)
    assert len({r.tobytes() for r in base}) == 10
    rep = base[np.random.default_rng(6).permutation(np.repeat(np.arange(10), 30))]
    got = cluster.kmeans_plus_plus(_dev(rep), 10, 0)
    assert len({rep[i].tobytes() for i in got}) == 10
    # every remaining row a duplicate: the lowest unchosen row
    more = cluster.kmeans_plus_plus(_dev(rep), 12, 0)
    assert np.array_equal(more[:10], got) and more[10] == min(set(range(300)) - set(got.tolist()))
    # dyadic rows: exact distances, so the draws are the restatement's
    dy = R.dyadic(8, 257, 11)
    for seed in (0, 1, 2):
        assert np.array_equal(cluster.kmeans_plus_plus(_dev(dy), 9, seed), C.kmeans_plus_plus(dy, 9, seed))
    with pytest.raises(ValueError):
        cluster.kmeans_plus_plus(xd, 501, 0)


# ------------------------------------------------------------------------------------------------ KMeans end to end
@pytest.fixture(scope="module")
def planted_fit(cluster):
    x, y = C.planted()
    best = None
    for seed in range(4):                                      # the restatement finds the planted partition first
        traj = C.lloyd(x, x[C.kmeans_plus_plus(x, 6, seed)])
        inertia = C.host_sum(traj[-1][4])
        if best is None or inertia < best[0]:
            best = (inertia, traj[-1][0])
    assert C.same_partition(best[1], y)
    xd = _dev(x)
    return x, y, xd, cluster.KMeans(6, n_init=4).fit(xd)


def test_kmeans_planted_mixture(cluster, planted_fit):
    x, y, xd, km = planted_fit
    labels = km.labels_.cpu().numpy()
    assert C.same_partition(labels, y) and km.converged and km.empty_clusters == []
    assert km.counts.tolist() == [100] * 6 and km.centroids.dtype == torch.float32 and tuple(km.centroids.shape) == (6, 16)
    pl, pd2 = km.predict(xd)
    assert torch.equal(pl, km.labels_)
    assert km.inertia == C.host_sum(km.cluster_inertia.cpu().numpy()) == km.inertia_history[-1]
    assert len(km.inertia_history) == km.n_iter and all(b <= a for a, b in zip(km.inertia_history, km.inertia_history[1:]))
    direct = float(((x.astype(np.float64) - km.centroids.cpu().numpy().astype(np.float64)[labels]) ** 2).sum())
    assert abs(km.inertia - direct) <= 1e-9 * direct
    again = cluster.KMeans(6, n_init=4).fit(xd)                # fit twice: the same bits
    assert torch.equal(again.centroids.view(torch.int32), km.centroids.view(torch.int32))
    assert torch.equal(again.labels_, km.labels_) and again.inertia == km.inertia and again.n_iter == km.n_iter
    assert torch.equal(again.cluster_inertia.view(torch.int64), km.cluster_inertia.view(torch.int64))


def test_kmeans_n_init_keeps_the_least_inertia(cluster):
    x = _dev(C.lloyd_inputs(600, 6, 1, 31)[0])
    singles = [cluster.KMeans(8, seed=s).fit(x) for s in range(3)]
    inertias = [s.inertia for s in singles]
    assert len(set(inertias)) > 1, "the seedings end in different optima on this set"
    km = cluster.KMeans(8, n_init=3).fit(x)
    win = singles[int(np.argmin(inertias))]                     # argmin: ties to the earlier run
    assert km.inertia == min(inertias) and torch.equal(km.centroids.view(torch.int32), win.centroids.view(torch.int32))


def test_kmeans_normalize_and_given_init(cluster, planted_fit):
    from tinyedm_amd.features import _unit_rows
    x, y, xd, _ = planted_fit
    a = cluster.KMeans(6, n_init=2, normalize=True).fit(xd)
    b = cluster.KMeans(6, n_init=2).fit(_unit_rows(xd))
    assert torch.equal(a.centroids.view(torch.int32), b.centroids.view(torch.int32)) and torch.equal(a.labels_, b.labels_)
    assert a.inertia == b.inertia and torch.equal(a.predict(xd)[0], a.labels_)
    init = xd[torch.from_numpy(C.kmeans_plus_plus(x, 6, 0)).to(DEV)].contiguous()
    g = cluster.KMeans(6, init=init).fit(xd)
    want = C.lloyd(x, init.cpu().numpy())
    assert np.array_equal(g.labels_.cpu().numpy(), want[-1][0]) and g.n_iter == len(want)
    raw = cluster.KMeans(6, init=init, normalize=True).fit(xd)  # a given init is normalised like the rows
    unit = cluster.KMeans(6, init=_unit_rows(init)).fit(_unit_rows(xd))
    assert torch.equal(raw.centroids.view(torch.int32), unit.centroids.view(torch.int32)) and raw.n_iter == unit.n_iter
    short = cluster.KMeans(6, init=init, max_iter=1).fit(xd)    # stopped early: the attributes still describe the centroids
    assert not short.converged and short.n_iter == 1 and torch.equal(short.predict(xd)[0], short.labels_)
    with pytest.raises(ValueError, match="non-finite"):
        cluster.KMeans(2).fit(torch.full((4, 2), float("nan"), device=DEV))
    with pytest.raises(ValueError, match="at least that many rows"):
        cluster.KMeans(9).fit(xd[:5])


def _run(module, argv):
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    return subprocess.run([sys.executable, "-m", module, *argv], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)


def test_command_line_round_trip(cluster, planted_fit, tmp_path):
    """fit on a training set, assign samples that miss one blob, and hand both label lists to prdc as they are"""
    x, y, _, km = planted_fit
    train, samples = x[:480], x[480:][y[480:] != 0]
    t, s, c, tl, sl = (str(tmp_path / n) for n in ("train.npy", "samples.npy", "clusters.npz", "train.json", "drawn.json"))
    np.save(t, train)
    np.save(s, samples)
    r = _run("tinyedm.cluster", ["--fit", "--features", t, "--k", "6", "--n_init", "4", "--out", c, "--labels_out", tl])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "inertia" in r.stdout
    train_labels = json.load(open(tl))
    assert len(train_labels) == 480 and C.same_partition(train_labels, y[:480])
    rep = str(tmp_path / "modes.json")
    r = _run("tinyedm.cluster", ["--clusters", c, "--features", s, "--ref_features", t, "--holdout_features", t,
                                 "--labels_out", sl, "--report", rep])
    assert r.returncode == 0, r.stderr[-2000:]
    report = json.load(open(rep))
    gone = train_labels[int(np.flatnonzero(y[:480] == 0)[0])]
    assert report["samples"]["missing"] == [gone] and abs(report["samples"]["coverage"] - 5 / 6) < 1e-12
    assert report["holdout"]["total_variation"] == 0.0 and report["holdout"]["coverage"] == 1.0
    assert "coverage" in r.stdout
    drawn = json.load(open(sl))
    assert len(drawn) == len(samples) and gone not in drawn
    out = str(tmp_path / "prdc.json")
    r = _run("tinyedm.prdc", ["--features", s, "--ref_features", t, "--labels_json", sl, "--ref_labels", tl, "--k", "3",
                              "--report", out])
    assert r.returncode == 0, r.stderr[-2000:]
    per = json.load(open(out))["samples"]["3"]["per_class"]
    assert set(per) == {str(k) for k in range(6)} and "skipped" in per[str(gone)]


# ------------------------------------------------------------------------------------------------ datamodule
def test_datamodule_reads_label_files(ops, tmp_path):
    from oracle import data_oracle as DO
    from tinyedm_amd import datamodules as DM
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (48, 3, 32, 32), dtype=np.uint8)
    lab = rng.integers(0, 10, 48)
    DO.write_cifar10_batches(str(tmp_path), img, lab, n_train=40)
    pseudo, val = rng.integers(0, 23, 40), rng.integers(0, 23, 8)
    (tmp_path / "train.json").write_text(json.dumps(pseudo.tolist()))
    np.save(tmp_path / "val.npy", val)
    dm = DM.CIFAR10DataModule(str(tmp_path), 32, batch_size=16, device=DEV, labels_path=str(tmp_path / "train.json"),
                              val_labels_path=str(tmp_path / "val.npy"), label_classes=23)
    assert dm.num_classes == 23
    dm.setup("fit")
    seen = 0
    for x, y in dm.train_dataloader():
        u8 = dm.denormalize(x).cpu().numpy()
        for i in range(u8.shape[0]):
            cand = [j for j in range(40) if np.array_equal(u8[i], img[j]) or np.array_equal(u8[i], img[j][:, :, ::-1])]
            assert cand and int(y[i]) == int(pseudo[cand[0]]), "a batch carries the file's label of its image"
            seen += 1
    assert seen == 40
    got = torch.cat([y for _, y in dm.val_dataloader()]).cpu().numpy()
    assert np.array_equal(got, val)
    dm.setup("test")
    assert np.array_equal(torch.cat([y for _, y in dm.test_dataloader()]).cpu().numpy(), val)
    (tmp_path / "short.json").write_text(json.dumps(pseudo[:39].tolist()))
    bad = DM.CIFAR10DataModule(str(tmp_path), 32, batch_size=16, device=DEV, labels_path=str(tmp_path / "short.json"),
                               val_labels_path=str(tmp_path / "val.npy"), label_classes=23)
    with pytest.raises(ValueError, match="39 labels"):
        bad.setup("fit")
    low = DM.CIFAR10DataModule(str(tmp_path), 32, batch_size=16, device=DEV, labels_path=str(tmp_path / "train.json"),
                               val_labels_path=str(tmp_path / "val.npy"), label_classes=int(pseudo.max()))
    with pytest.raises(ValueError, match="must lie in"):
        low.setup("fit")
