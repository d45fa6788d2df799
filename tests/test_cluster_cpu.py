"""Feature clustering without a GPU: the numpy restatement (tests/cluster_ref.py) against exact arithmetic and against
itself, the host-side rules of tinyedm_amd/cluster.py against the restatement, mode_report against hand-computed cases, and
the refusals of read_label_file and check_args."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_ref as C
import fknn_ref as R
from tinyedm_amd import _lib, cluster
from tinyedm_amd.datamodules import AbstractDataModule, read_label_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n,D,K,block", [(1, 1, 1, None), (7, 3, 9, None), (300, 5, 4, None), (300, 5, 4, 7), (131, 2, 3, 1)])
def test_ref_cluster_sums_exact_on_dyadic(n, D, K, block):
    """dyadic rows sum exactly in any order: the chunked order equals np.add.at, whatever the chunk length"""
    x = R.dyadic(11 + n, n, D)
    r = np.random.default_rng(n)
    labels = r.integers(0, K, n)
    d2 = r.integers(0, 64, n) / 8.0
    sums, counts, d2sums = C.cluster_sums(x, labels, K, d2, block=block)
    want = np.zeros((K, D))
    np.add.at(want, labels, x.astype(np.float64))
    wd = np.zeros(K)
    np.add.at(wd, labels, d2)
    assert np.array_equal(sums, want) and np.array_equal(d2sums, wd)
    assert np.array_equal(counts, np.bincount(labels, minlength=K))
    assert not np.signbit(sums[sums == 0]).any(), "an empty or cancelling cluster is +0.0"


def test_ref_cluster_sums_order_is_the_stated_one():
    """on float data the chunk length enters the bits (so the order is a real contract) and a cluster's sum does not
    depend on K or on the other clusters"""
    x = C.wide(5, 400, 3)
    labels = np.random.default_rng(5).integers(0, 3, 400)
    a = C.cluster_sums(x, labels, 3, block=64)[0]
    b = C.cluster_sums(x, labels, 3, block=400)[0]
    assert not np.array_equal(_bits(a), _bits(b))
    assert np.allclose(a, b, rtol=1e-9, atol=np.abs(x).max() * 1e-12)
    other = labels.copy()
    other[labels == 2] = 5
    c = C.cluster_sums(x, other, 8, block=64)[0]
    assert np.array_equal(_bits(c[:2]), _bits(a[:2])) and np.array_equal(_bits(c[5]), _bits(a[2]))


@pytest.mark.parametrize("case", C.LLOYD_CASES)
def test_ref_lloyd_decreases_and_reaches_a_fixed_point(case):
    x, init = C.lloyd_inputs(*case)
    traj = C.lloyd(x, init, require_gap=True)
    assert len(traj) < 100 and np.array_equal(traj[-1][0], traj[-2][0])
    inertia = [C.host_sum(t[4]) for t in traj]
    assert all(b <= a for a, b in zip(inertia, inertia[1:]))
    assert np.array_equal(traj[-1][2].view(np.uint32), traj[-2][2].view(np.uint32)), "same members, same centroid bits"
    assert traj[-1][3].min() >= 32


def test_ref_planted_mixture_is_recovered():
    x, y = C.planted()
    best = None
    for seed in range(4):
        traj = C.lloyd(x, x[C.kmeans_plus_plus(x, 6, seed)])
        inertia = C.host_sum(traj[-1][4])
        if best is None or inertia < best[0]:
            best = (inertia, traj[-1][0])
    assert C.same_partition(best[1], y)


# ------------------------------------------------------------------------------------------------ host-side rules
def test_fill_empty_clusters_matches_the_restatement():
    r = np.random.default_rng(3)
    for trial in range(40):
        n, K = int(r.integers(1, 30)), int(r.integers(1, 12))
        labels = r.integers(0, max(1, K // 2), n).astype(np.int64)
        d2 = (r.integers(0, 4, n) / 2.0).astype(np.float64)       # many ties and zeros
        la, da, lb, db = labels.copy(), d2.copy(), labels.copy(), d2.copy()
        assert cluster.fill_empty_clusters(la, da, K) == C.fill_empty(lb, db, K), trial
        assert np.array_equal(la, lb) and np.array_equal(da, db), trial


def test_fill_empty_clusters_by_hand():
    labels, d2 = np.array([0, 0, 0, 2, 2], np.int64), np.array([1.0, 4.0, 4.0, 9.0, 0.5])
    left = cluster.fill_empty_clusters(labels, d2, 5)
    # cluster 1 takes row 3 (largest d2; cluster 2 keeps row 4); cluster 3 takes row 1 (4.0, ties to the lower row);
    # cluster 4 takes row 2 (cluster 0 keeps row 0)
    assert left == [] and labels.tolist() == [0, 3, 4, 1, 2] and d2.tolist() == [1.0, 0.0, 0.0, 0.0, 0.5]
    labels, d2 = np.array([0, 0, 1], np.int64), np.array([0.0, 0.0, 0.0])
    assert cluster.fill_empty_clusters(labels, d2, 4) == [2, 3] and labels.tolist() == [0, 0, 1]
    labels, d2 = np.array([0, 1], np.int64), np.array([3.0, 2.0])
    assert cluster.fill_empty_clusters(labels, d2, 3) == [2], "a row that is its cluster's last member stays"


def test_draw_d2_matches_the_restatement():
    r = np.random.default_rng(9)
    for trial in range(200):
        w = r.integers(0, 5, int(r.integers(1, 20))) / 4.0
        u = float(r.random())
        got = cluster.draw_d2(w, u)
        assert got == C.draw(w, u)
        assert got is None or w[got] > 0
    assert cluster.draw_d2([0.0, 0.0], 0.3) is None
    assert cluster.draw_d2([0.0, 1.0, 0.0], 1.0 - 2.0 ** -53) == 1
    assert cluster.draw_d2([1.0, 1.0], 0.5) == 1 and cluster.draw_d2([1.0, 1.0], 0.49) == 0, "exceeds, not reaches"


# ------------------------------------------------------------------------------------------------ mode_report
def _close(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_close(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(_close(p, q) for p, q in zip(a, b))
    if isinstance(a, float) or isinstance(b, float):
        return math.isclose(a, b, rel_tol=1e-12, abs_tol=1e-15)
    return a == b


def test_mode_report_by_hand():
    same = cluster.mode_report([10, 30, 60], [1, 3, 6])["samples"]
    assert same["coverage"] == 1.0 and same["missing"] == [] and same["chi2"] == 0.0
    assert abs(same["total_variation"]) < 1e-15 and abs(same["js_divergence"]) < 1e-15
    assert all(abs(r - 1.0) < 1e-12 for r in same["ratio"])

    miss = cluster.mode_report([2, 2], [4, 0])["samples"]
    assert miss["missing"] == [1] and miss["coverage"] == 0.5 and miss["total_variation"] == 0.5 and miss["chi2"] == 4.0
    js = 0.5 * (0.5 * math.log(0.5 / 0.75) + 0.5 * math.log(0.5 / 0.25)) + 0.5 * math.log(1.0 / 0.75)
    assert math.isclose(miss["js_divergence"], js, rel_tol=1e-14)
    assert miss["ratio"] == [2.0, 0.0] and miss["share"] == [1.0, 0.0]

    # a cluster the references leave empty: not occupied, never missing, its samples counted apart
    rep = cluster.mode_report([3, 0, 1], [2, 1, 1], holdout_counts=[3, 0, 1])
    assert rep["occupied"] == 2 and rep["clusters"] == 3 and rep["n_ref"] == 4
    s = rep["samples"]
    assert s["ratio"][1] is None and s["missing"] == [] and s["coverage"] == 1.0 and s["outside_reference"] == 1
    assert math.isclose(s["total_variation"], 0.5 * (0.25 + 0.25 + 0.0))
    assert math.isclose(s["chi2"], (2 - 3.0) ** 2 / 3.0 + 0.0)
    h = rep["holdout"]
    assert h["coverage"] == 1.0 and h["chi2"] == 0.0 and abs(h["js_divergence"]) < 1e-15


def test_mode_report_matches_the_restatement_and_refuses():
    r = np.random.default_rng(2)
    for _ in range(20):
        K = int(r.integers(1, 9))
        ref, smp, hold = r.integers(0, 6, K), r.integers(0, 6, K), r.integers(0, 6, K)
        if ref.sum() == 0 or smp.sum() == 0 or hold.sum() == 0:
            continue
        assert _close(cluster.mode_report(ref, smp, hold), C.mode_report(ref, smp, hold))
    json.dumps(cluster.mode_report([1, 0], [1, 1]))
    assert "cluster" in cluster.format_table(cluster.mode_report([1, 0], [1, 1], [2, 0]))
    for bad in ([[1, 2], [1]], [[1, 2], [1.0, 2.0]], [[0, 0], [1, 1]], [[1, 1], [0, 0]], [[1, -1], [1, 1]], [[], []]):
        with pytest.raises(ValueError):
            cluster.mode_report(*bad)


# ------------------------------------------------------------------------------------------------ label files
def test_read_label_file(tmp_path):
    p = tmp_path / "l.json"
    p.write_text(json.dumps([0, 3, 2, 3]))
    got = read_label_file(str(p), 4, 4)
    assert got.dtype == np.int64 and got.tolist() == [0, 3, 2, 3]
    q = tmp_path / "l.npy"
    np.save(q, np.array([1, 0, 1], np.int32))
    assert read_label_file(str(q), 3, 2).tolist() == [1, 0, 1]
    with pytest.raises(ValueError, match="4 labels"):
        read_label_file(str(p), 5, 4)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        read_label_file(str(p), 4, 3)
    for text in ('{"a": 1}', "[0, 1.5]", "[0, true]", "[[0], [1]]"):
        p.write_text(text)
        with pytest.raises(ValueError):
            read_label_file(str(p), 2, 4)
    p.write_text("[0, -1]")
    with pytest.raises(ValueError):
        read_label_file(str(p), 2, 4)
    np.save(q, np.array([0.0, 1.0]))
    with pytest.raises(ValueError):
        read_label_file(str(q), 2, 4)


def test_datamodule_label_arguments_go_together():
    dm = AbstractDataModule("nowhere", 4)
    assert dm.labels_path is None and dm.label_classes is None
    for kw in ({"labels_path": "a.json"}, {"labels_path": "a.json", "val_labels_path": "b.json"},
               {"label_classes": 5}, {"labels_path": "a.json", "label_classes": 5}):
        with pytest.raises(ValueError, match="go together"):
            AbstractDataModule("nowhere", 4, **kw)
    with pytest.raises(ValueError, match="label_classes"):
        AbstractDataModule("nowhere", 4, labels_path="a", val_labels_path="b", label_classes=0)
    from tinyedm_amd.datamodules import CIFAR10DataModule, MNISTDataModule
    assert CIFAR10DataModule(labels_path="a", val_labels_path="b", label_classes=100).num_classes == 100
    assert MNISTDataModule(4, labels_path="a", val_labels_path="b", label_classes=7).num_classes == 7
    assert CIFAR10DataModule().num_classes == 10 and MNISTDataModule(4).num_classes == 10


# ------------------------------------------------------------------------------------------------ command line
def _args(*argv):
    return cluster.build_parser().parse_args(list(argv))


def test_check_args():
    cluster.check_args(_args("--fit", "--features", "a.npy", "--k", "10", "--out", "c.npz"))
    cluster.check_args(_args("--fit", "--features", "a.npy", "--k", "10", "20", "--out", "c.npz", "--labels_out", "l.json",
                             "--n_init", "4", "--normalize", "--seed", "3", "--tol", "0.001", "--max_iter", "5"))
    cluster.check_args(_args("--clusters", "c.npz", "--features", "s.npy", "--ref_features", "t.npy", "--holdout_features",
                             "h.npy", "--labels_out", "l.json", "--report", "m.json"))
    for argv, what in (
            (["--features", "a.npy"], "exactly one"),
            (["--fit", "--clusters", "c.npz", "--features", "a.npy", "--k", "3", "--out", "c.npz"], "exactly one"),
            (["--fit", "--k", "3", "--out", "c.npz"], "--features"),
            (["--fit", "--features", "a.npy", "--out", "c.npz"], "--k and --out"),
            (["--fit", "--features", "a.npy", "--k", "3"], "--k and --out"),
            (["--fit", "--features", "a.npy", "--k", "0", "--out", "c.npz"], "--k"),
            (["--fit", "--features", "a.npy", "--k", "3", "3", "--out", "c.npz"], "distinct"),
            (["--fit", "--features", "a.npy", "--k", "3", "--out", "c.txt"], ".npz"),
            (["--fit", "--features", "a.npy", "--k", "3", "--out", "c.npz", "--n_init", "0"], "--n_init"),
            (["--fit", "--features", "a.npy", "--k", "3", "--out", "c.npz", "--tol", "1.5"], "--tol"),
            (["--fit", "--features", "a.npy", "--k", "3", "--out", "c.npz", "--seed", "-1"], "--seed"),
            (["--fit", "--features", "a.npy", "--k", "3", "--out", "c.npz", "--report", "m.json"], "--report"),
            (["--fit", "--features", "a.npy", "--k", "3", "--out", "c.npz", "--ref_features", "t.npy"], "--ref_features"),
            (["--clusters", "c.npz", "--features", "s.npy", "--k", "3"], "--k"),
            (["--clusters", "c.npz", "--features", "s.npy", "--normalize"], "--normalize"),
            (["--clusters", "c.npz", "--features", "s.npy", "--out", "d.npz"], "--out"),
            (["--clusters", "c.npz", "--features", "s.npy", "--labels_out", "l.txt"], ".json")):
        with pytest.raises(ValueError, match=re.escape(what)):
            cluster.check_args(_args(*argv))


def test_kmeans_argument_checks():
    import torch
    for kw in ({"n_init": 0}, {"max_iter": 0}, {"tol": -1.0}, {"tol": 1.0}, {"seed": -1}, {"init": "random"},
               {"init": torch.zeros(3, 2)}, {"init": torch.zeros(4, 2, dtype=torch.float64)},
               {"init": torch.zeros(4, 2), "n_init": 2}):
        with pytest.raises(ValueError):
            cluster.KMeans(4, **kw)
    with pytest.raises(ValueError):
        cluster.KMeans(0)
    km = cluster.KMeans(4, init=torch.zeros(4, 2))
    with pytest.raises(ValueError, match="fit or load"):
        km.predict(torch.zeros(3, 2))
    with pytest.raises(ValueError, match="CUDA/HIP"):
        cluster.lloyd_step(torch.zeros(3, 2), torch.zeros(2, 2))


def test_save_load_round_trip(tmp_path):
    import torch
    km = cluster.KMeans(3, n_init=2, max_iter=7, tol=0.25, seed=5, normalize=True)
    r = np.random.default_rng(0)
    km.centroids = torch.from_numpy(r.standard_normal((3, 4)).astype(np.float32))
    km.counts = torch.tensor([5, 0, 2])
    km.cluster_inertia = torch.from_numpy(r.random(3))
    km.inertia, km.n_iter, km.converged = cluster.host_sum(km.cluster_inertia.numpy()), 4, True
    path = str(tmp_path / "c.npz")
    km.save(path)
    back = cluster.KMeans.load(path, device="cpu")
    assert np.array_equal(back.centroids.numpy().view(np.uint32), km.centroids.numpy().view(np.uint32))
    assert back.counts.tolist() == [5, 0, 2] and back.counts.dtype == torch.int64
    assert np.array_equal(_bits(back.cluster_inertia.numpy()), _bits(km.cluster_inertia.numpy()))
    assert (back.normalize, back.n_clusters, back.n_init, back.max_iter, back.tol, back.seed) == (True, 3, 2, 7, 0.25, 5)
    assert back.inertia == km.inertia and back.n_iter == 4 and back.converged is True and back.empty_clusters == [1]
    a = cluster.read_clusters(path)
    assert a["arguments"]["init"] == "k-means++"
    np.savez(str(tmp_path / "bad.npz"), centroids=np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError, match="KMeans.save"):
        cluster.read_clusters(str(tmp_path / "bad.npz"))


# ------------------------------------------------------------------------------------------------ the library surface
def test_header_binding_and_exports():
    with open(os.path.join(ROOT, "include", "tinyedm_hip.h")) as f:
        hdr = f.read()
    from tinyedm_amd import ops
    for name in ("edm_cluster_block", "edm_f32_cluster_sums_partial", "edm_f32_cluster_sums_finish"):
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", hdr, re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip() != "void"]) == len(_lib.SIGNATURES[name]), name
    if os.path.exists(_lib.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
        exported = set(re.findall(r"\bT (edm_[a-z0-9_]+)", nm.stdout))
        assert {"edm_cluster_block", "edm_f32_cluster_sums_partial", "edm_f32_cluster_sums_finish"} <= exported
        # the chunk length the tables are cut with is the built library's own (host logic: no GPU needed to ask)
        assert ops.cluster_block() == C.BLOCK, "the restatement reads the header the library was built from"
    import tinyedm
    import tinyedm.cluster as shim
    assert tinyedm.KMeans is cluster.KMeans and shim.main is cluster.main and tinyedm.mode_report is cluster.mode_report


# ------------------------------------------------------------------------------------------------ the documented commands
def _readme_train_overrides():
    """(config name, overrides) of the README's self-guided training command"""
    with open(os.path.join(ROOT, "README.md")) as f:
        lines = [ln for ln in f if "datamodule.labels_path=" in ln and "experiments/train.py" in ln]
    assert len(lines) == 1, "one README line documents the self-guided loop"
    cmd = [c for c in lines[0].split("#")[0].split("&&") if "experiments/train.py" in c][0].split()
    name = [a.split("=", 1)[1] for a in cmd if a.startswith("--config-name=")][0]
    return name, [a for a in cmd if "=" in a and not a.startswith("--")]


def test_readme_self_guided_command_composes(tmp_path):
    """the datamodule and the embedding of the documented training command instantiate from its own overrides"""
    from tinyedm_amd import config
    from tinyedm_amd.datamodules import CIFAR10DataModule
    name, overrides = _readme_train_overrides()
    keys = {o.split("=", 1)[0] for o in overrides}
    assert {"datamodule.labels_path", "datamodule.val_labels_path", "datamodule.label_classes",
            "model.embedding.num_classes", "model.embedding.label_dropout"} <= keys
    cfg = config.compose(name, os.path.join(ROOT, "experiments", "conf"), overrides)
    dm = config.instantiate(cfg["datamodule"])
    assert isinstance(dm, CIFAR10DataModule), "real images: the label files index the training set"
    assert dm.labels_path == "train_labels.json" and dm.val_labels_path == "test_labels.json"
    assert dm.num_classes == dm.label_classes == cfg["model"]["embedding"]["num_classes"] == 100
    assert cfg["model"]["embedding"]["label_dropout"] == 0.1
    import inspect
    import tinyedm
    assert {"num_classes", "label_dropout"} <= set(inspect.signature(tinyedm.Embedding.__init__).parameters)
