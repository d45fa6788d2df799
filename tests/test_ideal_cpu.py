"""The ideal denoiser, the parts that need no GPU: the numpy restatement against hand cases, the chunked running merge of the
kernels against the one-shot softmax, the host logic of tinyedm_amd/ideal.py (constructor and sigma refusals, log_density,
the command line's refusals, the report's reduction) and the header's declarations."""
import math
import os
import re

import numpy as np
import pytest

import ideal_cases as IC
import ideal_ref as IR
from tinyedm_amd import ideal as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("edm_ideal_begin", "edm_ideal_logits", "edm_ideal_softmax", "edm_ideal_accumulate", "edm_ideal_finish")


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("form", IR.FORMS)
def test_single_reference_returns_the_image(form):
    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, (1, 2, 3, 3), dtype=np.uint8)
    y = IR.normalize(data)
    x = rng.standard_normal((4, 18))
    for sigma in (0.002, 0.7, 80.0):
        out = IR.ideal(x, sigma, data, form=form)
        assert np.abs(out["D"] - y[0]).max() <= (0 if form == "f64" else 1e-6)
        assert np.array_equal(out["top_index"], np.zeros(4)) and np.allclose(out["top_weight"], 1.0)
        assert np.allclose(out["entropy"], 0.0) and np.allclose(out["effective_count"], 1.0)
    # lse of one Gaussian is its exponent
    out = IR.ideal(x, 0.7, data)
    assert np.allclose(out["lse"], -((x - y[0]) ** 2).sum(axis=1) / (2 * 0.49), rtol=1e-13)


def test_large_sigma_returns_the_mean():
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, (9, 1, 4, 4), dtype=np.uint8)
    y = IR.normalize(data)
    x = rng.standard_normal((3, 16))
    out = IR.ideal(x, 1e6, data)
    assert np.abs(out["D"] - y.mean(axis=0)).max() <= 1e-9
    assert np.allclose(out["effective_count"], 9.0, rtol=1e-9) and np.allclose(out["entropy"], math.log(9.0), rtol=1e-9)


def test_small_sigma_returns_the_nearest_image():
    rng = np.random.default_rng(2)
    data = rng.integers(0, 256, (12, 3, 2, 2), dtype=np.uint8)
    y = IR.normalize(data)
    for form in IR.FORMS:
        out = IR.ideal(y[[7, 0, 11]], 0.002, data, form=form)
        assert np.array_equal(out["top_index"], [7, 0, 11]) and np.allclose(out["top_weight"], 1.0)
        assert np.abs(out["D"] - y[[7, 0, 11]]).max() <= 1e-6


def test_duplicates_split_the_weight():
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, (6, 1, 3, 3), dtype=np.uint8)
    data[4] = data[1]
    y = IR.normalize(data)
    out = IR.ideal(y[[1]] + 1e-4, 0.01, data)
    assert out["top_index"][0] == 1                               # the lower index of the pair
    assert abs(out["top_weight"][0] - 0.5) <= 1e-12 and abs(out["entropy"][0] - math.log(2.0)) <= 1e-9
    assert np.abs(out["D"][0] - y[1]).max() <= 1e-12


def test_class_restriction_is_the_subset():
    rng = np.random.default_rng(4)
    data = IR.clustered_u8(rng, 20, (1, 3, 3), 6)
    ref_labels = rng.integers(0, 3, 20)
    ref_labels[:3] = [0, 1, 2]
    x = rng.standard_normal((5, 9)) * 0.3
    labels = np.array([0, 1, 2, 1, 0])
    sig = np.array([0.1, 0.3, 1.0, 3.0, 0.2])
    out = IR.ideal(x, sig, data, ref_labels=ref_labels, labels=labels)
    for q in range(5):
        rows = np.nonzero(ref_labels == labels[q])[0]
        sub = IR.ideal(x[q:q + 1], sig[q], data[rows])
        for k in ("D", "lse", "entropy", "top_weight"):
            assert np.array_equal(out[k][q], sub[k][0]), k
        assert out["top_index"][q] == rows[sub["top_index"][0]]


@pytest.mark.parametrize("chunk", [1, 3, 7, 64])
def test_chunked_merge_is_the_one_shot_softmax(chunk):
    """the running (max, sum, sum p (l - max), acc) of the kernels, rescaled between chunks, against one softmax; with it
    the entropy identity ent = lse - E_w[l]"""
    rng = np.random.default_rng(5)
    for scale in (1.0, 300.0, 1e5):
        l = -np.abs(rng.standard_normal(23)) * scale
        l[5] = l[19]                                              # equal logits in two chunks
        y = rng.standard_normal((23, 4))
        D, lse, ent = IR.chunked_merge(l, y, chunk)
        m = l.max()
        p = np.exp(l - m)
        w = p / p.sum()
        assert np.allclose(D, w @ y, rtol=1e-12, atol=1e-14)
        assert abs(lse - (m + math.log(p.sum()))) <= 1e-12 * max(1.0, abs(lse))
        nz = w > 0
        assert abs(ent - -(w[nz] * np.log(w[nz])).sum()) <= 1e-10
        assert abs(ent - (lse - (w * l).sum())) <= 1e-9 * max(1.0, abs(lse))
    # the maximum arrives last: every earlier chunk is rescaled to nothing
    l = np.array([-1e6, -2e6, -5e5, 0.0])
    D, lse, ent = IR.chunked_merge(l, np.eye(4), 1)
    assert np.array_equal(D, [0.0, 0.0, 0.0, 1.0]) and lse == 0.0 and ent == 0.0


def test_soft_cases_are_soft():
    """what the GPU tests rely on, on the fp64 form alone (the small shapes; the CIFAR-sized case asserts it when it runs)"""
    for name in ("tails", "chunks"):
        data, x, sig = IC.soft_case(name)
        eff = IR.ideal(x, sig, data)["effective_count"].mean()
        assert 2.0 <= eff <= data.shape[0] / 2.0, (name, eff)


# ------------------------------------------------------------------------------------------------ host logic
def _set(**kw):
    args = dict(shape=(10, 3, 4, 4), dtype_is_u8=True, labels=None, mean=0.5, std=0.5, sigma_data=0.5, num_classes=None,
                ref_chunk=None)
    args.update(kw)
    return I.check_set(**args)


def test_check_set_accepts():
    assert _set() == (None, None, None)
    lab, n, counts = _set(labels=np.arange(10) % 5)
    assert lab.dtype == np.int32 and n == 5 and counts.tolist() == [2] * 5
    assert _set(labels=[0] * 10, num_classes=1)[1] == 1
    _set(ref_chunk=1, mean=0, std=1)


@pytest.mark.parametrize("kw", [
    dict(dtype_is_u8=False),                             # not uint8
    dict(shape=(10, 48)),                                # rank
    dict(shape=(10, 3, 4)),
    dict(shape=(0, 3, 4, 4)),                            # empty set
    dict(shape=(10, 3, 0, 4)),
    dict(shape=(10, 3, 128, 128)),                       # 49152 elements per image
    dict(labels=np.zeros(9, dtype=np.int64)),            # label count
    dict(labels=np.zeros((10, 1), dtype=np.int64)),
    dict(labels=np.zeros(10)),                           # float labels
    dict(labels=np.array([0, 1, 3] * 3 + [0])),          # class 2 owns no image
    dict(labels=np.arange(10) % 2, num_classes=3),       # class 2 owns no image
    dict(labels=np.arange(10) % 4, num_classes=3),       # label outside the table
    dict(labels=np.arange(10) - 1),                      # negative label
    dict(num_classes=4),                                 # num_classes without labels
    dict(labels=np.arange(10) % 2, num_classes=0),
    dict(ref_chunk=0), dict(ref_chunk=-3), dict(ref_chunk=2.5), dict(ref_chunk=True),
    dict(mean=float("nan")), dict(mean=float("inf")), dict(std=float("nan")), dict(std=float("inf")),
    dict(std=0.0), dict(std=-0.5), dict(mean=(0.5, 0.5, 0.5)), dict(sigma_data=0.0), dict(sigma_data=float("nan")),
])
def test_check_set_refusals(kw):
    with pytest.raises(ValueError):
        _set(**kw)


def test_constructor_refuses_before_the_device():
    """the refusals of the constructor need no GPU: they come before the set is moved"""
    good = np.zeros((4, 1, 2, 2), dtype=np.uint8)
    for data, kw in ((good.astype(np.float32), {}), (good[0], {}), (good[:0], {}), (good, {"labels": [0, 1, 2]}),
                     (good, {"labels": [0, 0, 2, 2]}), (good, {"ref_chunk": 0}), (good, {"mean": float("nan")}),
                     (good, {"std": 0.0}), ([[1, 2]], {})):
        with pytest.raises(ValueError):
            I.IdealDenoiser(data, **kw)
    import torch
    with pytest.raises(ValueError):
        I.IdealDenoiser(torch.zeros(4, 1, 2, 2), labels=None)


def test_check_sigma():
    assert I.check_sigma(0.002) == 0.002 and I.check_sigma(80) == 80.0
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e39, True, "1", None):
        with pytest.raises(ValueError):
            I.check_sigma(bad)


def test_log_density_against_fp64():
    rng = np.random.default_rng(6)
    data = IR.clustered_u8(rng, 7, (1, 2, 3), 9)
    y = IR.normalize(data)
    x = y[[2, 5]] + 0.3 * rng.standard_normal((2, 6))
    sig = np.array([0.3, 1.1])
    out = IR.ideal(x, sig, data)
    # the mixture density, term by term
    want = []
    for q in range(2):
        dens = np.exp(-((x[q] - y) ** 2).sum(axis=1) / (2 * sig[q] ** 2)) / (2 * math.pi * sig[q] ** 2) ** 3
        want.append(math.log(dens.mean()))
    got = I.log_density(out["lse"], 7, 6, sig)
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-12)
    assert np.array_equal(got, IR.log_density(out["lse"], 7, 6, sig))
    assert np.allclose(I.log_density(out["lse"], np.array([7.0, 2.0]), 6, sig) - got, [0.0, math.log(3.5)], atol=1e-12)


# ------------------------------------------------------------------------------------------------ command line refusals
def _args(*argv):
    return I.build_parser().parse_args(list(argv))


DATA = ("--dataset", "cifar10", "--data_dir", "d")
DIRS = ("--image_dir", "h", "--train_image_dir", "t", "--image_size", "8")


def test_cli_accepts():
    from tinyedm_amd.evaluate import NoiseLevelEvaluator
    ev = I.check_args(_args(*DATA, "--report", "r.json", "--ckpt_path", "a.ckpt", "b.ckpt", "--load_ema", "--conditional"))
    assert isinstance(ev, NoiseLevelEvaluator) and ev.num_levels == 16
    assert I.check_args(_args(*DATA, "--report", "r.json", "--sigmas", "0.1", "1")).sigmas == [0.1, 1.0]
    I.check_args(_args(*DATA, "--report", "r.json", "--P_mean", "-0.4", "--P_std", "1.0", "--num_levels", "4"))
    I.check_args(_args(*DIRS, "--report", "r.json", "--sigmas", "1", "--mean", "0.5", "--std", "0.25"))
    I.check_args(_args(*DIRS, "--report", "r.json", "--sigmas", "1", "--labels_json", "a", "--train_labels_json", "b",
                       "--conditional"))
    assert I.check_args(_args(*DATA, "--samples", "4", "--output_dir", "o")) is None
    assert I.check_args(_args(*DATA, "--samples", "4", "--output_dir", "o", "--solver", "dpmpp", "--num_steps", "9")) is None
    assert I.check_args(_args(*DATA, "--samples", "4", "--output_dir", "o", "--S_churn", "10")) is None


@pytest.mark.parametrize("argv", [
    DATA,                                                               # no task
    DATA + ("--report", "r.json", "--samples", "2", "--output_dir", "o"),    # two tasks
    ("--report", "r.json", "--sigmas", "1"),                            # no data source
    DATA + DIRS + ("--report", "r.json", "--sigmas", "1"),              # two of them
    ("--dataset", "cifar10", "--report", "r.json", "--sigmas", "1"),    # --dataset without --data_dir
    ("--image_dir", "h", "--image_size", "8", "--report", "r.json", "--sigmas", "1"),       # no training set
    DATA + ("--train_image_dir", "t", "--report", "r.json", "--sigmas", "1"),
    DIRS + ("--report", "r.json", "--sigmas", "1", "--labels_json", "a"),                   # one label file of two
    DIRS + ("--report", "r.json", "--sigmas", "1", "--conditional"),                        # no labels
    DIRS + ("--report", "r.json", "--sigmas", "1", "--mean", "0.5", "0.4", "0.3", "--std", "0.2", "0.2", "0.2"),
    DIRS + ("--report", "r.json", "--sigmas", "1", "--mean", "0.5", "--std", "0"),
    DATA + ("--report", "r.json"),                                      # no checkpoint: the levels are not defined
    DATA + ("--report", "r.json", "--P_mean", "0"),
    DATA + ("--report", "r.json", "--sigmas", "1", "0.5"),              # not increasing
    DATA + ("--report", "r.json", "--sigmas", "1", "--num_images", "0"),
    DATA + ("--report", "r.json", "--sigmas", "1", "--num_draws", "0"),
    DATA + ("--report", "r.json", "--sigmas", "1", "--ref_chunk", "0"),
    DATA + ("--report", "r.json", "--sigmas", "1", "--output_dir", "o"),
    DATA + ("--report", "r.json", "--ckpt_path", "a.ckpt", "a.ckpt"),   # a checkpoint twice
    DATA + ("--samples", "4"),                                          # no --output_dir
    DATA + ("--samples", "0", "--output_dir", "o"),
    DATA + ("--samples", "4", "--output_dir", "o", "--ckpt_path", "a.ckpt"),
    DATA + ("--samples", "4", "--output_dir", "o", "--num_steps", "1"),
    DATA + ("--samples", "4", "--output_dir", "o", "--S_churn", "-1"),
    DATA + ("--samples", "4", "--output_dir", "o", "--solver", "dpmpp", "--S_churn", "5"),
])
def test_cli_refusals(argv):
    with pytest.raises(ValueError):
        I.check_args(_args(*argv))


def test_cli_refusal_exits_before_anything_is_loaded(capsys):
    with pytest.raises(SystemExit) as e:
        I.main(["--dataset", "cifar10", "--data_dir", "/nonexistent", "--report", "r.json"])
    assert e.value.code == 2 and "--sigmas" in capsys.readouterr().err


def test_alias_module():
    import tinyedm.ideal as A
    import tinyedm_amd
    assert A.main is I.main and A.IdealDenoiser is I.IdealDenoiser and tinyedm_amd.IdealDenoiser is I.IdealDenoiser


# ------------------------------------------------------------------------------------------------ the report's reduction
def test_reduce_gap_on_a_synthetic_matrix():
    from tinyedm_amd.evaluate import edm_weight
    rng = np.random.default_rng(8)
    chw, sigmas = 12, [0.1, 1.0, 10.0]
    names = ("ideal_train", "ideal_test", "train", "test", "to_ideal_train", "to_ideal_test")
    se = {k: rng.random((2, 3, 5)) * 7 for k in names}
    se["train"] = se["ideal_train"] + rng.random((2, 3, 5))
    eff = {"train": 1 + rng.random((2, 3, 5)) * 4, "test": 1 + rng.random((2, 3, 5)) * 9}
    out = I.reduce_gap(se, eff, chw, sigmas, 0.5)
    assert out["sigma"] == sigmas and out["weight"] == [edm_weight(s, 0.5) for s in sigmas]
    for k in names:
        col = k if k.startswith("to_ideal") else k + "_mse"
        want = se[k].mean(axis=(0, 2)) / chw
        assert np.allclose(out[col], want, rtol=1e-13), k
        assert np.allclose(out["weighted"][col], np.array(out["weight"]) * want, rtol=1e-13)
    assert out["excess_train"] == [a - b for a, b in zip(out["train_mse"], out["ideal_train_mse"])]
    assert all(v > 0 for v in out["excess_train"])
    assert out["weighted"]["excess_train"] == [w * v for w, v in zip(out["weight"], out["excess_train"])]
    for k in ("train", "test"):
        assert np.allclose(out["effective_count_" + k], eff[k].mean(axis=(0, 2)), rtol=1e-13)
    # the ideal columns alone, and an exact zero stays an exact zero
    alone = I.reduce_gap({k: se[k] for k in names[:2]}, eff, chw, sigmas, 0.5)
    assert "train_mse" not in alone and "excess_train" not in alone and alone["ideal_test_mse"] == out["ideal_test_mse"]
    same = I.reduce_gap({"ideal_train": se["train"], "train": se["train"], "to_ideal_train": np.zeros((2, 3, 5))}, {}, chw,
                        sigmas, 0.5)
    assert same["excess_train"] == [0.0] * 3 and same["to_ideal_train"] == [0.0] * 3
    with pytest.raises(ValueError):
        I.reduce_gap({"ideal_train": np.zeros((2, 4, 5))}, {}, chw, sigmas, 0.5)


# ------------------------------------------------------------------------------------------------ declarations
def test_header_declares_the_entries_and_ops_binds_them():
    from tinyedm_amd import _lib
    with open(os.path.join(ROOT, "include", "tinyedm_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "tinyedm_amd", "csrc", "ideal.hip")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "tinyedm_amd", "ops.py")) as f:
        ops_src = f.read()
    declared = set(re.findall(r"\bint\s+(edm_ideal_\w+)\s*\(", header))
    defined = set(re.findall(r'extern "C" int (edm_ideal_\w+)\(', src))
    bound = {k for k in _lib.SIGNATURES if k.startswith("edm_ideal_")}
    called = set(re.findall(r'_lib\.call\("(edm_ideal_\w+)"', ops_src))
    assert declared == defined == bound == called == set(ENTRIES)
    for name in ENTRIES:      # as many parameters in the header as argument types in the binding
        params = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name]), name
    assert "the reference has no call site; Karras et al. 2022 App. B.3" in header.replace("The reference", "the reference")
    assert "mfma_f32_16x16x4f32" in src and "atomicAdd" not in src
    from tinyedm_amd import ops
    assert (ops.IDEAL_MAX_K, ops.IDEAL_MAX_R) == (I.MAX_K, I.MAX_R)
