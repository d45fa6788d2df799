"""Host-side checks of the loss by noise level (no GPU): the training-distribution levels, the per-level statistics and
their merge against the restatements of tests/evaluate_ref.py, every argument error before anything is loaded, and the
new entry points in the header."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import evaluate_ref as R
from parity_log import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _E():
    import tinyedm_amd.evaluate as E
    return E


@pytest.mark.parametrize("P_mean,P_std,L", [(-1.2, 1.2, 16), (-0.4, 1.0, 7), (0.3, 2.0, 1), (-1.2, 1.2, 257)])
def test_level_sigmas(P_mean, P_std, L):
    got = _E().level_sigmas(P_mean, P_std, L)
    ref = R.level_sigmas(P_mean, P_std, L)
    assert len(got) == L
    err = max(abs(a - b) / b for a, b in zip(got, ref))
    record(f"evaluate/level_sigmas_{L}_rel", err, 1e-12)
    assert err <= 1e-12
    assert all(a < b for a, b in zip(got, got[1:]))
    # the quantile midpoints are symmetric about 1/2: the mean of ln sigma is P_mean
    log_mean = math.fsum(math.log(s) for s in got) / L
    assert abs(log_mean - P_mean) <= 1e-12, log_mean


def _se(draws=2, L=3, n=5):
    g = np.random.default_rng(3)
    return g.uniform(0.5, 40.0, size=(draws, L, n)) * np.array([1e-3, 1.0, 1e3])[None, :, None]


def test_level_statistics_by_hand():
    E = _E()
    se, chw, sigmas, sd = _se(), 12, [0.05, 0.7, 30.0], 0.5
    sums = E.level_sums(se, chw)
    ref_sums = R.level_sums(se, chw)
    assert sums.shape == (3, 3) and sums.dtype == np.float64
    assert np.abs(sums - ref_sums).max() <= 1e-12 * np.abs(ref_sums).max()
    got = E.level_stats(sums, sigmas, sd)
    ref = R.level_stats(se, chw, sigmas, sd)
    assert got["sigma"] == sigmas and got["count"] == [5, 5, 5]
    for key in ("mse", "mse_stderr", "loss"):
        err = max(abs(a - b) / abs(b) for a, b in zip(got[key], ref[key]))
        record(f"evaluate/stats_{key}_rel", err, 1e-12)
        assert err <= 1e-12, (key, got[key], ref[key])
    # lambda by hand at sigma = sigma_data: 2 / sigma_data^2
    assert abs(E.edm_weight(0.5, 0.5) - 8.0) <= 1e-15
    # one image: a mean, no standard error
    one = E.level_stats(E.level_sums(se[:, :, :1], chw), sigmas, sd)
    assert one["count"] == [1, 1, 1] and one["mse_stderr"] == [None, None, None]
    assert abs(one["mse"][1] - se[:, 1, 0].mean() / chw) <= 1e-12 * one["mse"][1]


def test_merge_level_sums_equals_unsharded():
    E = _E()
    se, chw = _se(draws=3, L=4 - 1, n=11), 48
    whole = E.level_sums(se, chw)
    parts = [E.level_sums(se[:, :, r::2], chw) for r in range(2)]       # ids = rank (mod 2)
    merged = E.merge_level_sums(parts)
    ref = R.merge_level_sums([R.level_sums(se[:, :, r::2], chw) for r in range(2)])
    for a, b in ((merged, whole), (merged, ref)):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    sig = [0.1, 1.0, 10.0]
    sa, sb = E.level_stats(merged, sig, 0.5), E.level_stats(whole, sig, 0.5)
    for key in ("mse", "mse_stderr", "loss"):
        assert max(abs(a - b) / abs(b) for a, b in zip(sa[key], sb[key])) <= 1e-12
    assert sa["count"] == [11, 11, 11]
    with pytest.raises(ValueError):
        E.merge_level_sums([])
    with pytest.raises(ValueError):
        E.merge_level_sums([whole, whole[:, :2]])


BASE = ["--ckpt_path", "/nonexistent/a.ckpt", "--report", "/nonexistent/out.json"]
DATA = ["--dataset", "cifar10", "--data_dir", "/nonexistent"]
CLI_ERRORS = [
    (BASE, "exactly one data source"),
    (BASE + DATA + ["--image_dir", "d", "--image_size", "8"], "exactly one data source"),
    (BASE + DATA + ["--sigmas", "0.5", "0.5", "2.0"], "strictly increasing"),
    (BASE + DATA + ["--sigmas", "2.0", "1.0"], "strictly increasing"),
    (BASE + DATA + ["--sigmas", "-1.0", "1.0"], "> 0"),
    (BASE + DATA + ["--num_levels", "0"], "num_levels"),
    (BASE + DATA + ["--labels_json", "l.json"], "--image_dir"),
    (BASE + ["--dataset", "mnist"], "--data_dir"),
    (BASE + ["--image_dir", "d"], "--image_size"),
    (BASE + DATA + ["--num_draws", "0"], "num_draws"),
    (BASE + DATA + ["--batch_size", "0"], "batch_size"),
    (BASE + DATA + ["--num_images", "0"], "--num_images"),
    (BASE + DATA + ["--seed", "-1"], "seed"),
]


@pytest.mark.parametrize("argv,needle", CLI_ERRORS, ids=[str(i) for i in range(len(CLI_ERRORS))])
def test_cli_argument_errors_before_anything_is_loaded(argv, needle, monkeypatch):
    """the checkpoint path does not exist and the GPU must not be touched: the refusal comes first"""
    E = _E()
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("the GPU was touched"))
    monkeypatch.setattr(torch, "load", lambda *a, **k: pytest.fail("a checkpoint was opened"))
    with pytest.raises(ValueError, match=needle):
        E.check_args(E.build_parser().parse_args(argv))
    with pytest.raises(SystemExit) as exc:
        E.main(argv)
    assert exc.value.code == 2


def test_cli_module_alias_exits_with_status_2():
    r = subprocess.run([sys.executable, "-m", "tinyedm.evaluate", *BASE], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 2 and "exactly one data source" in r.stderr, r.stderr[-1500:]


def test_constructor_errors():
    E = _E()
    ok = E.NoiseLevelEvaluator()
    assert ok.num_levels == 16 and ok.num_draws == 1 and ok.batch_size == 512 and ok.network_dtype == "bf16"
    assert E.NoiseLevelEvaluator(sigmas=torch.tensor([0.5, 1.0])).sigmas == [0.5, 1.0]
    for kw in (dict(num_levels=0), dict(num_levels=65536), dict(num_levels=2.0), dict(num_levels=True),
               dict(sigmas=[]), dict(sigmas=[1.0, 1.0]), dict(sigmas=[2.0, 1.0]), dict(sigmas=[0.0, 1.0]),
               dict(sigmas=[1.0, math.inf]), dict(sigmas=[math.nan]), dict(sigmas=[1.0, 1.0 + 1e-12]),
               dict(sigmas=list(range(1, 65537))), dict(P_std=0.0), dict(P_mean=math.nan), dict(seed=-1),
               dict(seed=1 << 64), dict(num_draws=0), dict(batch_size=0), dict(network_dtype="fp16")):
        with pytest.raises(ValueError):
            E.NoiseLevelEvaluator(**kw)
    # the training-distribution levels need a P_mean / P_std from somewhere
    with pytest.raises(ValueError, match="P_mean"):
        ok.levels_for(lambda x, s, l: x)
    lev = E.NoiseLevelEvaluator(num_levels=4, P_mean=-1.2, P_std=1.2).levels_for(lambda x, s, l: x)
    assert lev == R.level_sigmas(-1.2, 1.2, 4) or max(abs(a - b) / b for a, b in zip(lev, R.level_sigmas(-1.2, 1.2, 4))) <= 1e-12
    # a CPU image never reaches the library
    with pytest.raises(ValueError, match="GPU"):
        E.NoiseLevelEvaluator(sigmas=[1.0]).evaluate(lambda x, s, l: x, torch.zeros(2, 3, 4, 4))
    from tinyedm_amd.callbacks import LossByNoiseLevel
    for kw in (dict(num_images=0), dict(every_n_epochs=0), dict(num_levels=0), dict(sigmas=[2.0, 1.0])):
        with pytest.raises(ValueError):
            LossByNoiseLevel(**kw)


def test_ops_reject_cpu_operands_before_launch():
    from tinyedm_amd import ops
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.eval_diffuse(x, torch.zeros(2, dtype=torch.uint32), torch.zeros(2, dtype=torch.int32), torch.ones(1),
                         torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.eval_sqerr(x, x)
    assert ops.EVAL_MAX_LEVELS == 65535 == _E().MAX_LEVELS


def test_best_checkpoint():
    E = _E()
    ent = {"a": {"expected_loss": 0.31, "mean_loss": 0.31}, "b": {"expected_loss": 0.29, "mean_loss": 0.29}}
    assert E.best_checkpoint(ent) == ("b", "expected_loss")
    ent = {"a": {"expected_loss": None, "mean_loss": 0.2}, "b": {"expected_loss": None, "mean_loss": 0.4}}
    assert E.best_checkpoint(ent) == ("a", "mean_loss")


def test_restated_noise_stream():
    """the restatement the GPU tests compare against: unit normals, keyed by (id, level, draw, seed), its own tag"""
    seed = 0x9E3779B97F4A7C15
    n = R.eval_noise((3, 3, 32, 32), [5, 0, 1000003], [0, 2, 1], seed, 3)
    assert n.shape == (3, 3, 32, 32) and abs(n.mean()) < 5 / math.sqrt(n.size) and abs(n.std() - 1) < 5 / math.sqrt(2 * n.size)
    # a row is a function of its own (id, level) only
    assert np.array_equal(R.eval_noise((1, 3, 32, 32), [1000003], [1], seed, 3)[0], n[2])
    for other in (R.eval_noise((1, 3, 32, 32), [1000003], [2], seed, 3), R.eval_noise((1, 3, 32, 32), [1000003], [1], seed, 4),
                  R.eval_noise((1, 3, 32, 32), [1000004], [1], seed, 3), R.eval_noise((1, 3, 32, 32), [1000003], [1], seed + 1, 3)):
        assert abs(np.corrcoef(other.ravel(), n[2].ravel())[0, 1]) < 0.1
    # the tag keeps clear of every other stream's for each level < 65536
    assert R.EVAL_TAG == 0x45560000
    others = {0x4348, 0x4950, 0x4E4C, 0x4E4D, 0x0000}       # churn, blend, probes (ev 0 / 1), the 16-bit diffuser tags
    assert (R.EVAL_TAG ^ 0xFFFF) >> 16 == 0x4556 and 0x4556 not in others
    kat = [int(v) for v in R.philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert kat == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_abi_names_in_header_and_bindings():
    from tinyedm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    names = set(re.findall(r"\b(edm_[a-z0-9_]+)\s*\(", hdr))
    for name in ("edm_eval_diffuse", "edm_eval_sqerr"):
        assert name in names and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["edm_eval_diffuse"]) == 12 and len(_lib.SIGNATURES["edm_eval_sqerr"]) == 8
