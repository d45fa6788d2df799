"""Label dropout and single-network classifier-free guidance, host side (no GPU): the Embedding constructor's validation,
the hparams round trip (at label_dropout 0 the dict of the reference, pinned in tests/golden/hparams_cifar10_cond.json),
the host threshold of the in-kernel draw, the solvers' guide="unconditional" sentinel and the generate CLI."""
import json
import os
import re

import pytest

import tinyedm
from tinyedm.config import compose, instantiate
from tinyedm_amd import DeterministicSolver, MultistepSolver, StochasticSolver, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "experiments", "conf")


@pytest.mark.parametrize("p", [-0.1, 1.5, float("nan")])
def test_label_dropout_outside_unit_interval_rejected(p):
    with pytest.raises(ValueError, match="label_dropout"):
        tinyedm.Embedding(32, 64, 10, label_dropout=p)


@pytest.mark.parametrize("num_classes", [None, -1])
def test_label_dropout_needs_a_conditional_embedding(num_classes):
    with pytest.raises(ValueError, match="label_dropout"):
        tinyedm.Embedding(32, 64, num_classes, label_dropout=0.1)
    assert tinyedm.Embedding(32, 64, num_classes, label_dropout=0.0).label_dropout == 0.0


def test_label_dropout_bounds_accepted():
    for p in (0.0, 0.1, 1.0):
        assert tinyedm.Embedding(32, 64, 10, label_dropout=p).label_dropout == p


def test_hparams_at_zero_are_the_reference_dict(golden_dir):
    with open(os.path.join(golden_dir, "hparams_cifar10_cond.json")) as f:
        expected = json.load(f)
    model = instantiate(compose("cifar10_cond", CONF).model)
    d = tinyedm.utils.deinstantiate(model)
    assert "label_dropout" not in d["embedding"]
    assert json.loads(json.dumps(d)) == expected
    # an explicit 0 is the default too
    model0 = instantiate(compose("cifar10_cond", CONF, ["model.embedding.label_dropout=0.0"]).model)
    assert json.loads(json.dumps(tinyedm.utils.deinstantiate(model0))) == expected


def test_hparams_round_trip_at_nonzero():
    model = instantiate(compose("cifar10_cond", CONF, ["model.embedding.label_dropout=0.1"]).model)
    assert model.embedding.label_dropout == 0.1
    d = tinyedm.utils.deinstantiate(model)
    assert d["embedding"]["label_dropout"] == 0.1
    assert model.hparams["embedding"]["label_dropout"] == 0.1       # what a checkpoint stores
    again = instantiate(d)
    assert again.embedding.label_dropout == 0.1
    again.load_state_dict(model.state_dict(), strict=True)


def test_mnist_config_takes_the_override():
    model = instantiate(compose("mnist", CONF, ["model.embedding.label_dropout=0.1"]).model)
    assert model.conditional and model.embedding.label_dropout == 0.1


@pytest.mark.parametrize("p,thr", [(0.0, 0), (1e-9, 4), (0.1, 429496730), (0.5, 1 << 31), (1.0, 1 << 32)])
def test_host_threshold(p, thr):
    assert ops.label_drop_threshold(p) == thr
    assert ops.label_drop_threshold(p) == min(max(round(p * 2.0 ** 32), 0), 2 ** 32)


def test_host_threshold_clamped():
    assert ops.label_drop_threshold(-0.5) == 0
    assert ops.label_drop_threshold(2.0) == 1 << 32


@pytest.mark.parametrize("cls", [DeterministicSolver, StochasticSolver, MultistepSolver])
def test_solvers_accept_the_unconditional_sentinel(cls):
    sol = cls(num_steps=8, guide="unconditional", guidance=2.0)
    assert sol.guide == "unconditional"
    assert all(sol.guided_evaluations())
    assert not any(cls(num_steps=8, guide="unconditional", guidance=1.0).guided_evaluations())


@pytest.mark.parametrize("cls", [DeterministicSolver, StochasticSolver, MultistepSolver])
def test_solvers_reject_other_strings(cls):
    with pytest.raises(ValueError, match="unconditional"):
        cls(num_steps=8, guide="foo", guidance=2.0)
    sol = cls(num_steps=8, guide="unconditional", guidance=2.0)
    sol.guide = "uncond"            # a later assignment is checked at the next query (before any launch)
    with pytest.raises(ValueError, match="unconditional"):
        sol.guided_evaluations()


def test_generate_rejects_unconditional_with_a_guide_network(tmp_path, capsys):
    from tinyedm_amd.generate import main
    missing = str(tmp_path / "missing.ckpt")                 # never opened: the check runs first
    args = ["--ckpt_path", missing, "--output_dir", str(tmp_path / "out"), "--num_samples", "4", "--image_size", "32",
            "--num_classes", "10", "--batch_size", "4", "--guidance", "2", "--guide_unconditional"]
    with pytest.raises(SystemExit) as e:
        main(args + ["--guide_ckpt_path", missing])
    assert e.value.code == 2
    assert "--guide_unconditional" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        main(args + ["--guide_config_name", "cifar10"])
    assert e.value.code == 2
    assert not (tmp_path / "out").exists()


def test_generate_help_lists_the_flag(capsys):
    from tinyedm_amd.generate import main
    with pytest.raises(SystemExit):
        main(["--help"])
    assert "--guide_unconditional" in capsys.readouterr().out


def test_label_dropout_declared_in_header_and_lib():
    from tinyedm_amd import _lib
    with open(os.path.join(ROOT, "include", "tinyedm_hip.h")) as f:
        hdr = re.sub(r"\s+", " ", f.read())
    assert ("int edm_embed_combine_fwd(const float* emb_sigma, const float* wcls_hat, const long long* labels, float "
            "add_factor, int K, float* pre, float* out, int B, int E, unsigned long long drop_thr, unsigned long long "
            "seed, unsigned step, const void* dyn, const int* drop_in, int* drop_out, edm_stream_t stream);") in hdr
    assert "const int* drop, edm_stream_t stream);" in hdr
    assert len(_lib.SIGNATURES["edm_embed_combine_fwd"]) == 16
    assert len(_lib.SIGNATURES["edm_embed_combine_bwd"]) == 11
