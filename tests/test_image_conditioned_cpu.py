"""Image-conditioned sampling, host side (no GPU): the validation of start_step / image / mask / seed in solve() and of
invert(), all raised before a device is touched; multistep_coefficients(start_step=k); the generate CLI argument errors
and its PNG reader; the C ABI declarations of edm_state_init and edm_inpaint_blend."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tinyedm_amd import DeterministicSolver, MultistepSolver, StochasticSolver, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(x, sigma, labels):
    raise AssertionError("the model must not be evaluated on the host")


SOLVERS = {"heun": lambda **kw: DeterministicSolver(num_steps=8, **kw),
           "stochastic": lambda **kw: StochasticSolver(num_steps=8, S_churn=10.0, **kw),
           "multistep": lambda **kw: MultistepSolver(num_steps=8, order=3, **kw)}


@pytest.fixture(params=sorted(SOLVERS))
def sol(request):
    return SOLVERS[request.param]()


X0 = torch.zeros(2, 3, 8, 8)


@pytest.mark.parametrize("start", [-1, 8, 100, 1.0, "2", True, None])
def test_start_step_out_of_range(sol, start):
    with pytest.raises(ValueError, match="start_step"):
        sol.solve(_model, X0, start_step=start)


def test_mask_needs_image(sol):
    with pytest.raises(ValueError, match="image"):
        sol.solve(_model, X0, mask=torch.ones(8, 8, dtype=torch.bool))


@pytest.mark.parametrize("mask,match", [
    (torch.ones(2, 3, 8, 8), "shape"), (torch.ones(3, 1, 8, 8), "shape"), (torch.ones(8, 4), "shape"),
    (torch.ones(1, 8, 8), "shape"), (torch.ones(64), "shape"),
    (torch.ones(8, 8, dtype=torch.int32), "bool, uint8 or floating"), (torch.ones(8, 8, dtype=torch.int64), "bool"),
    (np.ones((8, 8), np.uint8), "tensor"), ([[1] * 8] * 8, "tensor"),
])
def test_bad_mask_rejected(sol, mask, match):
    with pytest.raises(ValueError, match=match):
        sol.solve(_model, X0, image=torch.zeros_like(X0), mask=mask)


@pytest.mark.parametrize("image", [torch.zeros(2, 3, 8, 4), torch.zeros(1, 3, 8, 8), torch.zeros(2, 3, 64),
                                   torch.zeros(2, 3, 8, 8, dtype=torch.int32), np.zeros((2, 3, 8, 8), np.float32)])
def test_bad_image_rejected(sol, image):
    with pytest.raises(ValueError, match="image"):
        sol.solve(_model, X0, image=image)
    with pytest.raises(ValueError, match="image"):
        sol.solve(_model, X0, image=image, start_step=3, mask=torch.ones(8, 8))


def test_mask_needs_four_dimensional_state(sol):
    x = torch.zeros(2, 192)
    with pytest.raises(ValueError, match="mask"):
        sol.solve(_model, x, image=torch.zeros_like(x), mask=torch.ones(8, 8))


@pytest.mark.parametrize("mask", [torch.ones(2, 1, 8, 8, dtype=torch.bool), torch.ones(1, 1, 8, 8, dtype=torch.uint8),
                                  torch.ones(8, 8), torch.ones(8, 8, dtype=torch.float64)])
def test_valid_arguments_reach_the_device_check(sol, mask):
    """every accepted mask format passes the host validation; what stops the call then is the missing GPU"""
    with pytest.raises(RuntimeError, match="GPU"):
        sol.solve(_model, X0, image=torch.zeros_like(X0), mask=mask, start_step=7)
    with pytest.raises(RuntimeError, match="GPU"):
        sol.solve(_model, X0, start_step=3)
    assert sol.solve_index == 0


def test_mask_is_converted_once_to_uint8():
    from tinyedm_amd.solvers import _mask_u8
    m = torch.zeros(8, 8)
    m[2:5, 1:7] = 0.25                          # non-zero = known
    for given, rows in ((m, 1), (m.bool().view(1, 1, 8, 8), 1), ((m != 0).to(torch.uint8).expand(2, 1, 8, 8) * 7, 2)):
        u = _mask_u8(given, (2, 3, 8, 8))
        assert u.dtype == torch.uint8 and u.shape == (rows, 64) and u.is_contiguous()
        assert torch.equal(u[0].view(8, 8), (m != 0).to(torch.uint8))


@pytest.mark.parametrize("name", sorted(SOLVERS))
@pytest.mark.parametrize("seed", [-1, 2 ** 64, 1.5, "7", True])
def test_bad_seed_rejected(name, seed):
    with pytest.raises(ValueError, match="seed"):
        SOLVERS[name](seed=seed)
    s = SOLVERS[name](seed=2 ** 64 - 1)
    assert s.seed == 2 ** 64 - 1 and s.solve_index == 0
    s.seed = seed
    with pytest.raises(ValueError, match="seed"):
        s.solve(_model, X0, image=torch.zeros_like(X0), mask=torch.ones(8, 8))
    s.seed, s.solve_index = 0, 2 ** 32
    with pytest.raises(ValueError, match="solve_index"):
        s.solve(_model, X0, image=torch.zeros_like(X0), mask=torch.ones(8, 8))


def test_seed_is_keyword_only_and_defaults_to_zero():
    for cls in (DeterministicSolver, MultistepSolver):
        a = cls(18, 0.002, 80.0, 7.0, None)
        assert (a.seed, a.solve_index) == (0, 0)
        with pytest.raises(TypeError):
            cls(18, 0.002, 80.0, 7.0, None, 5)
    assert DeterministicSolver(num_steps=18)._graph_key_extra() == ()
    assert DeterministicSolver(num_steps=18)._graph_key_extra(5) == ()


def test_invert_rejections():
    img = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="DeterministicSolver"):
        MultistepSolver(num_steps=8).invert(_model, img)
    with pytest.raises(ValueError, match="churn"):
        StochasticSolver(num_steps=8, S_churn=10.0).invert(_model, img)
    with pytest.raises(ValueError, match="churn"):
        StochasticSolver(num_steps=8, S_churn=10.0, S_min=0.5, S_max=2.0).invert(_model, img)
    for s in (DeterministicSolver(num_steps=8), StochasticSolver(num_steps=8),
              StochasticSolver(num_steps=8, S_churn=10.0, S_min=100.0, S_max=200.0)):      # no step is churned
        for end in (-1, 8, 1.0, True, None):
            with pytest.raises(ValueError, match="end_step"):
                s.invert(_model, img, end_step=end)
        with pytest.raises(ValueError, match="image"):
            s.invert(_model, img.int())
        with pytest.raises(RuntimeError, match="GPU"):
            s.invert(_model, img, end_step=7)
    assert "guided inversion is not implemented" in DeterministicSolver.invert.__doc__


def test_new_ops_have_no_cpu_path():
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.state_init(x, 1.0)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.state_init(x, 1.0, x)
    with pytest.raises(RuntimeError, match="CPU"):
        ops.inpaint_blend(x, x, torch.ones(1, 16, dtype=torch.uint8), 1.0, torch.zeros(4, dtype=torch.int32), 0)


# ------------------------------------------------------------------ multistep coefficients of a partial solve
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("k", [0, 1, 5, 16, 17])
def test_multistep_coefficients_restart_at_start_step(order, k):
    N = 18
    sol = MultistepSolver(num_steps=N, order=order)
    full, part = sol.multistep_coefficients(), sol.multistep_coefficients(start_step=k)
    assert part.dtype == torch.float32 and part.shape == (N, 4)
    assert torch.equal(sol.multistep_coefficients(start_step=0), full)
    first = MultistepSolver(num_steps=N, order=1).multistep_coefficients()
    assert torch.equal(part[k], first[k])                       # row k is first order
    assert not part[k, 2:].any()
    if order >= 2 and k + 1 < N - 1:
        second = MultistepSolver(num_steps=N, order=2).multistep_coefficients()
        assert torch.equal(part[k + 1], second[k + 1])          # then second ...
        assert part[k + 1, 2] != 0 and part[k + 1, 3] == 0
    assert torch.equal(part[k + order - 1:], full[k + order - 1:])       # ... and from k + order - 1 on the full rows
    assert part[-1].tolist() == [0.0, 1.0, 0.0, 0.0]
    ks = [s[0] for s in sol._steps(k)]
    assert ks[k:N - 1] == [min(order, i - k + 1) for i in range(k, N - 1)] and ks[-1] == 1


def test_multistep_coefficients_reject_bad_start_step():
    sol = MultistepSolver(num_steps=8, order=2)
    for bad in (-1, 8, 1.0, True):
        with pytest.raises(ValueError, match="start_step"):
            sol.multistep_coefficients(start_step=bad)
    assert sol._graph_key_extra() == sol._graph_key_extra(0) != sol._graph_key_extra(3)


# ------------------------------------------------------------------ generate CLI
ARGS = ["--config_name", "cifar10_cond", "--output_dir", "unused", "--num_samples", "4", "--image_size", "32",
        "--num_classes", "10", "--batch_size", "4", "--num_steps", "6"]


@pytest.mark.parametrize("extra,match", [
    (["--mask_box", "4", "4", "8", "8"], "--mask_box needs --init_dir"),
    (["--start_step", "2"], "--start_step needs --init_dir"),
    (["--invert_to", "lat.pt"], "--invert_to needs --init_dir"),
    (["--init_dir", "d", "--start_step", "6"], "--start_step must be below"),
    (["--init_dir", "d", "--start_step", "-1"], "--start_step"),
    (["--init_dir", "d", "--mask_box", "8", "4", "8", "12"], "--mask_box"),
    (["--init_dir", "d", "--mask_box", "0", "0", "33", "8"], "--mask_box"),
    (["--init_dir", "d", "--mask_box", "-1", "0", "8", "8"], "--mask_box"),
    (["--init_dir", "d", "--invert_to", "l.pt", "--solver", "dpmpp"], "--invert_to"),
    (["--init_dir", "d", "--invert_to", "l.pt", "--S_churn", "5"], "--invert_to"),
    (["--init_dir", "d", "--invert_to", "l.pt", "--mask_box", "0", "0", "8", "8"], "exclusive"),
])
def test_cli_argument_errors(capsys, extra, match):
    from tinyedm_amd.generate import main
    with pytest.raises(SystemExit) as e:
        main(ARGS + extra)
    assert e.value.code == 2                                    # an argparse error: nothing was loaded
    assert match in capsys.readouterr().err


def test_generate_function_rejects_the_same(tmp_path):
    from tinyedm_amd.generate import generate
    missing = str(tmp_path / "missing.ckpt")                    # never opened: the checks run first
    out = str(tmp_path / "out")
    with pytest.raises(ValueError, match="init_dir"):
        generate(missing, False, out, 4, 32, 10, 4, mask_box=(0, 0, 8, 8))
    with pytest.raises(ValueError, match="init_dir"):
        generate(missing, False, out, 4, 32, 10, 4, start_step=3)
    with pytest.raises(ValueError, match="mask_box"):
        generate(missing, False, out, 4, 32, 10, 4, init_dir=str(tmp_path), mask_box=(0, 0, 8, 40))
    assert not (tmp_path / "out").exists()


def test_generate_help_lists_conditioning_flags(capsys):
    from tinyedm_amd.generate import main
    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--init_dir", "--start_step", "--mask_box", "--invert_to"):
        assert re.search(rf"(^|\s){flag}(\s|$)", out, re.M), flag


def test_load_images_numeric_order_and_normalisation(tmp_path):
    from PIL import Image
    from tinyedm_amd.generate import load_images
    rng = np.random.default_rng(0)
    arrs = {i: rng.integers(0, 256, (8, 8, 3), dtype=np.uint8) for i in (0, 1, 2, 10, 11)}
    for i, a in arrs.items():
        Image.fromarray(a).save(tmp_path / f"{i}.png")
    mean, std = (0.5, 0.4, 0.3), (0.25, 0.2, 0.5)
    x = load_images(str(tmp_path), mean, std, 8, 3)
    assert x.shape == (5, 3, 8, 8) and x.dtype == torch.float32
    for row, i in enumerate(sorted(arrs)):                      # 2 before 10: numeric, not lexicographic
        # the inverse of the writer's clamp(x * std * 2 + mean, 0, 1) * 255 truncated: the centre of the level's bin
        ref = ((arrs[i].astype(np.float64).transpose(2, 0, 1) + 0.5) / 255.0 - np.array(mean)[:, None, None]) / \
            (2.0 * np.array(std)[:, None, None])
        assert np.abs(x[row].double().numpy() - ref).max() <= 1e-6
    Image.fromarray(arrs[0]).save(tmp_path / "grid.png")
    with pytest.raises(ValueError, match="index"):
        load_images(str(tmp_path), mean, std, 8, 3)
    os.remove(tmp_path / "grid.png")
    with pytest.raises(ValueError, match="expected uint8"):
        load_images(str(tmp_path), mean, std, 16, 3)


def test_datamodule_batches_carry_image_and_mask():
    from tinyedm_amd.datamodules import RandomNoiseDataModule
    imgs = torch.arange(5 * 3 * 4 * 4, dtype=torch.float32).view(5, 3, 4, 4)
    mask = torch.ones(4, 4, dtype=torch.uint8)
    plain = list(RandomNoiseDataModule(2, 0, 4, 5, 10, seed=3, device="cpu").predict_dataloader())
    cond = list(RandomNoiseDataModule(2, 0, 4, 5, 10, seed=3, device="cpu", images=imgs, mask=mask).predict_dataloader())
    assert [len(b) for b in plain] == [2, 2, 2] and [len(b) for b in cond] == [4, 4, 4]
    for i, (p, c) in enumerate(zip(plain, cond)):
        assert torch.equal(p[0], c[0]) and torch.equal(p[1], c[1])         # the same noise and labels
        assert torch.equal(c[2], imgs[2 * i:2 * i + 2]) and torch.equal(c[3], mask)
    with pytest.raises(ValueError, match="images"):
        RandomNoiseDataModule(2, 0, 4, 5, 10, device="cpu", images=imgs[:4])
    with pytest.raises(ValueError, match="mask"):
        RandomNoiseDataModule(2, 0, 4, 5, 10, device="cpu", mask=mask)


# ------------------------------------------------------------------ the C ABI
def test_new_entries_declared_in_header_and_lib():
    from tinyedm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    declared = set(re.findall(r"\b(edm_[a-z0-9_]+)\s*\(", hdr))
    for name in ("edm_state_init", "edm_inpaint_blend"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["edm_state_init"]) == 7 and len(_lib.SIGNATURES["edm_inpaint_blend"]) == 13
    assert "0x49500000" in hdr and "0x43480000" in hdr          # the blend's Philox tag is documented beside the churn's
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    exported = set(re.findall(r"\bT (edm_[a-z0-9_]+)", nm.stdout))
    assert {"edm_state_init", "edm_inpaint_blend"} <= exported
