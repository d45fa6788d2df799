"""Guided Heun sampling on the GPU (DeterministicSolver(guide=..., guidance=..., guidance_interval=...)):

 * the guided update kernels (solver_steps.hip) against an fp64 restatement, on the dwordx4 path, its scalar tail and the
   scalar path of a misaligned operand; w = 0 is bit-identical to the unguided update fed D_guide; a NaN raises the
   health bit;
 * guided trajectories of tiny nets against the CPU oracle composing D_guide + w*(D_main - D_guide) per sigma: CFG with
   an unconditional guide, autoguidance with a narrower conditional guide and an interval, and the fp32 eval path.
   Limits: 3x the unguided trajectory limits (bf16 1e-2, tests/test_network_gpu.py; f32 2e-4, tests/test_evalf32_gpu.py),
   since guidance scales the per-evaluation error by up to |w| + |1 - w| = 3 at w = 2;
 * guidance = 1 is the unguided solve, guidance = 0 the solve of the guide, bit for bit;
 * the hipGraph path: replays bit-identical to eager, a new guidance weight replays the same graph, a new interval
   or guide precision captures a new one;
 * the generate CLI end to end."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs
from parity_log import record

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _edm(P, ecfg, dcfg, dtype):
    """an eval-mode EDM on the GPU with the oracle's parameters (the _cifar pattern of tests/test_evalf32_gpu.py)"""
    import tinyedm_amd as T
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), dcfg.dropout_rate,
                     dcfg.sigma_data, dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    emb.load_state_dict({k[len("embedding."):]: v for k, v in P.items() if k.startswith("embedding.")}, strict=True)
    den.load_state_dict({k[len("denoiser."):]: v for k, v in P.items() if k.startswith("denoiser.")}, strict=True)
    den.set_eval_dtype(dtype)
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                  steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01)
    return model.to(DEV).eval()


def _narrow_cfgs():
    """a conditional guide of other widths than tiny_cfgs (autoguidance with a smaller network)"""
    e, d = tiny_cfgs(10)
    d = O.DenoiserCfg(in_channels=3, out_channels=3, encoder_block_types=list(d.encoder_block_types),
                      decoder_block_types=list(d.decoder_block_types), encoder_out_channels=[64, 64, 64],
                      decoder_out_channels=[64, 64, 64, 64, 64], skip_connections=list(d.skip_connections),
                      dropout_rate=0.0, sigma_data=0.5, embedding_dim=64, num_heads=2)
    return e, d


# ------------------------------------------------------------------ kernels
def _operands(n, offset, seed):
    g = torch.Generator().manual_seed(seed)
    # offset 1: every operand starts one float past a 16-byte boundary -> the kernels' scalar path
    return [torch.randn(n + 1, generator=g).to(DEV)[offset:offset + n] for _ in range(5)]


@pytest.mark.parametrize("n,offset", [(3 * 32 * 32 * 7, 0), (4099, 0), (4099, 1)],
                         ids=["n21504", "n4099-tail", "n4099-misaligned"])
def test_guided_updates_vs_fp64(ops, n, offset):
    x, Dm, Dg, Dm1, Dg1 = _operands(n, offset, n + offset)
    assert x.is_contiguous() and (x.data_ptr() % 16 == 0) == (offset == 0)
    t0, t1, w = 2.5, 1.7, 2.0
    w_dev = torch.full((1,), w, device=DEV)
    dx, x1 = ops.heun_euler_guided(x, Dm, Dg, w_dev, t0, t1)
    out = ops.heun_correct_guided(x, dx, x1, Dm1, Dg1, w_dev, t0, t1)
    ops.check_health(x.device, "guided updates")
    X, M, G, M1, G1 = (v.double().cpu() for v in (x, Dm, Dg, Dm1, Dg1))
    D = G + w * (M - G)
    dx_ref = (X - D) / t0
    x1_ref = X + (t1 - t0) * dx_ref
    D1 = G1 + w * (M1 - G1)
    dxc, x1c = dx.double().cpu(), x1.double().cpu()      # the correction restated on the kernel's own fp32 inputs
    out_ref = X + (t1 - t0) * (0.5 * dxc + 0.5 * (x1c - D1) / t1)
    for name, a, b in (("dx", dx, dx_ref), ("x1", x1, x1_ref), ("out", out, out_ref)):
        e = rel(a, b)
        assert e <= 2e-6, (name, e)

    # w = 0: value-identical to the unguided update fed D_guide
    w0 = torch.zeros(1, device=DEV)
    dx0, x10 = ops.heun_euler_guided(x, Dm, Dg, w0, t0, t1)
    dxu, x1u = ops.heun_euler(x, Dg, t0, t1)
    assert torch.equal(dx0, dxu) and torch.equal(x10, x1u)
    assert torch.equal(ops.heun_correct_guided(x, dxu, x1u, Dm1, Dg1, w0, t0, t1),
                       ops.heun_correct(x, dxu, x1u, Dg1, t0, t1))
    ops.check_health(x.device, "guided updates, w = 0")


def test_guided_updates_nonfinite_sets_health(ops):
    n = 4099
    x, Dm, Dg, Dm1, Dg1 = _operands(n, 0, 5)
    w_dev = torch.full((1,), 2.0, device=DEV)
    ops.check_health(x.device, "before")
    Dg[4097] = float("nan")                  # in the scalar tail
    ops.heun_euler_guided(x, Dm, Dg, w_dev, 2.5, 1.7)
    with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
        ops.check_health(x.device, "heun_euler_guided")
    Dg1[17] = float("nan")                   # in the dwordx4 body
    ops.heun_correct_guided(x, x, x, Dm1, Dg1, w_dev, 2.5, 1.7)
    with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
        ops.check_health(x.device, "heun_correct_guided")
    ops.check_health(x.device, "after")      # the read cleared the word


def test_guided_updates_reject_bad_operands(ops):
    x, Dm, Dg, _, _ = _operands(64, 0, 3)
    w_dev = torch.full((1,), 2.0, device=DEV)
    with pytest.raises(ValueError):
        ops.heun_euler_guided(x, Dm[:32], Dg, w_dev, 2.5, 1.7)
    with pytest.raises(TypeError):
        ops.heun_euler_guided(x, Dm, Dg.double(), w_dev, 2.5, 1.7)
    with pytest.raises(ValueError, match="w_dev"):
        ops.heun_euler_guided(x, Dm, Dg, torch.full((2,), 2.0, device=DEV), 2.5, 1.7)
    with pytest.raises(RuntimeError):
        ops.heun_euler_guided(x, Dm, Dg, torch.full((1,), 2.0), 2.5, 1.7)


# ------------------------------------------------------------------ trajectories vs the CPU oracle
def _oracle_guided(Pm, em, dm, Pg, eg, dg, w, interval, bf16):
    def D(x, s, labels):
        sig = s.reshape(-1).expand(x.shape[0])
        Dm = O.edm_forward(Pm, em, dm, x, sig, labels, bf16=bf16).float()
        if interval is not None and not (interval[0] < float(s) <= interval[1]):
            return Dm
        gl = labels if eg.num_classes is not None else None     # an unconditional EDM drops the labels
        Dg = O.edm_forward(Pg, eg, dg, x, sig, gl, bf16=bf16).float()
        return Dg + w * (Dm - Dg)
    return D


@pytest.mark.parametrize("case", ["cfg_bf16", "autoguidance_interval_bf16", "cfg_f32"])
def test_guided_trajectory_vs_oracle(ops, case):
    import tinyedm_amd as T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    em, dm = tiny_cfgs(10)
    Pm = O.init_params(em, dm, torch.Generator().manual_seed(7))
    if case.startswith("cfg"):
        eg, dg = tiny_cfgs(None)
        w, interval = 2.0, None
    else:
        eg, dg = _narrow_cfgs()
        w, interval = 2.5, (0.2, 7.0)
    Pg = O.init_params(eg, dg, torch.Generator().manual_seed(11))
    bf16 = not case.endswith("f32")
    dtype = "bf16" if bf16 else "f32"
    main, guide = _edm(Pm, em, dm, dtype), _edm(Pg, eg, dg, dtype)
    sol = T.DeterministicSolver(num_steps=5, sigma_min=0.01, sigma_max=20.0, rho=5.0, guide=guide, guidance=w,
                                guidance_interval=interval)
    flags = sol.guided_evaluations()
    assert any(flags) and (interval is None) == all(flags)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 3, 8, 8, generator=g)
    labels = torch.randint(0, 10, (2,), generator=g)
    x_hip = sol.solve(main, x0.to(DEV), labels.to(DEV)).cpu()
    t5 = O.karras_schedule(5, 0.01, 20.0, 5.0)
    with torch.no_grad():
        x_or = O.heun_solve(_oracle_guided(Pm, em, dm, Pg, eg, dg, w, interval, bf16), x0, t5, labels)
    e = rel(x_hip, x_or)
    lim = 3e-2 if bf16 else 6e-4
    record(f"guided/{case}_trajectory_vs_{'bf16' if bf16 else 'fp32'}_oracle", e, lim)
    assert e <= lim, e
    # the guidance must matter at this size: the unguided solve is far from the guided oracle
    x_main = T.DeterministicSolver(num_steps=5, sigma_min=0.01, sigma_max=20.0, rho=5.0).solve(
        main, x0.to(DEV), labels.to(DEV)).cpu()
    assert rel(x_main, x_or) > 5 * e


# ------------------------------------------------------------------ identities and the hipGraph path
@pytest.fixture(scope="module")
def pair(ops):
    em, dm = tiny_cfgs(10)
    eg, dg = tiny_cfgs(None)
    main = _edm(O.init_params(em, dm, torch.Generator().manual_seed(7)), em, dm, "bf16")
    guide = _edm(O.init_params(eg, dg, torch.Generator().manual_seed(11)), eg, dg, "bf16")
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(3, 3, 8, 8, generator=g).to(DEV)
    labels = torch.randint(0, 10, (3,), generator=g).to(DEV)
    return main, guide, x0, labels


def _solver(**kw):
    import tinyedm_amd as T
    return T.DeterministicSolver(num_steps=6, sigma_min=0.01, sigma_max=20.0, rho=5.0, **kw)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_guidance_one_is_the_unguided_solve(pair, graph):
    main, guide, x0, labels = pair
    calls = []
    spy = lambda x, s, c: calls.append(1) or guide(x, s, c)        # noqa: E731
    x_g = _solver(guide=spy, guidance=1.0, guidance_interval=(0.1, 5.0)).solve(main, x0, labels, graph=graph)
    x_u = _solver().solve(main, x0, labels, graph=graph)
    assert torch.equal(x_g, x_u)
    assert not calls


def test_guidance_zero_is_the_guide_solve(pair):
    main, guide, x0, labels = pair
    x_0 = _solver(guide=guide, guidance=0.0).solve(main, x0, labels)
    assert torch.equal(x_0, _solver().solve(guide, x0, labels))


def test_guided_hipgraph_replay_and_cache_key(pair):
    main, guide, x0, labels = pair
    sol = _solver(guide=guide, guidance=2.0)
    eager = sol.solve(main, x0, labels)
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager)
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager)           # pure replay
    assert len(sol._graphs[main]) == 1
    # a new guidance weight is a device value: same graph, new result
    sol.guidance = 3.5
    eager = sol.solve(main, x0, labels)
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager)
    assert len(sol._graphs[main]) == 1
    # a new interval changes which evaluations run the guide: a new capture
    sol.guidance_interval = (0.1, 5.0)
    eager = sol.solve(main, x0, labels)
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager)
    assert len(sol._graphs[main]) == 2
    # the guide's evaluation precision is part of the key
    guide.denoiser.set_eval_dtype("f32")
    try:
        eager = sol.solve(main, x0, labels)
        assert torch.equal(sol.solve(main, x0, labels, graph=True), eager)
        assert len(sol._graphs[main]) == 3
    finally:
        guide.denoiser.set_eval_dtype("bf16")


def test_guide_checks_before_launch(pair):
    main, _, x0, labels = pair
    em, _ = tiny_cfgs(10)
    _, d1 = tiny_cfgs(10)
    d1.out_channels = 1
    odd = _edm(O.init_params(em, d1, torch.Generator().manual_seed(2)), em, d1, "bf16")
    with pytest.raises(ValueError, match="channels"):
        _solver(guide=odd, guidance=2.0).solve(main, x0, labels)
    with pytest.raises(ValueError, match="training mode"):
        _solver(guide=torch.nn.Linear(2, 2).to(DEV).train(), guidance=2.0).solve(main, x0, labels)
    with pytest.raises(ValueError, match="on cpu"):
        _solver(guide=torch.nn.Linear(2, 2).eval(), guidance=2.0).solve(main, x0, labels)
    # guidance 1 never evaluates the guide, so nothing about it is checked
    _solver(guide=torch.nn.Linear(2, 2), guidance=1.0).solve(main, x0, labels)


# ------------------------------------------------------------------ generate CLI
def _generate(out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "generate.py"), "--config_name", "cifar10_cond",
           "--output_dir", str(out), "--num_samples", "4", "--batch_size", "4", "--num_steps", "3", "--num_classes",
           "10", "--image_size", "32", "--num_workers", "0", *extra]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def _pngs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_generate_cli_guidance(ops, tmp_path):
    from PIL import Image
    import tinyedm_amd as T
    from tinyedm_amd.config import compose, instantiate
    _generate(tmp_path / "plain")
    plain = _pngs(tmp_path / "plain")
    assert sorted(plain) == [f"{i}.png" for i in range(4)]
    # guidance 1 with a guide: the guide is unused and the images are byte-identical
    stdout = _generate(tmp_path / "w1", "--guide_config_name", "cifar10", "--guidance", "1")
    assert "unused" in stdout
    assert _pngs(tmp_path / "w1") == plain
    # guidance 2 with an unconditional guide from a checkpoint (gain_out away from its zero init: a random-init net's
    # output does not depend on its weights, so it could not change the samples)
    T.manual_seed(5)
    torch.manual_seed(5)
    guide = instantiate(compose("cifar10", os.path.join(ROOT, "experiments", "conf")).model)
    with torch.no_grad():
        guide.denoiser.gain_out.fill_(0.6)
    ckpt = str(tmp_path / "guide.ckpt")
    torch.save({"state_dict": {k: v.detach().cpu() for k, v in guide.state_dict().items()},
                "hyper_parameters": dict(guide.hparams)}, ckpt)
    _generate(tmp_path / "w2", "--guide_ckpt_path", ckpt, "--guidance", "2", "--guidance_interval", "0.1", "100")
    w2 = _pngs(tmp_path / "w2")
    assert sorted(w2) == sorted(plain)
    for f in w2:
        assert Image.open(tmp_path / "w2" / f).size == (32, 32)
    assert any(w2[f] != plain[f] for f in w2)
