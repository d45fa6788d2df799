"""Post-hoc EMA on the GPU (tinyedm_amd/posthoc_ema.py, csrc/optim.hip): edm_adam_ema_phema against edm_adam_ema
(theta / m / v bitwise, the main EMA to fp32 rounding) and an fp64 recursion, edm_phema_accumulate against numpy fp64, profile tracking through the eager and the
hipGraph-replayed step, resume, the unchanged default step, and reconstruction end to end through the CLI, the
checkpoint loader and `generate --load_ema`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("with_ema,zero_grad", [(True, True), (False, False), (True, False)])
def test_adam_ema_phema_matches_adam_ema_bitwise_and_fp64_profiles(K, with_ema, zero_grad):
    from tinyedm_amd import ops
    _need_gpu()
    n = 4099                                         # odd: the scalar tail runs
    g = torch.Generator().manual_seed(K)
    theta0 = torch.randn(n, generator=g).to(DEV)
    m0 = 0.1 * torch.randn(n, generator=g).to(DEV)
    v0 = torch.rand(n, generator=g).to(DEV) * 0.01
    ema0 = torch.randn(n, generator=g).to(DEV)
    prof = [torch.randn(n, generator=g).to(DEV) for _ in range(K)]
    ref = {"theta": theta0.clone(), "m": m0.clone(), "v": v0.clone(), "ema": ema0.clone()}
    new = {"theta": theta0.clone(), "m": m0.clone(), "v": v0.clone(), "ema": ema0.clone()}
    p64 = [p.double().cpu() for p in prof]
    betas = torch.zeros(K, device=DEV)
    for step in range(1, 4):
        grad = torch.randn(n, generator=g).to(DEV)
        grad_r, grad_n = grad.clone(), grad.clone()
        # new betas written into the SAME device array between launches (what a graph replay sees)
        b_host = torch.tensor([0.5 + 0.1 * k + 0.05 * step for k in range(K)], dtype=torch.float32)
        betas.copy_(b_host)
        args = (1e-2, 0.9, 0.99, 1e-8, step, 0.97, 0.5)
        ops.adam_ema(ref["theta"], grad_r, ref["m"], ref["v"], ref["ema"] if with_ema else None, *args,
                     zero_grad=zero_grad)
        ops.adam_ema_phema(new["theta"], grad_n, new["m"], new["v"], new["ema"] if with_ema else None, prof, betas,
                           *args, zero_grad=zero_grad)
        torch.cuda.synchronize()
        for k in ("theta", "m", "v"):
            assert torch.equal(ref[k], new[k]), (k, step)
        # the main EMA: the same expression, but the compiler contracts b*e + (1-b)*t into an FMA on different lanes in
        # the two kernels -> equal to the rounding of its two terms (accumulated over the steps)
        tol = 2 * step * torch.finfo(torch.float32).eps * (ref["ema"].abs() + ref["theta"].abs())
        assert bool(((ref["ema"] - new["ema"]).abs() <= tol).all()), step
        assert torch.equal(grad_r, grad_n)
        assert bool((grad_n == 0).all()) == zero_grad
        th = new["theta"].double().cpu()
        for k in range(K):
            b = float(b_host[k])
            p64[k] = b * p64[k] + (1.0 - b) * th
            err = (prof[k].double().cpu() - p64[k]).abs().max().item()
            assert err <= 4e-7 * max(1.0, p64[k].abs().max().item()), (k, step, err)


def test_adam_ema_phema_validates():
    from tinyedm_amd import ops
    _need_gpu()
    t = torch.zeros(64, device=DEV)
    with pytest.raises(ValueError):
        ops.adam_ema_phema(t, t.clone(), t.clone(), t.clone(), None, [t.clone() for _ in range(5)],
                           torch.zeros(5, device=DEV), 1e-3, 0.9, 0.99, 1e-8, 1, 0.0)
    with pytest.raises(ValueError):
        ops.adam_ema_phema(t, t.clone(), t.clone(), t.clone(), None, [torch.zeros(32, device=DEV)],
                           torch.zeros(1, device=DEV), 1e-3, 0.9, 0.99, 1e-8, 1, 0.0)
    with pytest.raises(ValueError):
        ops.phema_accumulate(torch.zeros(9, 16, device=DEV, dtype=torch.float64), torch.zeros(16, device=DEV), [0.0] * 9)


@pytest.mark.parametrize("L,n", [(1, 1003), (8, 1003), (8, 4096), (3, 4096)])
def test_phema_accumulate_matches_fp64(L, n):
    from tinyedm_amd import ops
    _need_gpu()
    rng = np.random.default_rng(L * n)
    acc = torch.zeros(L, n, device=DEV, dtype=torch.float64)
    ref = np.zeros((L, n))
    for _ in range(40):
        s = rng.normal(size=n).astype(np.float32)
        w = rng.uniform(-3, 3, size=L)
        ops.phema_accumulate(acc, torch.from_numpy(s).to(DEV), w)
        ref += w[:, None] * s.astype(np.float64)[None, :]
    got = acc.cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    out = ops.phema_finish(acc)
    assert out.dtype == torch.float32 and torch.equal(out.cpu(), torch.from_numpy(got.astype(np.float32)))


# ------------------------------------------------------------------ tracking during training
def _tiny_model(seed=7):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_trainer_gpu import build_model
    model, *_ = build_model(seed=seed)
    return model.to(DEV)


def _batches(n=6):
    from test_trainer_gpu import Batches
    return Batches(n=n)


def _base(trainer):
    from tinyedm_amd.ema import EMAOptimizer
    o = trainer.optimizers[0]
    return o.optimizer if isinstance(o, EMAOptimizer) else o


def _recorder():
    """callback (placed after PostHocEMA) recording theta and the profiles after every optimizer step"""
    class Rec:
        def __init__(self):
            self.theta, self.prof = [], []

        def on_train_batch_end(self, trainer, pl_module, outputs, batch, batch_idx):
            b = _base(trainer)
            self.theta.append(b.arena.theta.double().cpu())
            self.prof.append(b.phema.arenas.double().cpu())
    return Rec()


@pytest.mark.parametrize("graph", ["0", "1"])
def test_profiles_follow_the_fp64_recursion_of_the_trained_weights(tmp_path, monkeypatch, graph):
    import tinyedm_amd as T
    from tinyedm_amd.posthoc_ema import PostHocEMA
    _need_gpu()
    monkeypatch.setenv("EDM_GRAPH", graph)
    cb = PostHocEMA(sigma_rels=(0.05, 0.10), snapshot_every_n_steps=4, snapshot_dir=str(tmp_path / "phema"))
    rec = _recorder()
    tr = T.Trainer(max_epochs=2, max_steps=12, callbacks=[cb, rec])
    tr.fit(_tiny_model(), train_dataloaders=_batches())
    assert tr.step_launch == ("hipGraph replay" if graph == "1" else "eager loop")
    b = _base(tr)
    assert b.phema.count == 12 and len(rec.theta) == 12
    p = rec.theta[0].unsqueeze(0).repeat(2, 1)
    for t in range(1, 13):
        betas = torch.tensor(np.array(b.phema.beta_values(t), dtype=np.float64))      # (the fp32 betas the kernel read)
        p = betas[:, None] * p + (1 - betas[:, None]) * rec.theta[t - 1][None, :]
        err = (rec.prof[t - 1] - p).abs().max().item()
        assert err <= 1e-6 * max(1.0, p.abs().max().item()), (t, err)
    files = sorted(os.listdir(tmp_path / "phema"))
    assert files == [f"phema-{s:010d}.pt" for s in (4, 8, 12)]
    sd = torch.load(tmp_path / "phema" / files[-1], weights_only=True)
    assert sd["step"] == 12 and sd["gammas"] == list(cb.gammas)
    live = cb.profiles
    for k in range(2):
        assert len(sd["profiles"][k]) == len(b.arena.params)
        assert all(torch.equal(a, l.cpu()) for a, l in zip(sd["profiles"][k], live[k]))


def test_eager_and_replayed_training_track_the_same_profiles(tmp_path):
    """the MNIST config through experiments/train.py with two profiles, EDM_GRAPH=0 vs 1: same snapshot sequence;
    the profiles agree to the tolerance the captured and the eager step agree to (tests/test_graph_gpu.py: the step
    itself is not bitwise reproducible across the two launch forms -- float atomics in the reductions)"""
    _need_gpu()
    runs = {}
    for graph in ("0", "1"):
        out = tmp_path / f"g{graph}"
        out.mkdir()
        cmd = [sys.executable, os.path.join(ROOT, "experiments", "train.py"), "--config-name=mnist",
               "trainer.max_epochs=1", "+trainer.max_steps=24", "trainer.check_val_every_n_epoch=100",
               "datamodule.batch_size=16", "datamodule.num_samples=512", f"callbacks.checkpoint_callback.dirpath={out}",
               "callbacks.generate_callback.every_n_epochs=100",
               "callbacks.posthoc_ema={_target_: tinyedm.posthoc_ema.PostHocEMA, sigma_rels: [0.05, 0.10], "
               f"snapshot_every_n_steps: 8, snapshot_dir: {out / 'phema'}}}"]
        env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", EDM_GRAPH=graph)
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=str(out))
        assert r.returncode == 0, r.stderr[-3000:]
        runs[graph] = out / "phema"
    f0, f1 = sorted(os.listdir(runs["0"])), sorted(os.listdir(runs["1"]))
    assert f0 == f1 == [f"phema-{s:010d}.pt" for s in (8, 16, 24)]
    for f in f0:
        a = torch.load(runs["0"] / f, weights_only=True)
        b = torch.load(runs["1"] / f, weights_only=True)
        assert a["step"] == b["step"] and a["gammas"] == b["gammas"]
        for pa, pb in zip(a["profiles"], b["profiles"]):
            e = rel(torch.cat([t.reshape(-1) for t in pb]), torch.cat([t.reshape(-1) for t in pa]))
            assert e <= 2e-3, (f, e)


def test_resume_continues_profiles_and_snapshots(tmp_path, monkeypatch):
    import tinyedm_amd as T
    from tinyedm_amd.posthoc_ema import PostHocEMA
    _need_gpu()
    monkeypatch.setenv("EDM_GRAPH", "1")
    data = _batches(n=12)
    mk = lambda d: PostHocEMA(sigma_rels=(0.05, 0.10), snapshot_every_n_steps=2, snapshot_dir=str(d))
    tA = T.Trainer(max_epochs=1, max_steps=8, callbacks=[mk(tmp_path / "A")])
    tA.fit(_tiny_model(), train_dataloaders=data)
    tB = T.Trainer(max_epochs=1, max_steps=4, callbacks=[mk(tmp_path / "B")])
    tB.fit(_tiny_model(), train_dataloaders=data)
    tB._batch_in_epoch = 4
    path = str(tmp_path / "mid.ckpt")
    tB.save_checkpoint(path)
    ck = torch.load(path, weights_only=False)
    assert ck["optimizer_states"][0]["opt"]["phema"]["count"] == 4
    T.manual_seed(999)
    tC = T.Trainer(max_epochs=1, max_steps=8, callbacks=[mk(tmp_path / "B")])
    tC.fit(_tiny_model(seed=8), train_dataloaders=data, ckpt_path=path)
    assert _base(tC).phema.count == _base(tA).phema.count == 8
    assert rel(_base(tC).phema.arenas, _base(tA).phema.arenas) <= 1e-4
    fa, fb = sorted(os.listdir(tmp_path / "A")), sorted(os.listdir(tmp_path / "B"))
    assert fa == fb == [f"phema-{s:010d}.pt" for s in (2, 4, 6, 8)]
    for f in fa:
        a, b = (torch.load(tmp_path / d / f, weights_only=True) for d in ("A", "B"))
        assert a["step"] == b["step"] and a["global_step"] == b["global_step"]
        for pa, pb in zip(a["profiles"], b["profiles"]):
            assert rel(torch.cat([t.reshape(-1) for t in pb]), torch.cat([t.reshape(-1) for t in pa])) <= 1e-4
    # a checkpoint without profile state cannot be resumed with tracking on
    tD = T.Trainer(max_epochs=1, max_steps=2)
    tD.fit(_tiny_model(), train_dataloaders=data)
    plain = str(tmp_path / "plain.ckpt")
    tD.save_checkpoint(plain)
    tE = T.Trainer(max_epochs=1, max_steps=4, callbacks=[mk(tmp_path / "E")])
    with pytest.raises(ValueError, match="no profile state"):
        tE.fit(_tiny_model(), train_dataloaders=data, ckpt_path=plain)


@pytest.mark.parametrize("graph", ["0", "1"])
def test_without_the_callback_the_step_and_checkpoint_are_unchanged(tmp_path, monkeypatch, graph):
    import tinyedm_amd as T
    from tinyedm_amd import _lib
    _need_gpu()
    monkeypatch.setenv("EDM_GRAPH", graph)
    names = []
    real = _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", spy)
    tr = T.Trainer(max_epochs=1, max_steps=5)
    tr.fit(_tiny_model(), train_dataloaders=_batches())
    monkeypatch.setattr(_lib, "call", real)
    assert "edm_adam_ema" in names and not any("phema" in n for n in names)
    assert _base(tr).phema is None
    ck = tr.save_checkpoint(str(tmp_path / "c.ckpt"))
    assert set(ck["optimizer_states"][0]) == {"opt", "ema", "current_step", "gamma", "every_n_steps"}
    assert set(ck["optimizer_states"][0]["opt"]) == {"m", "v", "step", "layout", "offsets", "numels", "param_groups"}


# ------------------------------------------------------------------ reconstruction end to end
def test_reconstruction_end_to_end(tmp_path, monkeypatch):
    import tinyedm_amd as T
    from tinyedm_amd import posthoc_ema as PH
    from tinyedm_amd.ema import sigma_rel_to_gamma
    _need_gpu()
    monkeypatch.setenv("EDM_GRAPH", "1")
    snapdir = tmp_path / "phema"
    cb = PH.PostHocEMA(sigma_rels=(0.05, 0.10), snapshot_every_n_steps=3, snapshot_dir=str(snapdir))
    tr = T.Trainer(max_epochs=3, max_steps=15, callbacks=[cb])
    tr.fit(_tiny_model(), train_dataloaders=_batches())
    ckpt = str(tmp_path / "last.ckpt")
    tr.save_checkpoint(ckpt)
    last = torch.load(PH.snapshot_path(snapdir, 15), weights_only=True)
    # a tracked length at the last snapshot is that snapshot (to fp32 rounding of the coefficients' sum)
    rec = PH.reconstruct(snapdir, [0.10, 0.05])
    for r, k in zip(rec, (1, 0)):
        for a, b in zip(r, last["profiles"][k]):
            assert torch.allclose(a.cpu(), b, rtol=1e-6, atol=1e-6)
    # an untracked length equals the numpy fp64 combination of the same files
    snaps, t_r, coef = PH.plan(snapdir, [0.07], step=12)
    assert t_r == 12 and coef.shape == (5, 2, 1)
    ref = None
    for i, (s, path, _) in enumerate(snaps):
        sd = torch.load(path, weights_only=True)
        for k, prof in enumerate(sd["profiles"]):
            flat = torch.cat([t.reshape(-1) for t in prof]).double().numpy()
            ref = coef[i, k, 0] * flat if ref is None else ref + coef[i, k, 0] * flat
    got = torch.cat([t.reshape(-1) for t in PH.reconstruct(snapdir, [0.07], step=12)[0]]).double().cpu().numpy()
    assert np.linalg.norm(got - ref) <= 1e-6 * np.linalg.norm(ref)
    assert abs(coef.sum() - 1.0) < 5e-2
    # CLI -> checkpoint -> EDM.load_from_checkpoint(load_ema=True) and generate --load_ema
    out = tmp_path / "out"
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "-m", "tinyedm.posthoc_ema", "--ckpt_path", ckpt, "--snapshot_dir", str(snapdir),
                        "--ema_length", "0.07", "0.13", "--out_dir", str(out)], capture_output=True, text=True,
                       env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    made = out / "phema-0.0700-step0000000015.ckpt"
    assert made.exists() and (out / "phema-0.1300-step0000000015.ckpt").exists()
    ck = torch.load(made, weights_only=False)
    src = torch.load(ckpt, weights_only=False)
    assert set(ck) == set(src) and len(ck["optimizer_states"][0]["ema"]) == len(src["optimizer_states"][0]["ema"])
    ref07 = PH.reconstruct(snapdir, [0.07])[0]
    assert all(torch.equal(a, b.cpu()) for a, b in zip(ck["optimizer_states"][0]["ema"], ref07))
    m = T.EDM.load_from_checkpoint(str(made), load_ema=True)
    for p, e in zip(m.parameters(), ref07):
        assert torch.equal(p.detach().cpu(), e.cpu())
    gen = tmp_path / "gen"
    r = subprocess.run([sys.executable, "-m", "tinyedm.generate", "--ckpt_path", str(made), "--load_ema", "--output_dir",
                        str(gen), "--num_samples", "3", "--image_size", "8", "--num_classes", "10", "--batch_size", "4",
                        "--num_workers", "0", "--num_steps", "3"], capture_output=True, text=True, env=env,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(gen)) == ["0.png", "1.png", "2.png"]
