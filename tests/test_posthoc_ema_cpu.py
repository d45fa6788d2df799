"""Post-hoc EMA reconstruction (tinyedm_amd/posthoc_ema.py) on the host: the fp64 least-squares math of EDM2 Appendix C
against an independent discrete recursion, the validation rules, and the CLI's parsing and output structure."""
import json

import numpy as np
import pytest
import torch

from tinyedm_amd import posthoc_ema as PH
from tinyedm_amd.ema import sigma_rel_to_gamma


def track(theta, sigma_rel):
    """the exact discrete recursion the optimizer kernel runs: p_t = beta_t p_{t-1} + (1 - beta_t) theta_t,
    beta_t = (1 - 1/t)^(gamma + 1), t = 1, 2, ... (fp64); -> the profile after every step, [T, D]"""
    g = sigma_rel_to_gamma(sigma_rel)
    p = np.zeros(theta.shape[1])
    out = np.empty_like(theta)
    for t in range(1, theta.shape[0] + 1):
        b = (1.0 - 1.0 / t) ** (g + 1)
        p = b * p + (1.0 - b) * theta[t - 1]
        out[t - 1] = p
    return out


def trajectory(T=4000, D=512, seed=0):
    rng = np.random.default_rng(seed)
    drift = rng.normal(size=D) * 0.01
    return np.cumsum(rng.normal(size=(T, D)) * 0.05 + drift, axis=0)


def test_tracked_profile_at_a_snapshot_is_recovered_exactly():
    steps = np.arange(200, 4001, 200)
    gams = [sigma_rel_to_gamma(s) for s in (0.05, 0.10)]
    snap_t = np.repeat(steps, 2)
    snap_g = np.tile(gams, len(steps))
    for k, g in enumerate(gams):
        for t_r in (steps[-1], steps[7]):
            x = PH.solve_coefficients(snap_t, snap_g, t_r, g)
            onehot = np.zeros_like(x)
            onehot[np.nonzero((snap_t == t_r) & (snap_g == g))[0]] = 1.0
            assert np.abs(x - onehot).max() < 1e-9, np.abs(x - onehot).max()


def test_untracked_lengths_interpolate_far_better_than_the_nearest_profile():
    T, every = 4000, 200
    theta = trajectory(T)
    tracked = (0.05, 0.10)
    prof = {s: track(theta, s) for s in tracked}
    steps = np.arange(every, T + 1, every)
    snap_t = np.repeat(steps, len(tracked))
    snap_g = np.tile([sigma_rel_to_gamma(s) for s in tracked], len(steps))
    snaps = np.stack([prof[s][t - 1] for t in steps for s in tracked])          # same order as snap_t / snap_g
    for target in (0.07, 0.13):
        direct = track(theta, target)[-1]
        x = PH.solve_coefficients(snap_t, snap_g, T, sigma_rel_to_gamma(target))
        rec = x @ snaps
        scale = np.linalg.norm(direct - theta[-1])
        err = np.linalg.norm(rec - direct) / scale
        nearest = min(tracked, key=lambda s: abs(s - target))
        err_near = np.linalg.norm(prof[nearest][-1] - direct) / scale
        assert err < 1e-2 and err * 20 < err_near, (target, err, err_near)
        assert abs(x.sum() - 1.0) < 1e-2                   # (not renormalised: close to 1 inside the tracked range)


def test_validation_rules():
    with pytest.raises(ValueError):
        PH.PostHocEMA(sigma_rels=(0.0,))
    with pytest.raises(ValueError):
        PH.PostHocEMA(sigma_rels=(0.05, 0.29))
    with pytest.raises(ValueError):
        PH.PostHocEMA(sigma_rels=(0.05, 0.06, 0.07, 0.08, 0.09))          # K > 4
    with pytest.raises(ValueError):
        PH.PostHocEMA(sigma_rels=())
    with pytest.raises(ValueError):
        PH.PostHocEMA(snapshot_every_n_steps=0)
    cb = PH.PostHocEMA(sigma_rels=[0.05, 0.10, 0.2886], snapshot_every_n_steps=10)
    assert len(cb.gammas) == 3 and cb.gammas[2] >= 0
    g = sigma_rel_to_gamma(0.1)
    with pytest.raises(ValueError, match="not the step of a snapshot"):
        PH.solve_coefficients([100, 200], [g, g], 300, g)                  # after the last snapshot
    with pytest.raises(ValueError, match="not the step of a snapshot"):
        PH.solve_coefficients([100, 200], [g, g], 150, g)
    with pytest.raises(ValueError):
        PH.solve_coefficients([], [], 100, g)


def test_plan_rejects_empty_dirs_too_many_lengths_and_bad_lengths(tmp_path):
    with pytest.raises(ValueError):
        PH.plan(tmp_path, [0.1])                                            # no snapshot files
    with pytest.raises(ValueError):
        PH.plan(tmp_path / "absent", [0.1])
    _fake_snapshots(tmp_path, steps=(10, 20))
    with pytest.raises(ValueError):
        PH.plan(tmp_path, [0.05 + 0.01 * i for i in range(9)])               # L > 8
    with pytest.raises(ValueError):
        PH.plan(tmp_path, [0.3])
    with pytest.raises(ValueError):
        PH.plan(tmp_path, [0.1], step=15)
    snaps, t_r, coef = PH.plan(tmp_path, [0.07, 0.12])
    assert t_r == 20 and coef.shape == (2, 2, 2) and [s for s, _, _ in snaps] == [10, 20]


def test_large_gamma_and_step_give_finite_coefficients():
    g_small = sigma_rel_to_gamma(0.01)
    assert 90 < g_small < 100
    steps = np.linspace(1e6, 1e7, 10).round()
    snap_t = np.repeat(steps, 2)
    snap_g = np.tile([g_small, sigma_rel_to_gamma(0.2)], len(steps))
    for target in (0.01, 0.05, 0.2):
        x = PH.solve_coefficients(snap_t, snap_g, 1e7, sigma_rel_to_gamma(target))
        assert np.all(np.isfinite(x)) and abs(x.sum() - 1.0) < 0.1, (target, x.sum())


def _fake_snapshots(d, steps, shapes=((3, 2), (5,)), sigma_rels=(0.05, 0.10)):
    g = torch.Generator().manual_seed(0)
    gam = [float(sigma_rel_to_gamma(s)) for s in sigma_rels]
    for s in steps:
        torch.save({"step": s, "global_step": s, "sigma_rels": list(sigma_rels), "gammas": gam,
                    "profiles": [tuple(torch.randn(sh, generator=g) for sh in shapes) for _ in sigma_rels]},
                   PH.snapshot_path(d, s))


def test_cli_arguments_and_output_checkpoint_structure(tmp_path):
    a = PH.build_parser().parse_args(["--ckpt_path", "last.ckpt", "--snapshot_dir", "phema", "--ema_length", "0.07",
                                      "0.13", "--step", "400", "--out_dir", "out"])
    assert a.ema_length == [0.07, 0.13] and a.step == 400 and a.snapshot_dir == "phema" and a.device == "cuda"
    assert PH.build_parser().parse_args(["--ckpt_path", "c", "--snapshot_dir", "s", "--ema_length", "0.1",
                                         "--out_dir", "o"]).step is None
    with pytest.raises(SystemExit):
        PH.build_parser().parse_args(["--ckpt_path", "c", "--snapshot_dir", "s", "--out_dir", "o"])
    # the output writer from CPU-resident reconstructions (the GPU assembly is covered by tests/test_posthoc_ema_gpu.py)
    old_ema = (torch.zeros(3, 2), torch.zeros(5))
    ckpt = {"state_dict": {"w": torch.ones(3, 2)}, "hyper_parameters": {"x": 1}, "global_step": 20,
            "optimizer_states": [{"opt": {"m": torch.zeros(8)}, "ema": old_ema, "current_step": 20}]}
    recon = [(torch.full((3, 2), 1.0), torch.full((5,), 2.0)), (torch.full((3, 2), 3.0), torch.full((5,), 4.0))]
    coef = np.arange(8, dtype=np.float64).reshape(2, 2, 2)
    paths = PH.write_outputs(ckpt, [0.07, 0.13], recon, 20, [10, 20], coef, tmp_path / "out")
    assert [p.name for p in paths] == ["phema-0.0700-step0000000020.ckpt", "phema-0.1300-step0000000020.ckpt"]
    for p, r, l in zip(paths, recon, range(2)):
        ck = torch.load(p, weights_only=False)
        assert set(ck) == set(ckpt)
        assert ck["optimizer_states"][0]["current_step"] == 20 and "opt" in ck["optimizer_states"][0]
        assert all(torch.equal(a, b) for a, b in zip(ck["optimizer_states"][0]["ema"], r))
        meta = json.loads(p.with_suffix(".json").read_text())
        assert meta["t_r"] == 20 and meta["snapshot_steps"] == [10, 20]
        assert np.allclose(meta["coefficients"], coef[..., l]) and abs(meta["coefficient_sum"] - coef[..., l].sum()) < 1e-12
    assert ckpt["optimizer_states"][0]["ema"] is old_ema                     # the source is not modified
    # a checkpoint without optimizer state gets one holding just the EMA
    p = PH.write_outputs({"state_dict": {}}, [0.1], recon[:1], 20, [10, 20], coef[..., :1], tmp_path / "o2")[0]
    assert len(torch.load(p, weights_only=False)["optimizer_states"][0]["ema"]) == 2


def test_shim_module_resolves():
    import tinyedm.posthoc_ema as S
    from tinyedm_amd.config import instantiate
    cb = instantiate({"_target_": "tinyedm.posthoc_ema.PostHocEMA", "sigma_rels": [0.05, 0.1],
                      "snapshot_every_n_steps": 7, "snapshot_dir": "x"})
    assert isinstance(cb, S.PostHocEMA) and cb.snapshot_every_n_steps == 7
