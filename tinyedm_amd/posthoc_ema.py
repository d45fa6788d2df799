"""Post-hoc EMA (Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models", Sec. 3 and
Appendix C): track K power-function EMA profiles during training, snapshot them every N steps, and afterwards rebuild
the EMA of ANY length sigma_rel as a least-squares combination of the snapshots.

Training: ``PostHocEMA(sigma_rels=(0.05, 0.10), snapshot_every_n_steps=2000, snapshot_dir="phema")`` is a callback.  It
attaches the profile arenas to the FusedAdam (ema.PowerProfiles): the fused optimizer kernel updates them in the same
pass (edm_adam_ema_phema), eager and hipGraph-replayed steps alike.  Without the callback nothing changes.

Reconstruction::

    python -m tinyedm.posthoc_ema --ckpt_path last.ckpt --snapshot_dir phema --ema_length 0.07 0.13 --out_dir out

writes one checkpoint per length (the source checkpoint with ``optimizer_states[0]["ema"]`` replaced by the
reconstruction) that ``generate --load_ema`` and ``EDM.load_from_checkpoint(load_ema=True)`` read unchanged.
"""
from __future__ import annotations

import argparse
import copy
import json
import math
import os
import re
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np
import torch

from .ema import EMAOptimizer, FusedAdam, sigma_rel_to_gamma

SIGMA_REL_MAX = 0.2886          # sigma_rel of gamma = 0 (the longest power-function EMA): sqrt(1/12)
MAX_PROFILES = 4                # tracked per run (edm_adam_ema_phema)
MAX_LENGTHS = 8                 # reconstructed per pass over the snapshots (edm_phema_accumulate)
_FILE = re.compile(r"^phema-(\d{10})\.pt$")


def check_sigma_rel(s) -> float:
    s = float(s)
    if not (0.0 < s <= SIGMA_REL_MAX) or not math.isfinite(s):
        raise ValueError(f"post-hoc EMA: sigma_rel must lie in (0, {SIGMA_REL_MAX}], got {s}")
    return s


def snapshot_path(snapshot_dir, step: int) -> Path:
    return Path(snapshot_dir) / f"phema-{int(step):010d}.pt"


# ------------------------------------------------------------------ training side
class PostHocEMA:
    """Callback: K = len(sigma_rels) power-function profiles, one snapshot file every `snapshot_every_n_steps` profile
    updates (rank 0).  A snapshot file holds {step, global_step, sigma_rels, gammas, profiles}: `profiles[k]` is a tuple
    of per-parameter fp32 tensors in the order of EMAOptimizer.ema_params (independent of the arena layout).  The copy
    to the host goes through a device staging buffer and pinned memory on a side stream; the file is written at the
    next hook, so the step stream never waits for it.  Disk: 4 bytes per parameter per profile per snapshot (CIFAR-10
    net: 142 MB, ImageNet net: 1.09 GB)."""

    def __init__(self, sigma_rels: Sequence[float] = (0.05, 0.10), snapshot_every_n_steps: int = 2000,
                 snapshot_dir: str = "phema"):
        sigma_rels = [check_sigma_rel(s) for s in sigma_rels]
        if not 1 <= len(sigma_rels) <= MAX_PROFILES:
            raise ValueError(f"post-hoc EMA: 1 to {MAX_PROFILES} tracked lengths, got {len(sigma_rels)}")
        if int(snapshot_every_n_steps) != snapshot_every_n_steps or int(snapshot_every_n_steps) < 1:
            raise ValueError(f"post-hoc EMA: snapshot_every_n_steps must be an integer >= 1, got {snapshot_every_n_steps}")
        self.sigma_rels = tuple(sigma_rels)
        self.gammas = tuple(float(sigma_rel_to_gamma(s)) for s in sigma_rels)
        self.snapshot_every_n_steps = int(snapshot_every_n_steps)
        self.snapshot_dir = Path(snapshot_dir)
        self.base: Optional[FusedAdam] = None
        self._pending = None
        self._stage = self._pinned = self._stream = None

    @staticmethod
    def _base(trainer) -> FusedAdam:
        opt = trainer.optimizers[0]
        base = opt.optimizer if isinstance(opt, EMAOptimizer) else opt
        if not isinstance(base, FusedAdam):
            raise TypeError("PostHocEMA needs the flat-arena tinyedm_amd FusedAdam")
        return base

    def on_fit_start(self, trainer, pl_module):
        base = self._base(trainer)
        if base.phema is None or base.phema.gammas != self.gammas:
            base.attach_profiles(self.gammas)
        self.base = base

    @property
    def profiles(self):
        """-> [K] tuples of per-parameter device views of the live profiles (EMAOptimizer.ema_params order)"""
        a = self.base.arena
        return [tuple(row[o:o + p.numel()].view_as(p) for p, o in zip(a.params, a.offsets)) for row in self.base.phema.arenas]

    def on_train_batch_end(self, trainer, pl_module, outputs, batch, batch_idx):
        self.flush()
        ph = self.base.phema
        if ph.count % self.snapshot_every_n_steps == 0 and getattr(trainer, "global_rank", 0) == 0:
            self._start(ph.count, trainer.global_step)

    def _start(self, step, global_step):
        """device copy of the profiles (stream-ordered after the step), then device -> pinned host on a side stream"""
        arenas = self.base.phema.arenas
        if self._stage is None or self._stage.shape != arenas.shape:
            self._stage = torch.empty_like(arenas)
            self._pinned = torch.empty(arenas.shape, dtype=arenas.dtype).pin_memory()
            self._stream = torch.cuda.Stream(arenas.device)
        self._stage.copy_(arenas)
        cur = torch.cuda.current_stream(arenas.device)
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            self._pinned.copy_(self._stage, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self._pending = (ev, int(step), int(global_step))

    def flush(self):
        """write the snapshot whose copy is in flight, if any"""
        if self._pending is None:
            return
        ev, step, global_step = self._pending
        self._pending = None
        ev.synchronize()
        a = self.base.arena
        profiles = [tuple(row[o:o + p.numel()].view(p.shape).clone() for p, o in zip(a.params, a.offsets))
                    for row in self._pinned]
        self.snapshot_dir.mkdir(parents=True, exist_ok=True)
        path = snapshot_path(self.snapshot_dir, step)
        tmp = path.with_suffix(".tmp")
        torch.save({"step": step, "global_step": global_step, "sigma_rels": list(self.sigma_rels),
                    "gammas": list(self.gammas), "profiles": profiles}, tmp)
        os.replace(tmp, path)

    def on_train_epoch_end(self, trainer, pl_module):
        self.flush()

    def on_validation_start(self, trainer, pl_module):
        self.flush()

    def on_fit_end(self, trainer, pl_module):
        self.flush()


# ------------------------------------------------------------------ reconstruction math (fp64, host)
def log_profile_inner(t_a, g_a, t_b, g_b):
    """log <p_a, p_b> of two continuous power-function EMA profiles, p(tau) = (g+1) tau^g / t^(g+1) on [0, t] (EDM2
    Appendix C.3): (g_a+1)(g_b+1)/(g_a+g_b+1) * t_min^(g_a+g_b+1) / (t_a^(g_a+1) t_b^(g_b+1)), in log space (gamma
    reaches ~100 and t millions of steps: the direct powers overflow)"""
    t_a, g_a, t_b, g_b = (np.asarray(x, dtype=np.float64) for x in (t_a, g_a, t_b, g_b))
    t_min = np.minimum(t_a, t_b)
    return (np.log(g_a + 1) + np.log(g_b + 1) - np.log(g_a + g_b + 1) + (g_a + g_b + 1) * np.log(t_min)
            - (g_a + 1) * np.log(t_a) - (g_b + 1) * np.log(t_b))


def solve_coefficients(snap_t, snap_gamma, t_r, gamma_r) -> np.ndarray:
    """Least-squares weights x of the snapshot profiles (step snap_t[i], exponent snap_gamma[i]) that best match the
    profile (t_r, gamma_r): A x = b with A_ij = <p_i, p_j>, b_i = <p_i, p_r> (EDM2 Appendix C.3, no renormalisation).
    t_r must be the step of a snapshot; snapshots after t_r get weight 0.  gamma_r may be an array (one column each)."""
    snap_t = np.asarray(snap_t, dtype=np.float64).ravel()
    snap_gamma = np.asarray(snap_gamma, dtype=np.float64).ravel()
    if snap_t.size == 0 or snap_t.shape != snap_gamma.shape:
        raise ValueError("post-hoc EMA: no snapshots (or steps and gammas of different lengths)")
    if not (np.all(np.isfinite(snap_t)) and np.all(snap_t >= 1) and np.all(np.isfinite(snap_gamma))
            and np.all(snap_gamma >= 0)):
        raise ValueError("post-hoc EMA: snapshot steps must be >= 1 and gammas finite and >= 0")
    t_r = float(t_r)
    if not np.any(snap_t == t_r):
        raise ValueError(f"post-hoc EMA: the target step {t_r:g} is not the step of a snapshot (steps "
                         f"{sorted(set(snap_t.tolist()))[:4]}...{sorted(set(snap_t.tolist()))[-2:]}); a target after the "
                         "last snapshot cannot be reconstructed")
    scalar = np.ndim(gamma_r) == 0
    gamma_r = np.atleast_1d(np.asarray(gamma_r, dtype=np.float64))
    if not (np.all(np.isfinite(gamma_r)) and np.all(gamma_r >= 0)):
        raise ValueError("post-hoc EMA: target gamma must be finite and >= 0")
    use = snap_t <= t_r
    ti, gi = snap_t[use], snap_gamma[use]
    A = np.exp(log_profile_inner(ti[:, None], gi[:, None], ti[None, :], gi[None, :]))
    B = np.exp(log_profile_inner(ti[:, None], gi[:, None], t_r, gamma_r[None, :]))
    xs = np.linalg.lstsq(A, B, rcond=None)[0]
    x = np.zeros((snap_t.size, gamma_r.size))
    x[use] = xs
    if not np.all(np.isfinite(x)):
        raise ValueError("post-hoc EMA: the least-squares solve produced non-finite coefficients")
    return x[:, 0] if scalar else x


# ------------------------------------------------------------------ reconstruction from snapshot files (GPU)
def list_snapshots(snapshot_dir):
    """-> [(step, path, gammas)] of the snapshot files in snapshot_dir, sorted by step"""
    d = Path(snapshot_dir)
    if not d.is_dir():
        raise ValueError(f"post-hoc EMA: no snapshot directory {d}")
    out = []
    for f in sorted(d.iterdir()):
        if _FILE.match(f.name):
            meta = torch.load(f, map_location="cpu", weights_only=True, mmap=True)
            out.append((int(meta["step"]), f, [float(g) for g in meta["gammas"]]))
    if not out:
        raise ValueError(f"post-hoc EMA: no snapshot files (phema-*.pt) in {d}")
    return sorted(out, key=lambda e: e[0])


def plan(snapshot_dir, sigma_rels, step=None):
    """-> (snapshots [(step, path, gammas)], t_r, coefficients [S, K, L]) of a reconstruction"""
    sigma_rels = [check_sigma_rel(s) for s in sigma_rels]
    if not 1 <= len(sigma_rels) <= MAX_LENGTHS:
        raise ValueError(f"post-hoc EMA: 1 to {MAX_LENGTHS} lengths per reconstruction, got {len(sigma_rels)}")
    snaps = list_snapshots(snapshot_dir)
    K = len(snaps[0][2])
    if any(len(g) != K for _, _, g in snaps):
        raise ValueError("post-hoc EMA: the snapshots track different numbers of profiles")
    t_r = snaps[-1][0] if step is None else int(step)
    snap_t = np.repeat([s for s, _, _ in snaps], K)
    snap_g = np.array([g for _, _, gs in snaps for g in gs])
    gam = np.array([sigma_rel_to_gamma(s) for s in sigma_rels], dtype=np.float64)
    coef = solve_coefficients(snap_t, snap_g, t_r, gam).reshape(len(snaps), K, len(sigma_rels))
    return snaps, t_r, coef


@torch.no_grad()
def reconstruct(snapshot_dir, sigma_rels, step=None, device="cuda", return_plan=False):
    """-> per length in `sigma_rels`, a tuple of per-parameter fp32 tensors on `device` (EMAOptimizer.ema_params order):
    the EMA of that length at step `step` (default: the last snapshot).  Each snapshot file is read once; every
    profile of it is accumulated into all lengths at once (edm_phema_accumulate, fp64 accumulator)."""
    from . import ops
    snaps, t_r, coef = plan(snapshot_dir, sigma_rels, step)
    L = coef.shape[2]
    acc, shapes, host = None, None, None
    for i, (s, path, _) in enumerate(snaps):
        if s > t_r:
            continue
        sd = torch.load(path, map_location="cpu", weights_only=True, mmap=True)
        for k, prof in enumerate(sd["profiles"]):
            sh = [tuple(t.shape) for t in prof]
            if shapes is None:
                shapes = sh
                n = sum(math.prod(x) for x in sh)
                acc = torch.zeros(L, n, device=device, dtype=torch.float64)
                host = torch.empty(n, dtype=torch.float32).pin_memory()
                dev = torch.empty(n, device=device, dtype=torch.float32)
            elif sh != shapes:
                raise ValueError(f"post-hoc EMA: {path} holds parameters of other shapes than the first snapshot")
            torch.cat([t.reshape(-1) for t in prof], out=host)
            dev.copy_(host)           # (synchronous: `host` is rewritten for the next profile)
            ops.phema_accumulate(acc, dev, coef[i, k])
    out = ops.phema_finish(acc)
    res = []
    for l in range(L):
        parts, off = [], 0
        for sh in shapes:
            n = math.prod(sh)
            parts.append(out[l, off:off + n].view(sh))
            off += n
        res.append(tuple(parts))
    return (res, (snaps, t_r, coef)) if return_plan else res


# ------------------------------------------------------------------ CLI
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m tinyedm.posthoc_ema",
                                 description="Reconstruct the EMA of any length from post-hoc EMA snapshots")
    ap.add_argument("--ckpt_path", required=True, help="checkpoint of the run (weights, config; its EMA is replaced)")
    ap.add_argument("--snapshot_dir", required=True, help="directory of the run's phema-*.pt snapshot files")
    ap.add_argument("--ema_length", type=float, nargs="+", required=True, help="sigma_rel values to reconstruct")
    ap.add_argument("--step", type=int, default=None, help="target step: a snapshot's step (default: the last)")
    ap.add_argument("--out_dir", required=True, help="where the checkpoints and their metadata go")
    ap.add_argument("--device", default="cuda")
    return ap


def output_name(sigma_rel: float, t_r: int) -> str:
    return f"phema-{sigma_rel:.4f}-step{int(t_r):010d}"


def write_outputs(ckpt: dict, sigma_rels, recon: List[tuple], t_r: int, snap_steps, coef, out_dir) -> List[Path]:
    """One checkpoint per length: `ckpt` with optimizer_states[0]["ema"] replaced (or added) by its reconstruction, plus
    a JSON file of metadata (sigma_rel, t_r, snapshot steps, coefficients [S, K], their sum)."""
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    written = []
    for l, (s, ema) in enumerate(zip(sigma_rels, recon)):
        ck = copy.copy(ckpt)
        states = [dict(o) for o in ckpt.get("optimizer_states") or [{}]]
        states[0]["ema"] = tuple(t.detach().cpu().clone() for t in ema)
        ck["optimizer_states"] = states
        name = output_name(s, t_r)
        torch.save(ck, out_dir / f"{name}.ckpt")
        c = np.asarray(coef)[..., l]
        meta = {"sigma_rel": float(s), "gamma": float(sigma_rel_to_gamma(s)), "t_r": int(t_r),
                "snapshot_steps": [int(x) for x in snap_steps], "coefficients": c.tolist(),
                "coefficient_sum": float(c.sum())}
        (out_dir / f"{name}.json").write_text(json.dumps(meta, indent=1))
        written.append(out_dir / f"{name}.ckpt")
    return written


def main(argv=None):
    a = build_parser().parse_args(argv)
    ckpt = torch.load(a.ckpt_path, map_location="cpu", weights_only=False)
    recon, (snaps, t_r, coef) = reconstruct(a.snapshot_dir, a.ema_length, step=a.step, device=a.device,
                                            return_plan=True)
    for p in write_outputs(ckpt, a.ema_length, recon, t_r, [s for s, _, _ in snaps], coef, a.out_dir):
        print(f"[posthoc_ema] wrote {p}")


if __name__ == "__main__":
    main()
