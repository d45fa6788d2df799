"""Optimizer side of the step: fused Adam + power-function EMA over flat HBM arenas.

Replaces ``optim.Adam(fused=True)`` (reference edm.py:251-253) and the NeMo-derived
``EMAOptimizer`` / ``EMA`` callback (reference ema.py): parameters, gradients, Adam moments and the
EMA copy each live in ONE contiguous fp32 arena (35.6 M floats for the CIFAR net), parameters and
their ``.grad`` are views into them, and a step is a single HIP launch that reads theta,g,m,v,ema and
writes theta,m,v,ema once -- instead of the multi-tensor Adam launch plus two foreach passes on a
side stream.  The flat gradient arena is also what the data-parallel reducer all-reduces.
"""
from __future__ import annotations

import contextlib
from typing import Iterable, List, Optional

import numpy as np
import torch

from . import ops
from .utils import swap_tensors


def sigma_rel_to_gamma(sigma_rel):
    """reference ema.py:29-32."""
    t = sigma_rel ** -2
    return np.roots([1, 7, 16 - t, 12 - t]).real.max()


class MisconfigurationException(Exception):
    pass


def _align(n: int, a: int = 64) -> int:
    return (n + a - 1) // a * a


def sequential_offsets(params):
    """layout 1 (rounds 1-2): every parameter in list order, 64-element aligned"""
    offs, off = [], 0
    for p in params:
        offs.append(off)
        off += _align(p.numel())
    return offs, off


def _is_late(p) -> bool:
    """the parameter's gradient becomes final only when the backward pass ENDS: 0-dim parameters (block gains: one
    modulation finish per step; gain_out rides along) and the weights flagged by the network (`_edm_late`: the blocks'
    embed Linears and the Embedding module, whose weight gradients are ONE launch behind every block's backward)"""
    return p.dim() == 0 or bool(getattr(p, "_edm_late", False))


def layout_offsets(params, layout: int):
    """-> (offsets in the caller's parameter order, first offset of the late region, total elements) of arena layout 1 / 2 / 3"""
    if layout == 1:
        offs, total = sequential_offsets(params)
        return offs, total, total
    late = (lambda p: p.dim() == 0) if layout == 2 else _is_late
    offs, off = [0] * len(params), 0
    for i, p in enumerate(params):
        if not late(p):
            offs[i] = off
            off += _align(p.numel())
    lo = off
    for tensors_first in (True, False):          # late tensors, then the 0-dim parameters (layout 2: only the latter exist)
        for i, p in enumerate(params):
            if late(p) and (p.dim() > 0) == tensors_first:
                offs[i] = off
                off += _align(p.numel())
    return offs, lo, off


class FlatArena:
    """Re-homes a parameter list into one contiguous fp32 buffer (views keep names/shapes/strides).

    Layout 3 (round 5): the parameters whose gradients are final when their own layer's backward has run, in list order;
    then a TAIL with every parameter whose gradient becomes final only at the END of the backward pass -- the blocks' embed
    Linear weights and the Embedding module (their weight gradients are one launch behind all blocks), then the 0-dim
    parameters (block gains, gain_out).  `self.params` keeps the caller's order (index i is the i-th parameter of the
    optimizer, which is what torch-Adam checkpoints are keyed on), only the offsets differ.  Why: the data-parallel
    reducer launches a bucket's all-reduce when ALL its gradients are final.  In layout 2 (round 3: only the 0-dim parameters
    in the tail) every 32 MB bucket contained some block's embed weight, so NO bucket could start before the backward pass
    ended (tests/test_rccl_gpu.py, round 5: 0.00 of the bytes issued before the last weight-gradient launch); now the
    tail is the reducer's last bucket(s) and the body's buckets follow the weight-gradient launches."""
    LAYOUT = 3

    def __init__(self, params: List[torch.nn.Parameter]):
        self.params = [p for p in params if p.requires_grad]
        dev = self.params[0].device
        for p in self.params:
            if p.dtype != torch.float32:
                raise TypeError("FlatArena expects fp32 master parameters")
        self.offsets, self.scalar_lo, off = layout_offsets(self.params, self.LAYOUT)   # [scalar_lo, numel): the late region
        self.numel = off
        self.theta = torch.zeros(off, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(off, device=dev, dtype=torch.float32)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                view = self.theta[o:o + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view
                p.grad = self.grad[o:o + p.numel()].view_as(p)
                p._edm_direct = True          # weight-gradient kernels may accumulate into p.grad directly
                p._edm_hooks = []

    def rebind_grads(self):
        for p, o in zip(self.params, self.offsets):
            g = self.grad[o:o + p.numel()].view_as(p)
            if p.grad is None or p.grad.data_ptr() != g.data_ptr():
                p.grad = g

    def zero_grad(self):
        self.grad.zero_()
        self.rebind_grads()


class PowerProfiles:
    """The post-hoc EMA profiles of a FusedAdam (Karras et al. 2024, Sec. 3; tinyedm_amd/posthoc_ema.py): K fp32 arenas
    laid out like the parameter arena, each updated in the optimizer's pass with beta = (1 - 1/t)^(gamma_k + 1), t the
    1-based count of profile updates.  The K betas live in a device array that `upload(t)` rewrites from a ring of
    pinned host rows (fp64 on the host, rounded to fp32), so the eager and the captured step share one launch form."""

    SLOTS = 16

    def __init__(self, theta: torch.Tensor, gammas):
        self.gammas = tuple(float(g) for g in gammas)
        K = len(self.gammas)
        if not 1 <= K <= ops.PHEMA_MAX_PROFILES:
            raise ValueError(f"post-hoc EMA: 1 to {ops.PHEMA_MAX_PROFILES} profiles, got {K}")
        self.arenas = theta.detach().clone().unsqueeze(0).repeat(K, 1)       # (K, numel): row k is profile k
        self.count = 0
        self.betas = torch.zeros(K, device=theta.device, dtype=torch.float32)
        self._host = torch.zeros(self.SLOTS, K, dtype=torch.float32).pin_memory()
        self._events = [None] * self.SLOTS
        self._i = 0

    def beta_values(self, t: int):
        """host betas of the t-th update (fp64 -> fp32)"""
        return np.array([(1.0 - 1.0 / t) ** (g + 1.0) for g in self.gammas], dtype=np.float32)

    def upload(self, t: int):
        """write the betas of update t into the device array (stream-ordered before the next optimizer launch)"""
        k = self._i % self.SLOTS
        self._i += 1
        if self._events[k] is not None:
            self._events[k].synchronize()
        self._host[k].numpy()[:] = self.beta_values(t)
        self.betas.copy_(self._host[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._events[k] = ev


class GradGuardBuffers:
    """Device side of a FusedAdam's gradient guard: the chunk table over the arena's parameter tensors, the per-tensor
    fp64 sums of squares and the 64-byte record (ops.grad_guard), plus a second record / buffer for FusedAdam.grad_norm().
    Allocates and uploads, so it is built outside any stream capture (the rule of FusedAdam._complement_table), once per
    optimizer, and never freed before it: a captured step goes on reading these addresses."""

    def __init__(self, arena: FlatArena):
        dev = arena.theta.device
        self.table = ops.grad_guard_table(arena.offsets, [p.numel() for p in arena.params], arena.theta.numel(), dev)
        P = len(arena.params)
        self.sumsq = torch.zeros(P, dtype=torch.float64, device=dev)
        self.record = ops.guard_record(dev)
        self.probe_sumsq = torch.zeros(P, dtype=torch.float64, device=dev)
        self.probe_record = ops.guard_record(dev)


class GradGuard:
    """the limits of FusedAdam.set_guard and the buffers they act through"""

    def __init__(self, buf: GradGuardBuffers, max_norm, clip_value, skip_nonfinite: bool):
        self.buf = buf
        self.max_norm = None if max_norm is None else float(max_norm)
        self.clip_value = None if clip_value is None else float(clip_value)
        self.skip_nonfinite = bool(skip_nonfinite)

    def key(self):
        """what a captured launch freezes: a graph captured under other limits must not be replayed"""
        return (self.max_norm, self.clip_value, self.skip_nonfinite)

    def state(self) -> dict:
        r = ops.read_guard_record(self.buf.record)
        return {"max_norm": self.max_norm, "clip_value": self.clip_value, "skip_nonfinite": self.skip_nonfinite,
                "steps": r["steps"], "skipped": r["skipped"], "clipped": r["clipped"],
                "consecutive_skips": r["consecutive_skips"]}

    def load_counters(self, st: dict):
        rec = np.zeros(1, dtype=ops.GUARD_RECORD)
        rec["coef"] = 1.0
        rec["clip_value"] = np.inf
        for k in ("steps", "skipped", "clipped", "consecutive_skips"):
            rec[k] = int(st.get(k, 0))
        self.buf.record.copy_(torch.from_numpy(rec.view(np.int64).copy()))


class FusedAdam(torch.optim.Optimizer):
    """Adam (no weight decay / amsgrad) with torch.optim.Adam semantics, one launch over the arena."""

    def __init__(self, params: Iterable[torch.nn.Parameter], lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        params = list(params)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))
        self.arena = FlatArena(params)
        self.m = torch.zeros_like(self.arena.theta)
        self.v = torch.zeros_like(self.arena.theta)
        self.step_count = 0
        self.grad_scale = 1.0
        self._complement_tables = {}    # fused set -> (ranges, chunks, lo, hi): the rest of the arena (_complement_table)

    # fuse_zero_grad = True: `step()` clears the gradient arena in the pass that reads it (it is the last reader) and the
    # `zero_grad()` that follows is free -- instead of a separate 142 MB fill (Trainer.fit and bench.py switch it on;
    # off by default because torch optimizers leave .grad intact after step()).
    fuse_zero_grad = False
    _cleared = False
    # post-hoc EMA profiles (PowerProfiles), attached by posthoc_ema.PostHocEMA; None: the step is the plain adam_ema
    phema: Optional[PowerProfiles] = None

    def attach_profiles(self, gammas) -> PowerProfiles:
        """start tracking post-hoc EMA profiles with these gammas: every later step() / step_dyn() updates them"""
        self.phema = PowerProfiles(self.arena.theta, gammas)
        return self.phema

    # gradient guard (GradGuard), enabled by set_guard(); None: step() / step_dyn() run exactly the unguarded kernels
    guard: Optional["GradGuard"] = None

    def set_guard(self, max_norm: Optional[float] = None, clip_value: Optional[float] = None,
                  skip_nonfinite: bool = False, monitor: bool = False):
        """Guard every later step() / step_dyn(): one reduction over the gradient arena leaves the norm of the whole
        gradient, the clip coefficient and the skip decision in a device record, and the guarded optimizer kernel reads
        it -- no host synchronisation, so the sequence replays inside a hipGraph.

        max_norm: clip the gradient to this 2-norm (torch.nn.utils.clip_grad_norm_: coef = min(1, max_norm / (norm + 1e-6))).
        clip_value: limit every element of the scaled gradient to +-clip_value (clip_grad_value_).
        skip_nonfinite: a step whose gradient holds a NaN or an infinity changes nothing (weights, moments, EMA and
            post-hoc EMA profiles stay bit for bit; the gradient arena is cleared as usual).
        monitor: keep the reduction running with every limit off (what GradNormMonitor asks for).
        `set_guard()` with no argument removes the guard.

        The host does not know that a step was skipped: the Adam step count, the EMA step, the LR schedule and the Philox
        step advance on a skipped step as on any other, so the bias corrections after k skips are those of step t + k.
        While a guard is set a captured step takes the "unfused" path (graph.CapturedTrainStep.path)."""
        for name, x in (("max_norm", max_norm), ("clip_value", clip_value)):
            if x is not None and not float(x) >= 0.0:
                raise ValueError(f"FusedAdam.set_guard: {name} must be >= 0, got {x}")
        if max_norm is None and clip_value is None and not skip_nonfinite and not monitor:
            self.guard = None
            return None
        if self._guard_buffers is None:     # built once, kept for the life of the optimizer: captured graphs read them
            self._guard_buffers = GradGuardBuffers(self.arena)
        self.guard = GradGuard(self._guard_buffers, max_norm, clip_value, bool(skip_nonfinite))
        return self.guard

    _guard_buffers: Optional["GradGuardBuffers"] = None

    def _run_guard(self, grad_scale, dyn):
        gd = self.guard
        ops.grad_guard(self.arena.grad, gd.buf.table, gd.buf.sumsq, gd.buf.record, grad_scale=grad_scale, dyn=dyn,
                       max_norm=gd.max_norm, clip_value=gd.clip_value, skip_nonfinite=gd.skip_nonfinite)

    def _adam_guarded(self, ema, step, ema_beta, grad_scale, dyn, zero_grad):
        """the guard's reduction, then the guarded form of the optimizer kernel (with the profiles when they are tracked)"""
        g = self.param_groups[0]
        self._run_guard(grad_scale, dyn)
        args = (g["lr"], g["betas"][0], g["betas"][1], g["eps"], step, ema_beta, grad_scale)
        if self.phema is None:
            ops.adam_ema_guarded(self.arena.theta, self.arena.grad, self.m, self.v, ema, self.guard.buf.record, *args,
                                 dyn=dyn, zero_grad=zero_grad)
        else:
            ops.adam_ema_phema_guarded(self.arena.theta, self.arena.grad, self.m, self.v, ema,
                                       self.phema.arenas.unbind(0), self.phema.betas, self.guard.buf.record, *args,
                                       dyn=dyn, zero_grad=zero_grad)

    def guard_stats(self) -> dict:
        """what the guard's device record holds after the latest step (one D2H copy of 64 bytes, which waits for the stream)"""
        if self.guard is None:
            raise RuntimeError("FusedAdam.guard_stats: no guard is set (set_guard)")
        r = ops.read_guard_record(self.guard.buf.record)
        return {"grad_norm": r["norm"], "clip_coef": r["coef"], "skipped_steps": r["skipped"], "clipped_steps": r["clipped"],
                "consecutive_skips": r["consecutive_skips"], "steps": r["steps"], "skipped_last": bool(r["skip"])}

    def per_tensor_grad_norms(self) -> torch.Tensor:
        """2-norm of every parameter's scaled gradient as the latest guarded step saw it (device fp64 [P], arena order):
        the guard's per-tensor buffer, which stays valid after the step has cleared the arena"""
        if self.guard is None:
            raise RuntimeError("FusedAdam.per_tensor_grad_norms: no guard is set (set_guard)")
        return self.guard.buf.sumsq.sqrt()

    def grad_norm(self, per_tensor: bool = False) -> torch.Tensor:
        """The guard's reduction alone, for a loop of your own: the 2-norm of grad * grad_scale over the arena as it is now
        (fp64, on the device; nothing is read back), or the P per-parameter norms.  It neither needs nor disturbs a guard
        that is set: it has its own record and counts no step."""
        if self._guard_buffers is None:
            self._guard_buffers = GradGuardBuffers(self.arena)
        b = self._guard_buffers
        ops.grad_guard(self.arena.grad, b.table, b.probe_sumsq, b.probe_record, grad_scale=self.grad_scale, count=False)
        if per_tensor:
            return b.probe_sumsq.sqrt()
        return b.probe_record.view(torch.float64)[2].sqrt()       # (the record's fp64 `sumsq` field)

    def _adam_phema(self, ema, step, ema_beta, grad_scale, dyn, zero_grad):
        g = self.param_groups[0]
        ops.adam_ema_phema(self.arena.theta, self.arena.grad, self.m, self.v, ema, self.phema.arenas.unbind(0),
                           self.phema.betas, g["lr"], g["betas"][0], g["betas"][1], g["eps"], step, ema_beta,
                           grad_scale, dyn=dyn, zero_grad=zero_grad)

    def zero_grad(self, set_to_none: bool = False):
        # step() cleared the arena itself (fuse_zero_grad) and nothing has been written into it since: free.  "Since"
        # is tracked by the Denoiser forward (networks.note_backward_pending, via reset_backward_state), the one place
        # every gradient-producing pass goes through -- a step(); backward(); zero_grad() sequence clears for real.
        if self._cleared and not _grads_written_since_clear(self):
            self._cleared = False
            self.arena.rebind_grads()
            self._note_clear()
            return
        self._cleared = False
        self.arena.zero_grad()
        self._note_clear()

    # "The arena is all zero and no gradient-producing pass has started since": what lets graph.CapturedTrainStep apply the
    # update inside the weight-gradient finish kernels, which never read the arena rows they cover.  Every clearing call
    # notes the forward epoch; a Denoiser forward with autograd on (training or eval mode) moves it on.
    _clear_epoch = -1

    def _note_clear(self):
        from . import networks
        self._clear_epoch = networks.FORWARD_EPOCH

    def arena_known_clear(self) -> bool:
        from . import networks
        return self._clear_epoch == networks.FORWARD_EPOCH

    @torch.no_grad()
    def step(self, closure=None, ema: Optional[torch.Tensor] = None, ema_beta: float = 0.0):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        self.arena.rebind_grads()
        self.step_count += 1
        if self.guard is not None:
            if self.phema is not None:
                self.phema.upload(self.phema.count + 1)
            self._adam_guarded(ema, self.step_count, ema_beta, self.grad_scale, None, self.fuse_zero_grad)
            if self.phema is not None:
                self.phema.count += 1
        elif self.phema is None:
            ops.adam_ema(self.arena.theta, self.arena.grad, self.m, self.v, ema, g["lr"], g["betas"][0], g["betas"][1],
                         g["eps"], self.step_count, ema_beta, self.grad_scale, zero_grad=self.fuse_zero_grad)
        else:
            self.phema.upload(self.phema.count + 1)
            self._adam_phema(ema, self.step_count, ema_beta, self.grad_scale, None, self.fuse_zero_grad)
            self.phema.count += 1
        self._cleared = bool(self.fuse_zero_grad)
        from . import networks
        self._fwd_epoch_at_clear = networks.FORWARD_EPOCH
        if self.fuse_zero_grad:
            self._note_clear()
        networks.bump_weight_epoch()
        return loss

    @torch.no_grad()
    def step_dyn(self, dyn: torch.Tensor, ema: Optional[torch.Tensor] = None, fused=None):
        """The same update with lr / bias corrections / ema_beta / grad_scale read from the device record `dyn`
        (edm_step_params) and the gradient arena cleared in the same pass: the form a captured step replays
        (graph.CapturedTrainStep owns the host-side counters).

        fused: the (offset, numel) arena slices that the weight-gradient finish kernels of this backward pass have
        already updated (networks.FusedOptPass.updated): the pass then runs over the rest of the arena only."""
        g = self.param_groups[0]
        self.arena.rebind_grads()
        if self.guard is not None:      # the norm of the WHOLE gradient comes first: no row may have been updated yet
            if fused:
                raise RuntimeError("FusedAdam.step_dyn: a guarded step needs the whole-arena pass (the weight-gradient "
                                   "finish must not have updated rows before the gradient norm exists)")
            self._adam_guarded(ema, max(1, self.step_count), 0.0, 1.0, dyn, True)
        elif self.phema is not None:    # (the profile betas: uploaded by the caller, PowerProfiles.upload)
            if fused:
                raise RuntimeError("FusedAdam.step_dyn: post-hoc EMA profiles are updated by the whole-arena pass only")
            self._adam_phema(ema, max(1, self.step_count), 0.0, 1.0, dyn, True)
        elif fused:
            # the rest of the arena: its longest contiguous stretch through the plain kernel (grid-stride quads, no table),
            # the scattered remainder through the table-driven one
            ranges, chunks, lo, hi = self._complement_table(fused)
            args = (g["lr"], g["betas"][0], g["betas"][1], g["eps"], max(1, self.step_count), 0.0, 1.0)
            if hi > lo:
                ops.adam_ema(self.arena.theta[lo:hi], self.arena.grad[lo:hi], self.m[lo:hi], self.v[lo:hi],
                             None if ema is None else ema[lo:hi], *args, dyn=dyn, zero_grad=True)
            ops.adam_ema_ranges(self.arena.theta, self.arena.grad, self.m, self.v, ema, ranges, chunks, *args, dyn=dyn,
                                zero_grad=True)
        else:
            ops.adam_ema(self.arena.theta, self.arena.grad, self.m, self.v, ema, g["lr"], g["betas"][0], g["betas"][1],
                         g["eps"], max(1, self.step_count), 0.0, 1.0, dyn=dyn, zero_grad=True)
        self._note_clear()

    def _complement_table(self, fused):
        """(ranges, chunks, lo, hi): the arena OUTSIDE the slices of `fused` as its longest stretch [lo, hi) (lo on a 16-byte
        boundary, for ops.adam_ema) and a device table of everything else (ops.adam_ema_ranges).  Built once per set and kept
        for the life of the optimizer: a captured graph goes on reading the table (a model has a handful of sets, ~50 KB
        each).  A new set allocates and uploads, which a stream capture cannot do (the launch-table rule of DESIGN 3.7: the
        table must not live in the capturing graph's pool) -- the warm-up steps of a captured step run the same set eagerly
        first."""
        key = tuple(sorted(fused))
        tab = self._complement_tables.get(key)
        if tab is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdam: the set of layers updated by the weight-gradient finish differs from every "
                                   "eager step before this capture; its range table cannot be built under stream capture")
            n = self.arena.theta.numel()
            lo = hi = 0
            for start, length in ops.complement_ranges(key, n):
                a = (start + 3) // 4 * 4
                if start + length - a > hi - lo:
                    lo, hi = a, start + length
            ranges, chunks = ops.adam_ranges_table(key + (((lo, hi - lo),) if hi > lo else ()), n, self.arena.theta.device)
            tab = self._complement_tables[key] = (ranges, chunks, lo, hi)
        return tab

    def state_dict(self):
        # "offsets": where each parameter's slice sits in m / v.  Layout 3 derives them from a Python attribute of the
        # parameters (`_edm_late`); a checkpoint that only said "layout 3" could not tell a model whose flags differ
        # (Parameter re-created, deepcopy, user re-init) from the one that wrote it
        return {"m": self.m, "v": self.v, "step": self.step_count, "layout": FlatArena.LAYOUT,
                "offsets": list(self.arena.offsets), "numels": [p.numel() for p in self.arena.params],
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups],
                **({} if self.phema is None else {"phema": {"profiles": self.phema.arenas, "count": self.phema.count,
                                                             "gammas": list(self.phema.gammas)}}),
                **({} if self.guard is None else {"guard": self.guard.state()})}

    def load_state_dict(self, sd):
        """Accepts this class's own layout ({m, v, step}: flat arenas) or torch.optim.Adam's
        ({state: {i: {step, exp_avg, exp_avg_sq}}, param_groups}: what the reference's checkpoints hold)."""
        if "m" in sd:
            a = self.arena
            if "offsets" in sd:     # round 6 checkpoints carry the slices themselves
                old = [int(o) for o in sd["offsets"]]
                if len(old) != len(a.params) or [int(n) for n in sd["numels"]] != [p.numel() for p in a.params]:
                    raise ValueError("optimizer state: the checkpoint's parameter list (count / sizes) does not match the model")
                total = sd["m"].numel()
                if any(o < 0 or o + p.numel() > total for p, o in zip(a.params, old)):
                    raise ValueError("optimizer state: a stored offset lies outside the stored arena")
            else:                   # older checkpoints: the slices follow from the layout number and the CURRENT flags
                old, _, total = layout_offsets(a.params, int(sd.get("layout", 1)))
                if sd["m"].numel() != total:
                    raise ValueError(f"optimizer state: flat arena of {sd['m'].numel()} elements, expected {total}")
            if old == list(a.offsets) and sd["m"].numel() == self.m.numel():
                self.m.copy_(sd["m"])
                self.v.copy_(sd["v"])
            else:       # another arena layout (an earlier round's, or different late flags): every slice to its new home
                for p, o_new, o_old in zip(a.params, a.offsets, old):
                    n = p.numel()
                    self.m[o_new:o_new + n].copy_(sd["m"][o_old:o_old + n])
                    self.v[o_new:o_new + n].copy_(sd["v"][o_old:o_old + n])
            self.step_count = int(sd["step"])
            if self.phema is not None:
                self._load_profiles(sd, old)
        elif "state" in sd:
            if self.phema is not None:
                self._load_profiles(sd, None)
            a = self.arena
            if len(sd["state"]) not in (0, len(a.params)):
                raise ValueError(f"optimizer state has {len(sd['state'])} entries, the model {len(a.params)} parameters")
            steps = []
            for i, (p, o) in enumerate(zip(a.params, a.offsets)):
                st = sd["state"].get(i)
                if st is None:
                    continue
                if tuple(st["exp_avg"].shape) != tuple(p.shape):
                    raise ValueError(f"optimizer state {i}: shape {tuple(st['exp_avg'].shape)} != parameter {tuple(p.shape)}")
                self.m[o:o + p.numel()].view_as(p).copy_(st["exp_avg"])
                self.v[o:o + p.numel()].view_as(p).copy_(st["exp_avg_sq"])
                steps.append(int(st["step"]))
            self.step_count = max(steps) if steps else 0
        else:
            raise KeyError("optimizer state dict has neither this build's {m, v, step} nor torch Adam's {state, param_groups}")
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update({k: v for k, v in s.items() if k != "params"})
        if self.guard is not None and "guard" in sd:       # the counters continue; the limits are those of this run
            self.guard.load_counters(sd["guard"])


    def _load_profiles(self, sd, old_offsets):
        """the post-hoc EMA profiles of `sd` (same slices as m / v) into the attached PowerProfiles"""
        ph = sd.get("phema")
        if ph is None:
            raise ValueError("optimizer state: post-hoc EMA tracking is on, but the checkpoint holds no profile state -- "
                             "the profiles cannot be recreated mid-run (resume without the PostHocEMA callback, or "
                             "start tracking from step 0)")
        if [float(g) for g in ph["gammas"]] != list(self.phema.gammas):
            raise ValueError(f"optimizer state: the checkpoint tracks post-hoc EMA gammas {list(ph['gammas'])}, the run "
                             f"{list(self.phema.gammas)}")
        src, dst, a = ph["profiles"], self.phema.arenas, self.arena
        if tuple(src.shape) != (dst.shape[0], sd["m"].numel()):
            raise ValueError(f"optimizer state: post-hoc EMA profiles of shape {tuple(src.shape)}, expected "
                             f"({dst.shape[0]}, {sd['m'].numel()})")
        if old_offsets == list(a.offsets) and src.shape == dst.shape:
            dst.copy_(src)
        else:
            for p, o_new, o_old in zip(a.params, a.offsets, old_offsets):
                n = p.numel()
                dst[:, o_new:o_new + n].copy_(src[:, o_old:o_old + n])
        self.phema.count = int(ph["count"])


def _grads_written_since_clear(opt: "FusedAdam") -> bool:
    """a training-mode network forward (the start of every gradient-producing pass) ran after the clearing step()"""
    from . import networks
    return networks.FORWARD_EPOCH != getattr(opt, "_fwd_epoch_at_clear", -1)


class EMAOptimizer:
    """Same surface as the reference's EMAOptimizer (ema.py:160-348): wraps an optimizer, keeps an EMA
    copy updated with beta_t = (1 - 1/(t+1))^(gamma+1) after every ``every_n_steps`` optimizer steps,
    in-place weight swapping, and a state dict {opt, ema, current_step, gamma, every_n_steps}.
    With ``FusedAdam`` the EMA update is fused into the optimizer kernel."""

    def __init__(self, optimizer: FusedAdam, device=None, gamma: float = 0.0, every_n_steps: int = 1,
                 current_step: int = 0):
        if not isinstance(optimizer, FusedAdam):
            raise TypeError("tinyedm_amd.EMAOptimizer wraps tinyedm_amd.FusedAdam")
        self.optimizer = optimizer
        self.gamma = gamma
        self.device = device
        self.current_step = current_step
        self.every_n_steps = every_n_steps
        self.ema_arena = optimizer.arena.theta.clone()

    @property
    def ema_params(self):
        a = self.optimizer.arena
        return tuple(self.ema_arena[o:o + p.numel()].view_as(p) for p, o in zip(a.params, a.offsets))

    @property
    def param_groups(self):
        return self.optimizer.param_groups

    def all_parameters(self):
        return (p for g in self.param_groups for p in g["params"])

    def _should_update_at_step(self) -> bool:
        return self.current_step % self.every_n_steps == 0

    def step(self, closure=None, **kwargs):
        if self._should_update_at_step():
            decay = (1 - 1 / (self.current_step + 1)) ** (self.gamma + 1)
            loss = self.optimizer.step(closure, ema=self.ema_arena, ema_beta=float(decay))
        else:
            loss = self.optimizer.step(closure)
        self.current_step += 1
        return loss

    def zero_grad(self, set_to_none: bool = False):
        self.optimizer.zero_grad()

    def switch_main_parameter_weights(self):
        swap_tensors(self.optimizer.arena.theta, self.ema_arena)
        from .networks import bump_weight_epoch
        bump_weight_epoch()

    @contextlib.contextmanager
    def swap_ema_weights(self, enabled: bool = True):
        if enabled:
            self.switch_main_parameter_weights()
        try:
            yield
        finally:
            if enabled:
                self.switch_main_parameter_weights()

    def __getattr__(self, name):
        return getattr(self.__dict__["optimizer"], name)

    def synchronize(self):
        pass

    def state_dict(self):
        return {"opt": self.optimizer.state_dict(), "ema": tuple(t.clone() for t in self.ema_params),
                "current_step": self.current_step, "gamma": self.gamma, "every_n_steps": self.every_n_steps}

    def load_state_dict(self, sd):
        self.optimizer.load_state_dict(sd["opt"])
        for dst, src in zip(self.ema_params, sd["ema"]):
            dst.copy_(src)
        self.current_step = sd["current_step"]
        self.gamma = sd["gamma"]
        self.every_n_steps = sd["every_n_steps"]


class EMA:
    """Callback with the reference's hooks (ema.py:35-123): wraps the trainer's optimizers at fit start,
    swaps EMA weights in for validation/test unless ``validate_original_weights``."""

    def __init__(self, ema_length: float, validate_original_weights: bool = False, every_n_steps: int = 1,
                 cpu_offload: bool = False):
        if not (0 <= ema_length <= 0.2886):
            raise MisconfigurationException("EMA length value must be between 0 and 0.2886")
        if cpu_offload:
            raise MisconfigurationException("cpu_offload is not supported: the EMA lives in HBM next to the weights")
        self.ema_length = ema_length
        self.gamma = sigma_rel_to_gamma(ema_length)
        self.validate_original_weights = validate_original_weights
        self.every_n_steps = every_n_steps
        self.cpu_offload = cpu_offload

    def on_fit_start(self, trainer, pl_module) -> None:
        trainer.optimizers = [
            o if isinstance(o, EMAOptimizer) else EMAOptimizer(o, device=pl_module.device, gamma=self.gamma,
                                                               every_n_steps=self.every_n_steps,
                                                               current_step=trainer.global_step)
            for o in trainer.optimizers]

    def _should_validate_ema_weights(self, trainer) -> bool:
        return not self.validate_original_weights and any(isinstance(o, EMAOptimizer) for o in trainer.optimizers)

    def swap_model_weights(self, trainer):
        for o in trainer.optimizers:
            assert isinstance(o, EMAOptimizer)
            o.switch_main_parameter_weights()

    def on_validation_start(self, trainer, pl_module) -> None:
        if self._should_validate_ema_weights(trainer):
            self.swap_model_weights(trainer)

    def on_validation_end(self, trainer, pl_module) -> None:
        if self._should_validate_ema_weights(trainer):
            self.swap_model_weights(trainer)

    on_test_start = on_validation_start
    on_test_end = on_validation_end
