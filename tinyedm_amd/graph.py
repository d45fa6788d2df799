"""The whole training step as ONE hipGraph.

An eager step enqueues ~400 kernels from Python (autograd.Function bodies + ctypes): ~10-14 ms of host time per
step, i.e. the host, not the GPU, sets the step time once the kernels are fast.  Capturing
`training_step -> backward -> (gradient all-reduce) -> fused Adam+EMA` into a hipGraph and replaying it removes that
cost: a step is one input copy, one 48-byte parameter upload and one graph launch.  The step is captured as one chain (the
weight-gradient side stream of the eager step is switched off while capturing).

What changes between replays cannot be a by-value kernel argument (those are frozen at capture time), so the
per-step scalars -- Philox step/seed of dropout and the Diffuser, learning rate, EMA beta, Adam bias corrections,
1/world -- live in a device `edm_step_params` record (include/tinyedm_hip.h) that `StepParams.upload` rewrites from a
pinned host ring before every replay; the kernels read it through their `dyn` argument.

Reference call sites this replaces: the Lightning automatic-optimisation loop around `EDM.training_step`
(edm.py:205-236), `optim.Adam(fused=True).step` (edm.py:251) and `EMAOptimizer.step` (ema.py:229-291).
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _runtime_env, networks, ops
from .ema import EMAOptimizer, FusedAdam


def _backward(model, loss):
    """the module's Lightning-style backward hook (trainer.LightningModule.backward: a cached, marked unit gradient instead of
    autograd's per-step ones_like) when it has one"""
    hook = getattr(model, "backward", None)
    if callable(hook):
        hook(loss)
    else:
        loss.backward()


class StepParams:
    """Device `edm_step_params` record + a ring of pinned host copies (so the host never rewrites a slot whose
    asynchronous upload has not executed yet)."""

    WORDS = 12      # 48 bytes

    def __init__(self, device, slots: int = 16):
        self.dev = torch.zeros(self.WORDS, dtype=torch.int32, device=device)
        self.host = torch.zeros(slots, self.WORDS, dtype=torch.int32).pin_memory()
        self._u = self.host.numpy().view(np.uint32)
        self._f = self.host.numpy().view(np.float32)
        self._events = [None] * slots
        self._i = 0

    def upload(self, *, step: int, seed: int, lr: float, ema_beta: float, grad_scale: float, bc1: float, bc2sqrt: float):
        k = self._i % len(self._events)
        self._i += 1
        if self._events[k] is not None:
            self._events[k].synchronize()
        u, f = self._u[k], self._f[k]
        u[0] = step & 0xFFFFFFFF
        u[1] = seed & 0xFFFFFFFF
        u[2] = (seed >> 32) & 0xFFFFFFFF
        f[4], f[5], f[6], f[7], f[8] = lr, ema_beta, grad_scale, bc1, bc2sqrt
        self.dev.copy_(self.host[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._events[k] = ev


class _CapturedStep(NamedTuple):
    graph: torch.cuda.CUDAGraph
    x: torch.Tensor         # static copy of the batch's images
    y: object               # ... and of its labels, or None
    loss: torch.Tensor      # static: rewritten by every replay
    token: object           # launch-table slots and plan pins of the capture (ops.release_capture)
    aug: object = None      # static copy of the batch's augment labels (a 3-element batch), or None
    path: str = "unfused"   # the form of the optimizer update the graph holds (CapturedTrainStep.path) ...
    fused_slices: tuple = ()   # ... and the arena slices its weight-gradient finish kernels update


class CapturedTrainStep:
    """`loss = step(batch)`: one optimisation step of `model` (an EDM) under `optimizer` (FusedAdam, optionally inside
    an EMAOptimizer), replayed from a hipGraph captured on the first call with a given batch shape.

    `reducer` (GradReducer, optional): the data-parallel step.  Its bucket all-reduces (RCCL) are issued by the same
    autograd hooks as in the eager step, on the comm stream forked from the capture stream, and joined before the
    optimizer kernel -- so they become nodes of the graph and an N-rank step costs the host one graph launch too (the
    eager step needs ~360 ctypes calls + the hook / collective launches per step from Python).  Every rank captures the
    same sequence of collectives, in the same order.  Semantics equal the eager sequence
        loss = model.training_step(batch, i); model.backward(loss); grad_scale = reducer.finish(); optimizer.step();
        optimizer.zero_grad()
    including the host-side counters (Philox step, Adam step, EMA step, weight epoch)."""

    WARMUP = 2
    MAX_GRAPHS = 4      # captured batch shapes kept (least recently used beyond that are released)

    def __init__(self, model, optimizer, grad_scale: float = 1.0, reducer=None, wgrad_fork=None):
        # wgrad_fork: keep the weight-gradient side stream (networks.WGRAD_STREAM) as a BRANCH of the captured graph.  None:
        # EDM_GRAPH_FORK (default off: the CIFAR-10 step replays 2.6 % slower with the branch; the 272 M ImageNet net is the
        # other way round -- round 6 measurements in DESIGN 6).
        self.wgrad_fork = (os.environ.get("EDM_GRAPH_FORK", "0") == "1") if wgrad_fork is None else bool(wgrad_fork)
        self.model = model
        self.opt = optimizer
        self.base = optimizer.optimizer if isinstance(optimizer, EMAOptimizer) else optimizer
        if not isinstance(self.base, FusedAdam):
            raise TypeError("CapturedTrainStep needs the flat-arena FusedAdam")
        _runtime_env.require_graph_replay_safe("CapturedTrainStep")
        self.ema = optimizer if isinstance(optimizer, EMAOptimizer) else None
        self.reducer = reducer if (reducer is not None and reducer.active) else None
        if self.reducer is not None:
            if not self.reducer.capturable():
                raise ValueError("CapturedTrainStep: the captured data-parallel step needs the RCCL ('nccl') backend and "
                                 "the in-place fp32 transport")
            grad_scale = grad_scale / self.reducer.world
        self.grad_scale = grad_scale
        self.params = StepParams(self.base.arena.theta.device)
        # warm-up steps and the capture run on ONE dedicated stream: autograd's AccumulateGrad nodes remember the
        # stream they were created on, and a node left over from a default-stream step would pull the default
        # stream into the capture (unjoined at capture end)
        self.stream = torch.cuda.Stream(self.base.arena.theta.device)
        self._graphs = {}
        self._seen = {}
        self._calls = 0
        # True once a capture failed on ANY rank of a multi-rank job: every rank then runs the eager step from here on
        # (ranks replaying captured collectives beside a rank that issues none would hang)
        self.fallback = False
        # The 3x3 weight-gradient finish applies Adam + EMA to the rows it holds and the optimizer kernel runs over the
        # rest of the arena.  EDM_FUSED_OPT=0: the whole-arena optimizer pass (A/B runs, bisecting).
        self.fused_opt = os.environ.get("EDM_FUSED_OPT", "1") != "0"
        self._fused = False
        self.last_path = None           # "fused" / "unfused": which form the latest step took ...
        self.fused_slices = ()          # ... and the (arena offset, numel) of the weights its finish kernels updated

    def path(self) -> str:
        """the form the NEXT step takes.  "fused" needs this class to own the whole update with nothing between the finish
        and the optimizer (no gradient all-reduce), no second consumer of the new weights in the optimizer pass (post-hoc
        EMA profiles), no gradient guard (FusedAdam.set_guard: the finish kernels would update rows before the norm of the
        whole gradient exists), and a gradient arena known to be all zero: the fused rows never read it."""
        ok = (self.fused_opt and self.reducer is None and self.base.phema is None and self.base.guard is None
              and self.base.fuse_zero_grad
              and self.base.arena_known_clear() and not networks._DGRAD_ONLY[0])
        return "fused" if ok else "unfused"

    def _opt_pass(self):
        if not self._fused:
            return contextlib.nullcontext(None)
        return networks.fused_opt_pass(self.base, self.ema.ema_arena if self.ema is not None else None, self.params.dev)

    def _step_dyn(self, fo):
        self.base.step_dyn(self.params.dev, ema=self.ema.ema_arena if self.ema is not None else None,
                           fused=None if fo is None else fo.updated)
        self.last_path = "unfused" if fo is None else "fused"
        self.fused_slices = () if fo is None else tuple(sorted(fo.updated))

    # ---- host-side bookkeeping identical to the eager path
    def _upload(self):
        g = self.base.param_groups[0]
        t = self.base.step_count + 1
        b1, b2 = g["betas"]
        beta = 1.0          # ema = 1*ema + 0*theta: the step leaves the EMA untouched
        if self.ema is not None and self.ema._should_update_at_step():
            beta = (1 - 1 / (self.ema.current_step + 1)) ** (self.ema.gamma + 1)
        self.params.upload(step=networks.rng.step, seed=networks.rng.seed, lr=float(g["lr"]), ema_beta=float(beta),
                           grad_scale=float(self.grad_scale), bc1=1.0 - b1 ** t, bc2sqrt=math.sqrt(1.0 - b2 ** t))
        if self.base.phema is not None:     # post-hoc EMA profiles: their betas ride in a device array of their own
            self.base.phema.upload(self.base.phema.count + 1)

    def _advance(self):
        self.base.step_count += 1
        if self.ema is not None:
            self.ema.current_step += 1
        networks.rng.step += 1
        if self.base.phema is not None:
            self.base.phema.count += 1
        networks.bump_weight_epoch()

    def _snapshot(self):
        return (self.base.step_count, self.ema.current_step if self.ema is not None else 0, networks.rng.step,
                self.base.phema.count if self.base.phema is not None else 0)

    def _restore(self, snap):
        self.base.step_count, cs, networks.rng.step, pc = snap
        if self.ema is not None:
            self.ema.current_step = cs
        if self.base.phema is not None:
            self.base.phema.count = pc

    def _eager(self, batch):
        """one step through the ordinary Python path, driven by the same device parameter record"""
        snap = self._snapshot()
        cur = torch.cuda.current_stream()
        self.stream.wait_stream(cur)
        side, networks.WGRAD_STREAM = networks.WGRAD_STREAM, self.wgrad_fork   # the launch structure of the capture that follows
        try:
            with torch.cuda.stream(self.stream):
                with self._opt_pass() as fo:
                    loss = self.model.training_step(batch, 0)
                    _backward(self.model, loss)
                if self.reducer is not None:
                    self.reducer.finish()   # joins the comm stream; 1/world rides in the device record (grad_scale)
                self._step_dyn(fo)
                loss = loss.detach()        # drop the autograd graph (and with it the AccumulateGrad nodes) now
        except BaseException:
            if self.reducer is not None:
                self.reducer.reset()        # a half-consumed pass must not leak pending counts into the next step
            raise
        finally:
            networks.WGRAD_STREAM = side
        cur.wait_stream(self.stream)
        self._restore(snap)
        return loss

    def _capture_agreed(self, batch):
        """Capture, then -- with more than one rank -- agree on the outcome: a rank-local failure (out of memory, a runtime
        that refuses a node) must not leave the other ranks replaying collectives nobody answers.  Returns the graph entry,
        or None when the job falls back to the eager step (single rank: the exception propagates)."""
        ent, err = None, None
        try:
            ent = _CapturedStep(*self._capture(batch))
        except Exception as e:      # noqa: BLE001
            err = e
        multi = self.reducer is not None and self.reducer.world > 1
        if multi:
            import torch.distributed as dist
            flag = torch.tensor([0 if err is not None else 1], device=self.base.arena.theta.device, dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.reducer.group)
            if int(flag.item()) == 0:
                import warnings
                warnings.warn("tinyedm_amd: capturing the data-parallel step failed on at least one rank"
                              + (f" (here: {type(err).__name__}: {str(err)[:200]})" if err is not None else "")
                              + "; every rank runs the eager step")
                self.fallback = True
                return None
        elif err is not None:
            raise err
        return ent

    def __call__(self, batch):
        x, y, *rest = batch
        a = rest[0] if rest else None       # augment labels of a (x, y, aug) batch
        key = (tuple(x.shape), x.dtype, None if y is None else (tuple(y.shape), y.dtype))
        if a is not None:                   # (a 2-element batch keeps the key it always had)
            key += ((tuple(a.shape), a.dtype),)
        # the two forms are different launch sequences: a step that may not take the fused one (e.g. gradients of an
        # eval-mode backward wait in the arena) does not replay a graph that would ignore them
        self._fused = self.path() == "fused"    # (read by _eager / _capture: their signatures are what subclasses override)
        if self._fused:
            key += ("fused",)
        if self.base.guard is not None:     # (the guard's limits are by-value arguments of the launches a graph holds)
            key += (("guard",) + self.base.guard.key(),)
        self._upload()
        networks.rng.dyn = self.params.dev
        try:
            ent = ops.lru_get(self._graphs, key)
            seen = self._seen.get(key, 0)
            self._seen[key] = seen + 1
            # (a batch shape is captured on its SECOND visit: its first step runs eagerly so that the plans / scratch of that
            # shape are allocated outside the capture -- e.g. the ragged last batch of an epoch)
            if ent is None and not self.fallback and self._calls >= self.WARMUP and seen >= 1:
                ent = self._capture_agreed(batch)
                if ent is not None:
                    ops.lru_put(self._graphs, key, ent, self.MAX_GRAPHS)
            if ent is None:
                loss = self._eager(batch)          # allocator / plan / stream warm-up before capturing; the fallback
            else:
                loss = ent.loss
                ent.x.copy_(x, non_blocking=True)
                if ent.y is not None:
                    ent.y.copy_(y, non_blocking=True)
                if ent.aug is not None:
                    ent.aug.copy_(a, non_blocking=True)
                ent.graph.replay()
                self.last_path, self.fused_slices = ent.path, ent.fused_slices
                self.base._note_clear()     # (the replayed optimizer pass cleared the arena, as step_dyn notes for an eager one)
        finally:
            networks.rng.dyn = None
        self._calls += 1
        self._advance()
        return loss

    def _capture(self, batch):
        x, y, *rest = batch
        sx = x.clone()
        sy = None if y is None else y.clone()
        sa = rest[0].clone() if rest and rest[0] is not None else None
        snap = self._snapshot()
        torch.cuda.synchronize()
        mode = "global"
        if self.reducer is not None:
            # torch's process-group watchdog thread polls the events of earlier (eager) collectives with hipEventQuery;
            # under a GLOBAL-mode capture that call from another thread is an error that invalidates the capture.  The
            # device is idle now, so give the watchdog a moment to retire what it still holds, and capture in
            # thread-local mode (only this thread's calls are policed).
            import time
            time.sleep(0.5)
            mode = "thread_local"
        graph = torch.cuda.CUDAGraph()
        # the step is captured as ONE chain: a weight-gradient side branch replays slower than the chain (CIFAR-10:
        # 15.5 vs 15.1 ms) -- hipGraph schedules the branch less favourably than the host's enqueue order does
        side, networks.WGRAD_STREAM = networks.WGRAD_STREAM, self.wgrad_fork
        try:
            # (a failed capture leaves no graph: capturing() gives its launch-table slots back)
            with ops.capturing(graph, stream=self.stream, capture_error_mode=mode) as capture:
                with self._opt_pass() as fo:
                    loss = self.model.training_step((sx, sy) if sa is None else (sx, sy, sa), 0)
                    _backward(self.model, loss)     # the reducer's hooks fork the comm stream off the capture stream ...
                if self.reducer is not None:
                    self.reducer.finish()       # ... and this joins it: the all-reduces are nodes of the graph
                self._step_dyn(fo)
                loss = loss.detach()
        except BaseException:
            if self.reducer is not None:
                self.reducer.reset()        # pending counts / fired set of the aborted pass
            raise
        finally:
            networks.WGRAD_STREAM = side
            self._restore(snap)
        return graph, sx, sy, loss, capture.token, sa, self.last_path, self.fused_slices

    def _drop(self, key):
        ops.drop_capture(self._graphs, key)

    def release(self):
        """drop every captured graph (their launch-table slots go back to the pool): call when the step object is retired"""
        for key in list(self._graphs):
            self._drop(key)

    def __del__(self):
        try:
            if self._graphs:
                torch.cuda.synchronize()        # (a replay of a dying graph may still be running: see _drop)
            for ent in self._graphs.values():
                ops.release_capture(ent.token)
        except Exception:       # noqa: BLE001  (interpreter shutdown)
            pass
