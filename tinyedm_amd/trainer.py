"""Minimal stand-ins for the parts of lightning the reference's hot path touches (lightning is not
installed): a LightningModule base (``log``, ``hparams``, ``lr_schedulers``, ``device``) and a Trainer
(``fit`` / ``predict``, callbacks, gradient accumulation, one process per GPU with the flat-arena
gradient reducer).  Everything that is control plane in Lightning (checkpoint managers, loggers,
progress bars) is out of scope; hooks used by the reference's EMA callback are honoured."""
from __future__ import annotations

import os
import time
from typing import Any, List, Optional

import torch
import torch.distributed as dist

from .ddp import GradReducer
from .ema import EMAOptimizer, FusedAdam, MisconfigurationException


class LightningModule(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.hparams: dict = {}
        self.trainer: Optional["Trainer"] = None
        self._logged: dict = {}

    @property
    def device(self):
        try:
            return next(self.parameters()).device
        except StopIteration:
            return torch.device("cpu")

    def log(self, name: str, value: Any, **kwargs) -> None:
        self._logged[name] = value

    def lr_schedulers(self):
        return self.trainer.lr_scheduler if self.trainer is not None else None

    def configure_callbacks(self):
        return []

    def backward(self, loss: torch.Tensor, *args, **kwargs) -> None:
        """Lightning's `LightningModule.backward(loss)` hook (what its automatic optimisation calls after `training_step`;
        default there: `loss.backward()`).  Here the root gradient is a cached scalar 1 that carries a mark: autograd's own
        `ones_like(loss)` is a fill launch per step, and the loss function's backward (metric.py) multiplies its saved
        gradient by the incoming one -- another launch -- unless it sees the mark.  Same gradients, two launches fewer."""
        if loss.dim() == 0 and not args and not kwargs:
            loss.backward(gradient=unit_gradient(loss))
        else:
            loss.backward(*args, **kwargs)


_UNIT = {}


def unit_gradient(loss: torch.Tensor) -> torch.Tensor:
    """the cached 0-dim 1.0 of `loss`'s device / dtype, marked `_edm_unit` (see LightningModule.backward)"""
    key = (loss.device, loss.dtype)
    one = _UNIT.get(key)
    if one is None:
        if loss.is_cuda and torch.cuda.is_current_stream_capturing():
            return torch.ones_like(loss)        # (never cache a tensor whose fill belongs to a graph being captured)
        one = _UNIT[key] = torch.ones((), device=loss.device, dtype=loss.dtype)
        one._edm_unit = True
    return one


class _ConstLR:
    def __init__(self, lr):
        self._lr = lr

    def get_last_lr(self):
        return [self._lr]

    def step(self):
        pass


class Trainer:
    """``Trainer(max_epochs=, max_steps=, accumulate_grad_batches=, check_val_every_n_epoch=, callbacks=,
    devices=, accelerator=, strategy=, precision=, logger=)`` -- the kwargs of conf/*.yaml ``trainer:``.
    ``precision`` is accepted for config compatibility: the HIP path always runs the bf16-mixed policy.

    ``gradient_clip_val`` / ``gradient_clip_algorithm`` ("norm": the 2-norm of the whole gradient, "value": every
    element) are Lightning's; ``skip_nonfinite_steps`` makes a step whose gradient holds a NaN or an infinity change
    nothing.  All three act on the device through FusedAdam.set_guard, in the eager loop and in the hipGraph replay
    alike.  The host does not know that a step was skipped: global_step, the Adam step count, the EMA step, the LR
    schedule and the Philox step advance as on any other step, so later bias corrections are those of t + skips.
    ``max_consecutive_skips`` skipped steps in a row end the run with GraphCorruptionError at the next health check."""

    def __init__(self, max_epochs: int = 1, max_steps: int = -1, accumulate_grad_batches: int = 1,
                 check_val_every_n_epoch: int = 1, callbacks: Optional[List[Any]] = None, devices: Any = 1,
                 accelerator: str = "gpu", strategy: str = "auto", precision: Any = "bf16-mixed", logger: Any = None,
                 log_every_n_steps: int = 50, gradient_clip_val: Optional[float] = None,
                 gradient_clip_algorithm: Optional[str] = "norm", skip_nonfinite_steps: bool = False,
                 max_consecutive_skips: int = 10, **_ignored):
        if gradient_clip_val is not None and not float(gradient_clip_val) >= 0.0:
            raise ValueError(f"Trainer: gradient_clip_val must be >= 0, got {gradient_clip_val}")
        gradient_clip_algorithm = "norm" if gradient_clip_algorithm is None else str(gradient_clip_algorithm).lower()
        if gradient_clip_algorithm not in ("norm", "value"):
            raise ValueError(f"Trainer: gradient_clip_algorithm must be 'norm' or 'value', got {gradient_clip_algorithm!r}")
        if int(max_consecutive_skips) < 1:
            raise ValueError(f"Trainer: max_consecutive_skips must be >= 1, got {max_consecutive_skips}")
        # (Lightning: a gradient_clip_val of 0 means "no clipping")
        self.gradient_clip_val = float(gradient_clip_val) if gradient_clip_val else None
        self.gradient_clip_algorithm = gradient_clip_algorithm
        self.skip_nonfinite_steps = bool(skip_nonfinite_steps)
        self.max_consecutive_skips = int(max_consecutive_skips)
        self.max_epochs, self.max_steps = max_epochs, max_steps
        self.accumulate_grad_batches = accumulate_grad_batches
        self.check_val_every_n_epoch = check_val_every_n_epoch
        self.callbacks = list(callbacks or [])
        self.precision = precision
        self.logger = logger
        self.log_every_n_steps = log_every_n_steps
        self.optimizers: List[Any] = []
        self.lr_scheduler = None
        self.scheduler_interval = "epoch"
        self.global_step = 0
        self.current_epoch = 0
        self.world_size = int(os.environ.get("WORLD_SIZE", "1"))
        self.global_rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.reducer: Optional[GradReducer] = None
        self.datamodule = None
        self.callback_metrics: dict = {}
        self._resume_skip = 0          # batches of the first epoch already consumed before the checkpoint was written
        # The step is replayed from a hipGraph (graph.CapturedTrainStep) whenever that is possible: no gradient accumulation,
        # the flat-arena optimizer, and the safe runtime setting in place (_runtime_env).  Round 5: this is the DEFAULT on one
        # GPU -- the replay is 3 % faster than the eager loop since the step dropped below the host's ~10 ms of enqueue
        # (13.16 vs 13.56 ms, BENCH_r04), and it is what bench.py times.  EDM_GRAPH=0 opts out; with more than one rank the
        # captured step (RCCL nodes inside the graph) has only ever run with a forced single rank, so it stays opt-in there
        # (EDM_GRAPH=1) until a multi-GPU node has seen it.
        env = os.environ.get("EDM_GRAPH")
        self.use_graph = (self.world_size == 1) if env is None else env != "0"
        # No explicit choice (EDM_GRAPH unset): fit() PROBES -- PROBE_STEPS steps through each form once the graph exists, and
        # the faster one trains on.  The replay wins where the host's enqueue is the longer pole (CIFAR-10: 13.1 vs 13.6 ms);
        # the eager loop overlaps the weight-gradient kernels on a side stream, which wins on the large nets (ImageNet
        # latent config, 272 M parameters, round 4: 1 334 img/s eager vs 1 263 replayed).  Every probed step is an ordinary
        # optimisation step either way.
        self.graph_auto = env is None
        self.step_launch = None                 # "hipGraph replay" / "eager loop": what fit() settled on

    # ------------------------------------------------------------------ setup
    def _setup_distributed(self, model):
        if torch.cuda.is_available():
            torch.cuda.set_device(self.local_rank)
        if self.world_size > 1 and not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if torch.cuda.is_available():
                dist.init_process_group("nccl", device_id=torch.device("cuda", self.local_rank))
            else:
                dist.init_process_group("gloo")
        if torch.cuda.is_available():
            model.to(torch.device("cuda", self.local_rank))
        if self.world_size > 1:
            # every rank built the model from the same seed; the Philox streams (Diffuser noise, dropout) must differ
            # per rank or all ranks would noise their different shards with identical draws
            from . import networks
            if not getattr(self, "_rank_seeded", False):
                self._base_seed = networks.rng.seed
                networks.rng.seed = self._rank_seed(self._base_seed)
                self._rank_seeded = True

    def _rank_seed(self, base_seed: int) -> int:
        """Philox seed of this rank for a run whose (rank-independent) seed is `base_seed`"""
        if self.world_size <= 1:
            return base_seed
        return (base_seed + 0x9E3779B97F4A7C15 * self.global_rank) & 0xFFFFFFFFFFFFFFFF

    def _call(self, hook: str, *args):
        for cb in self.callbacks:
            fn = getattr(cb, hook, None)
            if fn is not None:
                fn(self, *args)

    def _configure(self, model):
        model.trainer = self
        self._model = model
        self.callbacks += [c for c in model.configure_callbacks()]
        cfg = model.configure_optimizers()
        if isinstance(cfg, dict):
            opt = cfg["optimizer"]
            sch = cfg.get("lr_scheduler")
            if isinstance(sch, dict):
                self.scheduler_interval = sch.get("interval", "epoch")
                sch = sch["scheduler"]
            self.lr_scheduler = sch
        else:
            opt = cfg
        self.optimizers = [opt]
        if self.lr_scheduler is None:
            self.lr_scheduler = _ConstLR(opt.param_groups[0]["lr"])
        base = opt.optimizer if isinstance(opt, EMAOptimizer) else opt
        if isinstance(base, FusedAdam):
            self.reducer = GradReducer(base.arena)
            self.reducer.broadcast_parameters()
            self.reducer.broadcast_buffers(model)

    # ------------------------------------------------------------------ fit
    def fit(self, model, datamodule=None, train_dataloaders=None, val_dataloaders=None, ckpt_path=None):
        self._setup_distributed(model)
        self._configure(model)
        self.datamodule = datamodule
        if datamodule is not None and hasattr(datamodule, "setup"):
            datamodule.setup("fit")
        self._call("on_fit_start", model)
        start_epoch = 0
        if ckpt_path is not None:                 # resume (reference: experiments/train.py:30-33)
            start_epoch = self.load_checkpoint(ckpt_path, model)
        self._call("on_train_start", model)
        train = train_dataloaders if train_dataloaders is not None else datamodule.train_dataloader()
        val = val_dataloaders
        if val is None and datamodule is not None and hasattr(datamodule, "val_dataloader"):
            val = datamodule.val_dataloader()
        opt = self.optimizers[0]
        base = opt.optimizer if isinstance(opt, EMAOptimizer) else opt
        model.train()
        self._set_guard(base)
        if isinstance(base, FusedAdam):
            base.fuse_zero_grad = True        # step() is always followed by zero_grad() here
        opt.zero_grad()
        captured = None
        if (self.use_graph and self.accumulate_grad_batches == 1 and isinstance(base, FusedAdam)
                and torch.cuda.is_available()
                and (self.reducer is None or not self.reducer.active or self.reducer.capturable())):
            from . import _runtime_env
            if _runtime_env.GRAPH_REPLAY_SAFE:
                from .graph import CapturedTrainStep
                # N > 1 ranks: the bucket all-reduces are captured into the graph (every rank replays the same sequence)
                captured = CapturedTrainStep(model, opt, reducer=self.reducer)
            else:       # same arithmetic through the eager loop (see _runtime_env: the GPU was initialised too early)
                import warnings
                warnings.warn(f"tinyedm_amd: {_runtime_env.VAR}=0 was not in place before the GPU was initialised; "
                              "training runs the eager step instead of the hipGraph replay")
        self.step_launch = "eager loop" if captured is None else "hipGraph replay"
        probe = _LaunchProbe() if (captured is not None and self.graph_auto) else None
        done = 0 < self.max_steps <= self.global_step
        t0, imgs = time.time(), 0
        for epoch in range(start_epoch, self.max_epochs):
            if done:
                break
            self.current_epoch = epoch
            ep_t0, ep_imgs = time.time(), imgs
            if hasattr(train, "epoch"):
                train.epoch = epoch               # resident loaders: the shuffle is a function of (seed, epoch)
            for bi, batch in enumerate(train):
                if self._resume_skip > 0:         # mid-epoch checkpoint: these batches were consumed before it
                    self._resume_skip -= 1
                    continue
                self._batch_in_epoch = bi + 1
                batch = _to_device(batch, model.device)
                last_micro = (bi + 1) % self.accumulate_grad_batches == 0
                imgs += batch[0].shape[0] * self.world_size
                use_captured = captured is not None
                if use_captured and probe is not None:
                    use_captured = probe.choose(captured, batch)
                    if probe.done:
                        if not probe.graph_wins:
                            captured.release()
                            captured = None
                        self.step_launch = "hipGraph replay" if captured is not None else "eager loop"
                        probe = None
                if use_captured:
                    loss = captured(batch)
                else:
                    if self.reducer is not None:
                        self.reducer.enabled = last_micro
                    loss = model.training_step(batch, bi)
                    if self.accumulate_grad_batches == 1:
                        model.backward(loss)
                    else:
                        (loss / self.accumulate_grad_batches).backward()
                    if last_micro:
                        base.grad_scale = self.reducer.finish() if self.reducer is not None else 1.0
                        opt.step()
                        opt.zero_grad()
                if last_micro:
                    self.global_step += 1
                    if self.scheduler_interval == "step":
                        self.lr_scheduler.step()
                    guard_line = ""
                    if self.global_step % self.log_every_n_steps == 0:
                        stats = self._guard_stats(base)
                        self._check_health(model, loss, stats)
                        if stats is not None:
                            self.callback_metrics.update(grad_norm=stats["grad_norm"], grad_clip_coef=stats["clip_coef"],
                                                         skipped_steps=stats["skipped_steps"])
                            guard_line = (f" grad_norm {stats['grad_norm']:.4g} clip_coef {stats['clip_coef']:.4g} "
                                          f"skipped {stats['skipped_steps']}")
                    if self.global_rank == 0 and self.global_step % self.log_every_n_steps == 0:
                        print(f"[fit] epoch {epoch} step {self.global_step} loss {float(loss.detach()):.4f} "
                              f"{imgs / (time.time() - t0):.1f} img/s{guard_line}", flush=True)
                    # Lightning's hook, here once per completed optimizer step (posthoc_ema.PostHocEMA writes its snapshots)
                    self._call("on_train_batch_end", model, loss, batch, bi)
                    if 0 < self.max_steps <= self.global_step:
                        done = True
                        break
            self._batch_in_epoch = 0
            if self.global_rank == 0 and os.environ.get("EDM_FIT_EPOCH_RATE") == "1" and torch.cuda.is_available():
                torch.cuda.synchronize()      # (diagnostic: the steady-state rate of the training loop, one epoch at a time)
                print(f"[fit] epoch {epoch} rate {(imgs - ep_imgs) / (time.time() - ep_t0):.1f} img/s "
                      f"({self.step_launch}{', probing' if probe is not None else ''})", flush=True)
            if self.scheduler_interval == "epoch":
                self.lr_scheduler.step()
            if hasattr(model, "train_mse") and int(model.train_mse.total) > 0:
                self.callback_metrics["train_loss"] = float(model.train_mse.compute())
                model.train_mse.reset()
            if torch.cuda.is_available() and "loss" in locals():
                self._check_health(model, loss)          # before callbacks that write checkpoints / sample images
            self._epoch_complete = True
            self._call("on_train_epoch_end", model)
            if val is not None and (epoch + 1) % self.check_val_every_n_epoch == 0:
                self.validate(model, val)
            self._epoch_complete = False
        if isinstance(base, FusedAdam):
            base.fuse_zero_grad = False       # back to torch semantics: step() leaves .grad for the caller to clear
        if self.reducer is not None:
            self.reducer.close()              # hooks off the parameters, networks.W3_TAIL back (the next fit() builds its own)
        self._call("on_fit_end", model)

    def _set_guard(self, base):
        """gradient_clip_val / skip_nonfinite_steps -> FusedAdam.set_guard; with neither, a guard that the user or a callback set stays as it is"""
        if self.gradient_clip_val is None and not self.skip_nonfinite_steps:
            return
        if not isinstance(base, FusedAdam):
            raise MisconfigurationException("Trainer: gradient_clip_val / skip_nonfinite_steps act inside the fused "
                                            f"optimizer kernel and need tinyedm_amd.FusedAdam, not {type(base).__name__}")
        by_norm = self.gradient_clip_algorithm == "norm"
        base.set_guard(max_norm=self.gradient_clip_val if by_norm else None,
                       clip_value=None if by_norm else self.gradient_clip_val, skip_nonfinite=self.skip_nonfinite_steps)

    @staticmethod
    def _guard_stats(base):
        """the guard's device record (one 64-byte read), or None without a guard"""
        if not isinstance(base, FusedAdam) or base.guard is None or not torch.cuda.is_available():
            return None
        return base.guard_stats()

    def _check_health(self, model, loss=None, guard_stats=None):
        """The sentinel of the (graph-replayed or eager) step: the optimizer kernel leaves a bit in the device health
        word when a non-finite gradient / weight went through it; read here, at the log interval and at epoch ends,
        it turns a diverged or corrupted run into an exception instead of a checkpoint full of NaN.

        With a guard that skips non-finite steps the guard's record is read at the same points: a non-finite loss of a
        step the guard skipped is not an error (nothing was updated), `max_consecutive_skips` skips in a row are."""
        if not torch.cuda.is_available():
            return
        from . import ops
        ops.check_health(model.device, f"Trainer.fit (epoch {self.current_epoch}, step {self.global_step})")
        opt = self.optimizers[0] if self.optimizers else None
        base = opt.optimizer if isinstance(opt, EMAOptimizer) else opt
        skipping = isinstance(base, FusedAdam) and base.guard is not None and base.guard.skip_nonfinite
        if skipping:
            st = guard_stats if guard_stats is not None else base.guard_stats()
            if st["consecutive_skips"] >= self.max_consecutive_skips:
                raise ops.GraphCorruptionError(
                    f"Trainer.fit: the last {st['consecutive_skips']} optimizer steps were skipped for non-finite gradients "
                    f"(max_consecutive_skips={self.max_consecutive_skips}) at step {self.global_step}; "
                    f"{st['skipped_steps']} skipped in all")
            if st["skipped_last"]:
                return
        if loss is not None and not bool(torch.isfinite(loss.detach()).all()):
            raise ops.GraphCorruptionError(f"Trainer.fit: loss is not finite at step {self.global_step}")

    @torch.no_grad()
    def validate(self, model, val):
        self._call("on_validation_start", model)
        model.eval()
        if hasattr(model, "val_mse"):
            model.val_mse.reset()
        for bi, batch in enumerate(val):
            model.validation_step(_to_device(batch, model.device), bi)
        out = model.val_mse.compute() if hasattr(model, "val_mse") else None
        if out is not None:
            self.callback_metrics["val_loss"] = float(out)
        self._call("on_validation_epoch_end", model)
        model.train()
        self._call("on_validation_end", model)
        return out

    # ------------------------------------------------------------------ checkpoints
    def save_checkpoint(self, path, model=None):
        """Writes the Lightning checkpoint keys the reference's `EDM.load_from_checkpoint` reads (edm.py:159-203):
        `state_dict`, `hyper_parameters` (deinstantiated config, utils.py:5-27) and `optimizer_states[0]["ema"]`."""
        from . import networks
        model = model if model is not None else self._model
        ckpt = {"state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
                "hyper_parameters": dict(model.hparams), "epoch": self.current_epoch, "global_step": self.global_step,
                "optimizer_states": [_cpu_tree(o.state_dict()) for o in self.optimizers],
                "lr_schedulers": [self.lr_scheduler.state_dict()] if hasattr(self.lr_scheduler, "state_dict") else [],
                # what Lightning keeps in its loop state / torch RNG state: where in the epoch the run was, and the
                # counter-based RNG position (the Philox streams are a pure function of (seed, step))
                # rng_seed is the run's BASE seed (without the per-rank offset of _setup_distributed): every rank re-applies
                # its own offset when it resumes, so the ranks keep drawing different noise for their different shards
                "tinyedm_amd": {"rng_seed": getattr(self, "_base_seed", networks.rng.seed), "rng_step": networks.rng.step,
                                "epoch_complete": bool(getattr(self, "_epoch_complete", False)),
                                "batch_in_epoch": int(getattr(self, "_batch_in_epoch", 0))}}
        if self.global_rank == 0:
            torch.save(ckpt, path)
        return ckpt

    def load_checkpoint(self, path, model) -> int:
        """Resume from a checkpoint written by `save_checkpoint` (or by the reference: Lightning key layout): weights,
        optimizer (Adam moments in this build's flat layout or torch.optim.Adam's per-parameter layout, EMA), LR
        scheduler, counters and RNG position.  Must run after the optimizers exist (fit() calls it after
        on_fit_start).  Returns the epoch to continue with."""
        from . import networks
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        model.load_state_dict(ckpt["state_dict"], strict=False)
        networks.bump_weight_epoch()
        for o, sd in zip(self.optimizers, ckpt.get("optimizer_states", [])):
            o.load_state_dict(sd)
        for sd in ckpt.get("lr_schedulers", [])[:1]:
            if hasattr(self.lr_scheduler, "load_state_dict"):
                self.lr_scheduler.load_state_dict(sd)
        self.current_epoch, self.global_step = ckpt.get("epoch", 0), ckpt.get("global_step", 0)
        priv = ckpt.get("tinyedm_amd", {})
        if "rng_step" in priv:
            self._base_seed = int(priv["rng_seed"])
            networks.rng.seed, networks.rng.step = self._rank_seed(self._base_seed), priv["rng_step"]
        # Lightning semantics: a checkpoint written at the end of epoch e continues with epoch e+1; one written
        # mid-epoch re-enters epoch e after the batches it had already consumed
        if priv.get("epoch_complete", True):
            self._resume_skip = 0
            return self.current_epoch + 1
        self._resume_skip = int(priv.get("batch_in_epoch", 0))
        return self.current_epoch

    # ------------------------------------------------------------------ predict
    @torch.no_grad()
    def predict(self, model, datamodule=None, dataloaders=None, return_predictions: Optional[bool] = None, ckpt_path=None,
                distributed: bool = True):
        """Lightning's signature as the reference calls it (generate.py:45-47: ``predict(model, datamodule=...,
        return_predictions=False, ckpt_path=None)``).  ``return_predictions=False`` keeps nothing (the writer callback
        consumes each batch) and returns None; ``ckpt_path`` loads the weights first.
        ``distributed=False``: replicas-only sampling (no process group; each rank runs its own loader)."""
        if ckpt_path is not None:
            ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=False)
            model.load_state_dict(ckpt["state_dict"], strict=False)
            from . import networks
            networks.bump_weight_epoch()
        if return_predictions is None:
            return_predictions = True
        if distributed:
            self._setup_distributed(model)
        elif torch.cuda.is_available():
            model.to(torch.device("cuda", torch.cuda.current_device()))
        model.trainer = self
        model.eval()
        self.datamodule = datamodule
        if dataloaders is None and hasattr(datamodule, "setup"):
            datamodule.setup("predict")
        loader = dataloaders if dataloaders is not None else datamodule.predict_dataloader()
        outs = []
        for bi, batch in enumerate(loader):
            batch = _to_device(batch, model.device)
            out = model.predict_step(batch, bi)
            for cb in self.callbacks:
                fn = getattr(cb, "write_on_batch_end", None)
                if fn is not None:
                    fn(self, model, out, None, batch, bi, 0)
            if return_predictions:
                outs.append(out)
        return outs if return_predictions else None


class _EventClock:
    """device time between two points of the current stream (HIP events): what a block of steps costs the GPU, host gaps
    included, without a host synchronisation per step"""

    def mark(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def elapsed(self, a, b) -> float:
        b.synchronize()
        return a.elapsed_time(b)


class _LaunchProbe:
    """Which form of the step is faster for THIS model / batch on THIS box: once the step has been captured (its first
    replay has happened), PROBE_STEPS full-size steps run through the eager loop and PROBE_STEPS through the replay; the
    verdict stands for the rest of fit().  Each block is preceded by untimed steps of its own form (the first
    pass through the Trainer's eager path starts the weight-gradient side stream and its allocator pool cold, and a 5 %
    margin -- the 272 M ImageNet net: 1 338 img/s eager, 1 269 replayed -- flips on one cold step), and is timed with HIP
    events on the stream the steps run on, so the host's batch fetch only counts where it leaves the device idle."""
    PROBE_STEPS = 8
    WARM_STEPS = {"eager": 2, "graph": 1}

    def __init__(self, clock=None):
        self.clock = _EventClock() if clock is None else clock
        self.phase, self.n, self.t0, self.shape = "wait", 0, None, None
        self.times = {}
        self.done, self.graph_wins = False, True

    def choose(self, captured, batch) -> bool:
        """-> run this step through the captured graph?  (call once per step, before the step)"""
        key = tuple(batch[0].shape)
        has_graph = any(k[0] == key for k in captured._graphs)
        if self.phase == "wait":                    # until the graph of the (first, full-size) batch shape exists
            if not has_graph:
                return True                         # (CapturedTrainStep runs its own eager warm-up steps)
            self.shape, self.phase, self.n = key, "eager", -self.WARM_STEPS["eager"]
        if key != self.shape:                       # a ragged batch in the middle of the probe: not timed
            return has_graph
        if self.n == self.PROBE_STEPS:
            self.times[self.phase] = self.clock.elapsed(self.t0, self.clock.mark())
            if self.phase == "eager":
                self.phase, self.n = "graph", -self.WARM_STEPS["graph"]
            else:
                self.done = True
                self.graph_wins = self.times["graph"] <= self.times["eager"]
                return self.graph_wins
        if self.n == 0:
            self.t0 = self.clock.mark()
        self.n += 1
        return self.phase == "graph"


def _cpu_tree(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _cpu_tree(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_cpu_tree(v) for v in x)
    return x


def _to_device(batch, device):
    if isinstance(batch, (list, tuple)):
        return type(batch)(_to_device(b, device) for b in batch)
    if isinstance(batch, torch.Tensor):
        return batch.to(device, non_blocking=True)
    return batch
