"""ODE / SDE samplers with the loop optionally captured in a hipGraph: the 2nd-order Heun ones, deterministic as in the
reference (solvers.py:4-59) and stochastic as Algorithm 2 of Karras et al. 2022, and the DPM-Solver++ multistep one
(Lu et al. 2022) that spends one network evaluation per step; the adaptive Heun / Euler pair; and the table solve iterated
in parallel over a window of steps (ParaDiGMS, Shih et al. 2023)."""
import math
import weakref
from dataclasses import dataclass
from typing import NamedTuple

import torch

from . import _runtime_env, ops
from .networks import Denoiser

UNCONDITIONAL = "unconditional"     # guide= sentinel: the model's own label-free evaluation is the guide


def _is_unconditional(guide) -> bool:
    return isinstance(guide, str) and guide == UNCONDITIONAL


def _check_step(who: str, name: str, step, num_steps: int) -> None:
    if isinstance(step, bool) or not isinstance(step, int) or not 0 <= step < num_steps:
        raise ValueError(f"{who}: {name} must be an integer in [0, {num_steps - 1}], got {step!r}")


def _check_float(who: str, name: str, t) -> None:
    if not isinstance(t, torch.Tensor) or not t.dtype.is_floating_point:
        raise ValueError(f"{who}: {name} must be a floating-point tensor")


def _check_gpu(cls: str, name: str, t) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"tinyedm_amd.{cls}: {name} must be a GPU tensor (there is no CPU path)")


def _sigma_table(who: str, sigmas) -> torch.Tensor:
    """a caller's sigma table (a sequence, numpy array or 1-D tensor of the N non-zero levels) as the fp32 host tensor a
    solver stores; ValueError unless it has >= 2 finite, positive entries that still decrease strictly as fp32 values"""
    try:
        if isinstance(sigmas, torch.Tensor):
            t = sigmas.detach().cpu().to(torch.float64)
        else:       # (through numpy: torch would round a list of Python floats to fp32 before the checks see it)
            import numpy as np
            t = torch.from_numpy(np.array(sigmas, dtype=np.float64))
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{who}: sigmas must be a sequence, numpy array or 1-D tensor of numbers") from None
    if t.dim() != 1 or t.numel() < 2:
        raise ValueError(f"{who}: sigmas must be one-dimensional with at least 2 entries, got shape {tuple(t.shape)}")
    if not bool(torch.isfinite(t).all()) or not bool((t > 0).all()):
        raise ValueError(f"{who}: sigmas must be finite and > 0 (the closing 0 is appended), got {t.tolist()}")
    t = t.float()
    if not bool(torch.isfinite(t).all()) or not bool((t > 0).all()) or not bool((t[1:] < t[:-1]).all()):
        raise ValueError(f"{who}: sigmas must be strictly decreasing, finite and > 0 as float32 values, got {t.tolist()}")
    return t


class Trajectory(NamedTuple):
    """what DeterministicSolver.trace records of one Heun solve of N steps"""
    x: torch.Tensor         # fp32 [N + 1, B, *shape]: node i is the state at t_i, node N the result of the solve
    slope: torch.Tensor     # fp32 [N, B, *shape]: the Euler slope dx at (x_i, t_i) (of the mixed D, with a guide)
    sigmas: torch.Tensor    # fp32 [N + 1] on the host: the table, closing 0 included


def _denoisers(net):
    """(module, its eval_dtype) of every Denoiser of a network -- the modules that own an evaluation precision and
    eval-mode weight packs; nothing for a plain callable"""
    if isinstance(net, torch.nn.Module):
        for m in net.modules():
            if isinstance(m, Denoiser):
                yield m, m.eval_dtype


class _Captured(NamedTuple):
    """one captured solve: the graph, the static tensors it reads and writes, and what its destruction gives back"""
    graph: object           # torch.cuda.CUDAGraph
    x: torch.Tensor         # static copy of x0 (or of the image of invert / log_likelihood)
    labels: object          # static copy of the class labels, or None
    out: object             # what the captured loop returned (static: cloned after every replay)
    t_dev: torch.Tensor     # the sigma table on the device
    token: object           # launch-table slots and plan pins of the capture (ops.release_capture)
    w_dev: object           # the guidance weight the graph reads, or None for an unguided solve
    guide: object           # the guide network (kept alive: the key holds its id); None for none or 'unconditional'
    state: object           # the mode's device state: _ChurnState, _MultistepState, _NllState, _PicardState or None
    cond: object            # static _Conditioning, or None
    rest: object            # static _Restoration, or None


class _Mode(NamedTuple):
    """what a captured entry runs, built by the entry point that knows it (solve, invert, log_likelihood)"""
    key: tuple              # what the mode appends to the graph key
    state: object           # () -> the entry's own device state, written for this call; or None
    loop: object            # (entry) -> the result, run on the entry's static tensors
    rewrite: object         # (state) -> None: rewrite that state host to device before a replay


def _release_solves(per_model: dict):
    try:
        for ent in per_model.values():
            ops.release_capture(ent.token)
        per_model.clear()
    except Exception:       # noqa: BLE001  (interpreter shutdown)
        pass


NLL_DELTA = 1e-2        # default relative half-width of the likelihood estimator's central difference


class _NllState(NamedTuple):
    """what a likelihood solve owns beside its images (a captured entry owns its own)"""
    rec: torch.Tensor       # the device record of the probe stream (ops.churn_record), rewritten before every replay
    L: torch.Tensor         # fp64 [B]: the accumulated log-density, zeroed by the loop itself


def bits_per_dim(logp, dims: int, std, levels: int = 256) -> torch.Tensor:
    """Bits per dimension of images with ``levels`` grey levels from the log-density ``logp`` (nats) of the NORMALISED
    image x = (u / (levels - 1) - mean) / std, as DeterministicSolver.log_likelihood returns it:

        bpd = (-logp / dims + mean_c log((levels - 1) * std_c)) / ln 2

    the density carried back to pixel units u, where one grey level has width 1.  ``dims`` = C*H*W, ``std`` the
    normalisation's standard deviation (a number or one per channel; channels have equal size).  Host only, fp64."""
    if isinstance(dims, bool) or not isinstance(dims, int) or dims < 1:
        raise ValueError(f"bits_per_dim: dims must be a positive integer, got {dims!r}")
    if isinstance(levels, bool) or not isinstance(levels, int) or levels < 2:
        raise ValueError(f"bits_per_dim: levels must be an integer >= 2, got {levels!r}")
    std = torch.as_tensor(std, dtype=torch.float64).flatten().cpu()
    if std.numel() == 0 or not bool((std > 0).all()) or not bool(torch.isfinite(std).all()):
        raise ValueError(f"bits_per_dim: std must be positive and finite, got {std.tolist()}")
    logp = torch.as_tensor(logp).detach().to(device="cpu", dtype=torch.float64)
    return (-logp / dims + torch.log((levels - 1) * std).mean()) / math.log(2.0)


class _Conditioning(NamedTuple):
    """the image conditioning of one solve (a captured entry owns static copies)"""
    start: int              # the step the solve enters at: x_start = image + t_start * x0
    image: object           # fp32 [B, C, H, W] or None (= 0)
    mask: object            # uint8 [1 or B, H*W], non-zero = known pixel, or None
    rec: object             # the device record of the inpainting noise (ops.churn_record), or None without a mask


@dataclass(frozen=True)
class LinearDegradation:
    """The measurement operator of zero-shot restoration (``solve(..., degradation=, measurement=)``): y = A x with A
    the mean over every ``scale`` x ``scale`` pixel block (``scale`` in 1, 2, 4, 8: box down-sampling) and, with
    ``gray``, also over the channels (at most 8).  Its pseudo-inverse A+ replicates a value to its block: A A+ = I and
    A+ A is an orthogonal projector.  ``scale=1`` without ``gray`` is the identity and raises ValueError.  Images are
    [B, C, H, W] with H and W multiples of ``scale``; y is [B, 1 if gray else C, H/scale, W/scale]."""
    scale: int = 4
    gray: bool = False

    def __post_init__(self):
        ops.check_degradation(self.scale, self.gray)

    def measurement_shape(self, x_shape) -> tuple:
        """the shape of A x for x of shape ``x_shape``; ValueError where A is not defined.  Host only."""
        return ops.measurement_shape(tuple(x_shape), self.scale, self.gray)

    def measure(self, image) -> torch.Tensor:
        """y = A image (ops.degrade), fp32.  ``image``: a floating-point GPU tensor [B, C, H, W]."""
        _check_float("LinearDegradation.measure", "image", image)
        self.measurement_shape(image.shape)
        _check_gpu("LinearDegradation", "image", image)
        return ops.degrade(image.float().contiguous(), self.scale, self.gray)

    def pinv(self, y, channels: int) -> torch.Tensor:
        """A+ y, fp32 [B, channels, H*scale, W*scale]: every value replicated to its block (and to ``channels``
        channels with ``gray``; otherwise ``channels`` is y's own).  It is the projection of the zero image
        (ops.project_denoised), bit for bit the A+ of a solve."""
        if not isinstance(y, torch.Tensor) or not y.dtype.is_floating_point or y.dim() != 4:
            raise ValueError("LinearDegradation.pinv: y must be a floating-point [B, C', h, w] tensor")
        if isinstance(channels, bool) or not isinstance(channels, int) or channels < 1:
            raise ValueError(f"LinearDegradation.pinv: channels must be a positive integer, got {channels!r}")
        shape = (y.shape[0], channels, y.shape[2] * self.scale, y.shape[3] * self.scale)
        if tuple(y.shape) != self.measurement_shape(shape):
            raise ValueError(f"LinearDegradation.pinv: y of shape {tuple(y.shape)} is no measurement of a "
                             f"{channels}-channel image")
        _check_gpu("LinearDegradation", "y", y)
        return ops.project_denoised(torch.zeros(shape, device=y.device), y.float().contiguous(), self.scale, self.gray)

    def adjoint(self, r, channels: int) -> torch.Tensor:
        """A^T r, fp32 [B, channels, H*scale, W*scale]: r replicated to its blocks (and channels, with ``gray``) and divided
        by the block size n -- exactly the transpose of the averaging A (<A u, v> = <u, A^T v>); A+ = n A^T."""
        if not isinstance(r, torch.Tensor) or not r.dtype.is_floating_point or r.dim() != 4:
            raise ValueError("LinearDegradation.adjoint: r must be a floating-point [B, C', h, w] tensor")
        if isinstance(channels, bool) or not isinstance(channels, int) or channels < 1:
            raise ValueError(f"LinearDegradation.adjoint: channels must be a positive integer, got {channels!r}")
        shape = (r.shape[0], channels, r.shape[2] * self.scale, r.shape[3] * self.scale)
        if tuple(r.shape) != self.measurement_shape(shape):
            raise ValueError(f"LinearDegradation.adjoint: r of shape {tuple(r.shape)} is no measurement of a "
                             f"{channels}-channel image")
        _check_gpu("LinearDegradation", "r", r)
        return ops.degrade_adjoint(r.float().contiguous(), channels, self.scale, self.gray)


@dataclass(frozen=True)
class GaussianBlur:
    """A measurement operator of diffusion posterior sampling (``solve(..., operator=, measurement=, dps_scale=)``): a
    separable Gaussian blur of every channel with ``2 * radius + 1`` taps exp(-k^2 / (2 std^2)), normalised to sum 1
    (``radius`` 1..4), and ZERO padding, so y has the image's shape and -- the taps being symmetric -- the operator is its
    own adjoint.  One small kernel (ops.blur2d).  It has no cheap pseudo-inverse: DDNM (``degradation=``) does not take it."""
    std: float = 1.0
    radius: int = 2

    def __post_init__(self):
        ops.gaussian_taps(self.std, self.radius)

    @property
    def taps(self) -> tuple:
        """the normalised taps as fp32 values"""
        return ops.gaussian_taps(self.std, self.radius)

    def measurement_shape(self, x_shape) -> tuple:
        if len(x_shape) != 4 or any(int(v) < 1 for v in x_shape):
            raise ValueError(f"GaussianBlur: expected a non-empty [B, C, H, W] shape, got {tuple(x_shape)}")
        return tuple(int(v) for v in x_shape)

    def measure(self, image) -> torch.Tensor:
        """y = A image, fp32 [B, C, H, W]; ``image``: a floating-point GPU tensor [B, C, H, W]"""
        _check_float("GaussianBlur.measure", "image", image)
        self.measurement_shape(image.shape)
        _check_gpu("GaussianBlur", "image", image)
        return ops.blur2d(image.float().contiguous(), self.taps)

    def adjoint(self, r, channels: int | None = None) -> torch.Tensor:
        """A^T r = A r (zero padding, symmetric taps)"""
        if channels is not None and (not isinstance(r, torch.Tensor) or r.dim() != 4 or r.shape[1] != channels):
            raise ValueError(f"GaussianBlur.adjoint: r must be a [B, {channels}, H, W] tensor")
        return self.measure(r)


class _Dps(NamedTuple):
    """the posterior-sampling conditioning of one solve"""
    op: object              # LinearDegradation or GaussianBlur
    y: torch.Tensor         # fp32, the measurement shape of the state
    scale: float            # zeta >= 0


class _Restoration(NamedTuple):
    """the measurement conditioning of one solve (a captured entry owns a static copy of y)"""
    scale: int
    gray: bool
    y: torch.Tensor         # fp32, the measurement shape of the state

    def project(self, D, Dg=None, w_dev=None):
        """D^ = D + A+ (y - A D) of one network evaluation, the guidance mix included when Dg is given"""
        return ops.project_denoised(D, self.y, self.scale, self.gray, Dg, None if Dg is None else w_dev)


def _check_measurement(x0, op, measurement) -> None:
    """the measurement y of a solve against x0 and its operator, on the host (nothing is read from a device)"""
    _check_float("solve", "measurement", measurement)
    if x0.dim() != 4:
        raise ValueError(f"solve: a measurement needs x0 of shape [B, C, H, W], got {tuple(x0.shape)}")
    shape = op.measurement_shape(x0.shape)
    if tuple(measurement.shape) != shape:
        raise ValueError(f"solve: measurement must have shape {shape} for x0 {tuple(x0.shape)} under {op}, got "
                         f"{tuple(measurement.shape)}")
    if measurement.device != x0.device:
        raise ValueError(f"solve: measurement is on {measurement.device}, x0 on {x0.device}")


def _mask_u8(mask, shape):
    """a bool / uint8 / float mask of shape [B,1,H,W], [1,1,H,W] or [H,W] as uint8 [B or 1, H*W] (non-zero = known)"""
    B, _, H, W = shape
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"solve: mask must be a tensor, got {type(mask).__name__}")
    if not (mask.dtype in (torch.bool, torch.uint8) or mask.dtype.is_floating_point):
        raise ValueError(f"solve: mask must be bool, uint8 or floating point, got {mask.dtype}")
    if tuple(mask.shape) not in {(B, 1, H, W), (1, 1, H, W), (H, W)}:
        raise ValueError(f"solve: mask must have shape {(B, 1, H, W)}, {(1, 1, H, W)} or {(H, W)}, got "
                         f"{tuple(mask.shape)}")
    return (mask != 0).to(torch.uint8).reshape(-1, H * W).contiguous()


class DeterministicSolver:
    """Algorithm 1 of Karras et al. 2022 with sigma(t)=t, s(t)=1.  Same constructor as the reference.

    The sigma table is built with the reference's exact fp32 expression (bitwise-equal table,
    solvers.py:33-41) and uploaded to the device ONCE: the reference's per-step ``t0.to(device)``
    host->device copies (63 sync points for 32 steps) disappear, which is what makes the whole
    solve capturable as one hipGraph (``solve(..., graph=True)``).

    Guided sampling (keyword-only ``guide``, ``guidance``, ``guidance_interval``): an evaluation at sigma uses

        D(x; sigma, c) = D_guide(x; sigma, c) + guidance * (D_main(x; sigma, c) - D_guide(x; sigma, c))

    classifier-free guidance with an unconditional ``guide`` (an unconditional EDM drops the labels itself),
    autoguidance with a smaller / less-trained conditional one.  ``guide="unconditional"`` is classifier-free guidance
    from the model alone: D_guide is the model's own label-free evaluation ``model(x, sigma, None)`` (same weights, same
    evaluation packs), for a conditional EDM trained with ``Embedding(label_dropout=p)``.  With ``guidance_interval=(lo, hi)`` only the
    evaluations with lo < sigma <= hi (sigma = the fp32 table value) are guided; the others use D_main alone and do not
    evaluate the guide.  ``guidance == 1`` guides nothing: the guide is never evaluated and the solve is the unguided
    one.  ``guidance`` and ``guidance_interval`` are plain attributes, read at every solve; a captured solve reads the
    guidance weight from device memory, so changing it replays the same graph.

    Image-conditioned sampling (keyword-only arguments of ``solve``; the defaults are the plain solve, bit for bit):
    ``start_step=k`` enters the table at t_k with the state x_k = image + t_k * x0 (``image`` defaults to 0, x0 is unit
    noise) and runs the steps i >= k only: SDEdit / image-to-image.  ``mask`` (with ``image``) is inpainting by
    replacement (Song et al. 2021; RePaint without its resampling jumps): before the Euler evaluation of every step
    i >= k the pixels where the mask is non-zero are replaced by image + t_i * n with fresh n ~ N(0, I), and after the
    last step by the image itself, so the result equals ``image`` there bit for bit.  That is N - k + 1 blends
    (ops.inpaint_blend) and no extra network evaluation.  The mask is binary (non-zero = known pixel, kept); soft masks
    and RePaint's resampling are not implemented.  The noise comes from ``seed`` and ``solve_index`` as the churn of
    StochasticSolver does, under a Philox tag of its own; ``solve_index`` increments after every inpainting solve.
    Zero-shot restoration (keyword-only ``degradation`` and ``measurement`` of ``solve``, both or neither): sample an
    image whose measurement ``degradation``(x) is ``measurement`` (LinearDegradation: super-resolution, colourisation)
    by the range / null-space decomposition of DDNM (Wang et al. 2023): every network evaluation of the loop (guided
    or not) is replaced by its projection D^ = D + A+ (y - A D) (ops.project_denoised, one more fp32 pass) before the
    unguided update, so the last step returns an image with A x = y to rounding.  No extra network evaluation, no
    backward pass.  ``start_step`` / ``image`` combine with it (SDEdit entered from ``degradation.pinv(y, C)``); ``mask``
    with ``measurement`` raises ValueError, and so does any invalid combination, on the host before any launch.  Noisy
    measurements (DDNM+), time travel / resampling and blur kernels are not implemented; ``invert`` and
    ``log_likelihood`` do not take the arguments.
    Diffusion posterior sampling (keyword-only ``operator``, ``measurement``, ``dps_scale`` of ``solve``; Chung et al. 2023
    in EDM / Heun form; Heun solvers, eager, bf16 evaluation path): step i evaluates D = model(x_i, t_i) with its input
    gradient, forms r = y - A D and g = J^T A^T r (``tinyedm.input_vjp``'s dgrad-only backward), takes the ordinary Euler +
    Heun step to x' and returns x' + (dps_scale / ||r_b||) g per sample (x' where the residual is zero).  ``operator`` is a
    ``LinearDegradation`` or a ``GaussianBlur``; y may be noisy; ``dps_scale=0`` is the plain solve bit for bit.  With
    ``degradation=``, a guide, ``mask=``, ``graph=True`` or ``MultistepSolver`` it raises ValueError.
    ``invert`` runs the probability-flow ODE upwards, image -> latent; ``log_likelihood`` does the same and integrates
    the change of variables along the way (keyword-only ``delta``: the relative half-width of its central difference).
    A caller's table (keyword-only ``sigmas``: a sequence, numpy array or 1-D tensor of the N non-zero levels, e.g. a
    ``tinyedm.schedule.Schedule``'s) replaces the Karras expression: ``num_steps`` becomes its length, ``sigma_max`` and
    ``sigma_min`` its ends, ``rho`` None; fewer than 2 entries, a value that is not finite or not positive, or values
    that do not decrease strictly as float32 raise ValueError.  The table is constructor-only.  ``trace`` records the
    states and Euler slopes of a solve (the teacher of the schedule search)."""

    MAX_GRAPHS = 4      # captured solves kept per model (shape / precision combinations; least recently used dropped)

    def __init__(self, num_steps: int = 18, sigma_min: float = 0.002, sigma_max: float = 80.0, rho: float = 7.0,
                 dtype: str | None = None, *, guide=None, guidance: float = 1.0,
                 guidance_interval: tuple[float, float] | None = None, seed: int = 0, delta: float = NLL_DELTA,
                 sigmas=None):
        table = None if sigmas is None else _sigma_table(type(self).__name__, sigmas)
        if table is not None:       # a caller's table: its length and its ends replace the Karras parameters
            num_steps, sigma_max, sigma_min, rho = table.numel(), table[0].item(), table[-1].item(), None
        self.num_steps = num_steps
        self.delta = delta
        self.seed = seed
        self.solve_index = 0
        self.sigma_min = sigma_min
        self.sigma_max = sigma_max
        self.rho = rho
        if dtype not in (None, "float32"):
            raise ValueError("tinyedm_amd.DeterministicSolver integrates in float32 (the reference's only working "
                             "setting: its .to(dtype) call crashes for string dtypes)")
        self.dtype = torch.float32
        if table is None:
            i = torch.arange(num_steps, dtype=torch.float32)
            t = (sigma_max ** (1 / rho) + i / (num_steps - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho
        else:
            t = table
        self.t_steps = torch.cat([t, torch.zeros(1)])       # constructor-only: never rewritten (captured solves rely on it)
        self._graphs = weakref.WeakKeyDictionary()      # model -> {(shapes, device[, guide]): captured solve}
        self.guide = guide
        self.guidance = guidance
        self.guidance_interval = guidance_interval
        self.guided_evaluations()                       # (validates guidance and guidance_interval)
        self._check_stream()

    # ------------------------------------------------------------------ guidance
    def guided_evaluations(self) -> tuple[bool, ...]:
        """Which of the 2N-1 network evaluations are guided, in loop order: Euler at t_0, correction at t_1, Euler at
        t_1, ..., Euler at t_{N-1}.  Host only; raises ValueError on an invalid guidance setting."""
        w = float(self.guidance)
        if not math.isfinite(w):
            raise ValueError(f"DeterministicSolver: guidance must be finite, got {self.guidance}")
        if isinstance(self.guide, str) and self.guide != UNCONDITIONAL:
            raise ValueError(f"DeterministicSolver: guide must be a network, None or {UNCONDITIONAL!r}, got "
                             f"{self.guide!r}")
        if w != 1.0 and self.guide is None:
            raise ValueError(f"DeterministicSolver: guidance={w} needs a guide network (guide=None)")
        if self.guidance_interval is not None:
            lo, hi = (float(v) for v in self.guidance_interval)
            if not 0.0 <= lo < hi:
                raise ValueError(f"DeterministicSolver: guidance_interval (lo, hi) needs 0 <= lo < hi, got "
                                 f"{tuple(self.guidance_interval)}")
        sigmas = self._evaluation_sigmas()
        if w == 1.0:
            return (False,) * len(sigmas)
        if self.guidance_interval is None:
            return (True,) * len(sigmas)
        return tuple(lo < s <= hi for s in sigmas)

    def _evaluation_sigmas(self) -> list[float]:
        """the sigma of each of the 2N-1 evaluations, in loop order (the fp32 table values, exactly)"""
        ts = self.t_steps.tolist()
        return [ts[i // 2 + i % 2] for i in range(2 * self.num_steps - 1)]

    def _check_stream(self) -> None:
        """the seed and solve index of the in-kernel noise (inpainting; the churn of StochasticSolver)"""
        _check_uint(self.seed, 64, "seed")
        _check_uint(self.solve_index, 32, "solve_index")

    # ------------------------------------------------------------------ image conditioning
    def _conditioning(self, x0, start_step, image, mask):
        """Validate start_step / image / mask of a solve against x0 on the host (shapes, dtypes and devices: nothing is
        read from a device) and return (start, image, mask as uint8 [B or 1, H*W]); None for the plain solve."""
        _check_step("solve", "start_step", start_step, self.num_steps)
        if mask is not None and image is None:
            raise ValueError("solve: mask needs image (the known pixels)")
        if image is None and start_step == 0:
            return None
        if image is not None:
            _check_float("solve", "image", image)
            if tuple(image.shape) != tuple(x0.shape):
                raise ValueError(f"solve: image must have x0's shape {tuple(x0.shape)}, got {tuple(image.shape)}")
        if mask is not None:
            if x0.dim() != 4:
                raise ValueError(f"solve: a mask needs x0 of shape [B, C, H, W], got {tuple(x0.shape)}")
            mask = _mask_u8(mask, x0.shape)
            self._check_stream()
            if self.num_steps >= ops.INPAINT_MAX_STEPS:
                raise ValueError(f"solve: inpainting needs num_steps < {ops.INPAINT_MAX_STEPS}")
        for t, name in ((image, "image"), (mask, "mask")):
            if t is not None and t.device != x0.device:
                raise ValueError(f"solve: {name} is on {t.device}, x0 on {x0.device}")
        return start_step, image, mask

    def _blend(self, x, cond, t, step):
        return ops.inpaint_blend(x, cond.image, cond.mask, t, cond.rec, step)

    def _solve_done(self, masked: bool) -> None:
        """after every solve: an inpainting solve has used up the noise of solve_index"""
        if masked:
            self.solve_index += 1

    @staticmethod
    def _restoration(x0, mask, degradation, measurement):
        """Validate degradation / measurement of a solve against x0 on the host (nothing is read from a device) and
        return them; None without them."""
        if degradation is None and measurement is None:
            return None
        if degradation is None or measurement is None:
            raise ValueError("solve: degradation and measurement go together (the operator and its y)")
        if not isinstance(degradation, LinearDegradation):
            raise ValueError(f"solve: degradation must be a LinearDegradation, got {type(degradation).__name__}")
        if mask is not None:
            raise ValueError("solve: mask (inpainting by replacement) and measurement (restoration) are two "
                             "conditionings; their combination is not implemented")
        _check_measurement(x0, degradation, measurement)
        return degradation, measurement

    # ------------------------------------------------------------------ subclass hooks (StochasticSolver)
    def _graph_key_extra(self, start_step: int = 0) -> tuple:
        """what the subclass adds to the key of a captured solve"""
        return ()

    def _solve_state(self, x0, start_step: int = 0):
        """per-solve device tensors the loop reads (a captured entry owns its own), written for this solve; or None.
        x0: the solve's fp32 initial noise (its shape and device)"""
        return None

    def _write_solve_state(self, state) -> None:
        """rewrite an entry's device tensors before a replay"""

    def _step_start(self, x, i, ts, t_dev, state):
        """the state, sigma and device sigma the step-i Euler evaluation starts from"""
        return x, ts[i], t_dev[i]

    def _check_guide(self, model, device, class_labels):
        """the checks that need the networks: run before any launch of a solve that evaluates the guide"""
        from .edm import EDM
        if _is_unconditional(self.guide):
            owner = getattr(model, "__self__", model)
            if not (isinstance(owner, EDM) and owner.conditional):
                raise ValueError("DeterministicSolver: guide='unconditional' needs a class-conditional EDM as the model")
            if class_labels is None:
                raise ValueError("DeterministicSolver: guide='unconditional' needs class_labels (without them the "
                                 "model's evaluation is the unconditional one already)")
            return
        guide = getattr(self.guide, "__self__", self.guide)
        if isinstance(guide, torch.nn.Module):
            if guide.training:
                raise ValueError("DeterministicSolver: the guide network is in training mode; call guide.eval()")
            t = next(guide.parameters(), None)
            if t is not None and t.device != device:
                raise ValueError(f"DeterministicSolver: the guide network is on {t.device}, the solve on {device}")
        owner = getattr(model, "__self__", model)
        if isinstance(guide, EDM) and isinstance(owner, EDM):
            g, m = guide.denoiser, owner.denoiser
            if (g.in_channels, g.out_channels) != (m.in_channels, m.out_channels):
                raise ValueError(f"DeterministicSolver: guide channels (in {g.in_channels}, out {g.out_channels}) differ "
                                 f"from the model's (in {m.in_channels}, out {m.out_channels})")

    def _guide_eval(self, model, x, sigma, class_labels):
        """D_guide of one guided evaluation (the one place that resolves guide='unconditional')"""
        if _is_unconditional(self.guide):
            return model(x, sigma, None).float().contiguous()
        return self.guide(x, sigma, class_labels).float().contiguous()

    # ------------------------------------------------------------------ eager
    def _evaluate(self, model, x, sigma, class_labels, guided: bool, w_dev, rest):
        """One network evaluation at (x, sigma): (D, Dg).  Dg is the guide's evaluation when this one is guided and the
        update kernel is to mix it in; with a restoration the projection has mixed it already and D is the projected
        (and mixed) evaluation, for the unguided update."""
        D = model(x, sigma, class_labels).float().contiguous()
        Dg = self._guide_eval(model, x, sigma, class_labels) if guided else None
        if rest is not None:
            return rest.project(D, Dg, w_dev), None
        return D, Dg

    def _step(self, evaluate, x1, i, ts, t_dev, guided, w_dev, state):
        """step i of the loop, t_i -> t_{i+1}: Euler and, but for the last step, the Heun correction"""
        return self._heun_step(evaluate, x1, i, ts, t_dev, guided, w_dev, state)[1]

    def _heun_step(self, evaluate, x1, i, ts, t_dev, guided, w_dev, state):
        """the Heun step i as (dx, x_{i+1}): dx is the Euler slope at the step's start, which trace() records"""
        x, t0, s0 = self._step_start(x1, i, ts, t_dev, state)
        t1 = ts[i + 1]
        D, Dg = evaluate(x, s0, guided[2 * i])
        dx, x1 = ops.heun_euler(x, D, t0, t1) if Dg is None else ops.heun_euler_guided(x, D, Dg, w_dev, t0, t1)
        if i < self.num_steps - 1:
            D1, Dg1 = evaluate(x1, t_dev[i + 1], guided[2 * i + 1])
            x1 = ops.heun_correct(x, dx, x1, D1, t0, t1) if Dg1 is None else \
                ops.heun_correct_guided(x, dx, x1, D1, Dg1, w_dev, t0, t1)
        return dx, x1

    # ------------------------------------------------------------------ the teacher's recorder
    def _check_trace(self) -> None:
        """which solvers can record their solve (the Heun ones whose steps start at the table's own states)"""
        if type(self)._step is not DeterministicSolver._step:
            raise ValueError(f"{type(self).__name__}.trace: the recorder follows the Heun step of DeterministicSolver; "
                             f"{type(self).__name__} takes another step")
        if type(self)._step_start is not DeterministicSolver._step_start and self._graph_key_extra():
            raise ValueError(f"{type(self).__name__}.trace: a churned solve is not an ODE and has no trajectory to record; "
                             "set S_churn = 0 (or use DeterministicSolver)")

    @torch.no_grad()
    def trace(self, model, x0, class_labels=None, *, graph: bool = False, start_step: int = 0, image=None, mask=None,
              degradation=None, measurement=None, operator=None, dps_scale=None) -> Trajectory:
        """The plain eager Heun solve with what its loop computes kept: Trajectory(x, slope, sigmas), x fp32
        [N + 1, B, ...] the states at t_0 .. t_N (x[0] = ops.scale_f32(x0, t_0) and x[N] = solve(model, x0, labels), bit
        for bit), slope fp32 [N, B, ...] the Euler slope at (x_i, t_i) as ops.heun_euler / heun_euler_guided return it (of
        the mixed D with a guide; guidance_interval is honoured).  The two buffers are allocated once and written row by
        row.  Image conditioning, restoration, posterior sampling and graph=True raise ValueError."""
        for name, on in (("graph=True", graph), ("start_step", start_step != 0), ("image", image is not None),
                         ("mask", mask is not None), ("degradation", degradation is not None),
                         ("measurement", measurement is not None), ("operator", operator is not None),
                         ("dps_scale", dps_scale is not None)):
            if on:
                raise ValueError(f"{type(self).__name__}.trace: {name} is not implemented for the recorder (it runs the "
                                 "plain eager solve); use solve")
        self._check_trace()
        guided = self.guided_evaluations()
        _check_float("trace", "x0", x0)
        if x0.dim() < 2 or x0.numel() == 0:
            raise ValueError(f"trace: x0 must be a non-empty [B, ...] tensor, got {tuple(x0.shape)}")
        _check_gpu(type(self).__name__, "x0", x0)
        if any(guided):
            self._check_guide(model, x0.device, class_labels)
        x0 = x0.float().contiguous()
        N, ts, t_dev = self.num_steps, self.t_steps.tolist(), self.t_steps.to(x0.device)
        w_dev = torch.full((1,), float(self.guidance), device=x0.device) if any(guided) else None
        X = torch.empty((N + 1, *x0.shape), dtype=torch.float32, device=x0.device)
        slope = torch.empty((N, *x0.shape), dtype=torch.float32, device=x0.device)

        def evaluate(x, sigma, flag):
            return self._evaluate(model, x, sigma, class_labels, flag, w_dev, None)
        X[0].copy_(ops.scale_f32(x0, ts[0]))
        for i in range(N):
            dx, x1 = self._heun_step(evaluate, X[i], i, ts, t_dev, guided, w_dev, None)
            slope[i].copy_(dx)
            X[i + 1].copy_(x1)
        return Trajectory(X, slope, self.t_steps.clone())

    # ------------------------------------------------------------------ diffusion posterior sampling
    def _posterior(self, model, x0, guided, mask, graph, degradation, operator, measurement, dps_scale):
        """Validate operator / measurement / dps_scale of a solve on the host (nothing is read from a device) and return
        (operator, measurement, scale); None without an operator."""
        if operator is None:
            if dps_scale is not None:
                raise ValueError("solve: dps_scale needs operator= (the measurement operator of posterior sampling)")
            return None
        if degradation is not None:
            raise ValueError("solve: degradation= (DDNM projection) and operator= (posterior sampling) are two ways to use a "
                             "measurement; give one")
        if not isinstance(operator, (LinearDegradation, GaussianBlur)):
            raise ValueError(f"solve: operator must be a LinearDegradation or a GaussianBlur, got {type(operator).__name__}")
        if measurement is None:
            raise ValueError("solve: operator and measurement go together (the operator and its y)")
        if self.guide is not None or any(guided):
            raise ValueError("solve: operator= (posterior sampling) with a guide is not implemented")
        if mask is not None:
            raise ValueError("solve: operator= (posterior sampling) with mask= (inpainting by replacement) is not implemented")
        if type(self)._step is not DeterministicSolver._step:
            raise ValueError(f"solve: operator= (posterior sampling) needs a Heun solver, not {type(self).__name__}")
        if graph:
            raise ValueError("solve: operator= (posterior sampling) with graph=True is not implemented (the step runs a "
                             "backward pass)")
        scale = 1.0 if dps_scale is None else dps_scale
        if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale) or scale < 0:
            raise ValueError(f"solve: dps_scale must be a finite number >= 0, got {dps_scale!r}")
        _check_measurement(x0, operator, measurement)
        from . import vjp
        parts = vjp._library_parts(model)
        if parts is not None and parts[1].eval_dtype != "bf16":
            raise ValueError(f"solve: operator= (posterior sampling) needs the bf16 path (the one with a backward pass); the "
                             f"denoiser evaluates in {parts[1].eval_dtype!r}: set_eval_dtype(\"bf16\") / --network_dtype bf16")
        return operator, measurement, float(scale)

    def _dps_step(self, model, class_labels, x1, i, ts, t_dev, state, dps):
        """step i of a posterior-sampling solve (Chung et al. 2023 in EDM / Heun form): the ordinary step from the Euler
        evaluation D -- taken with its input gradient -- then x' + (zeta / ||r||) J^T A^T r, r = y - A D"""
        from .vjp import open_input_vjp
        x, t0, s0 = self._step_start(x1, i, ts, t_dev, state)
        t1 = ts[i + 1]
        D, pullback = open_input_vjp(model, x, s0, class_labels)
        D = D.contiguous()
        r, nrm = ops.dps_residual(dps.y, dps.op.measure(D))
        g = pullback(dps.op.adjoint(r, D.shape[1])).contiguous()
        dx, x1 = ops.heun_euler(x, D, t0, t1)
        if i < self.num_steps - 1:
            D1 = model(x1, t_dev[i + 1], class_labels).float().contiguous()
            x1 = ops.heun_correct(x, dx, x1, D1, t0, t1)
        return ops.dps_update(x1, g, nrm, dps.scale)

    def _loop(self, model, x0, class_labels, t_dev, guided, w_dev, state=None, cond=None, rest=None, dps=None):
        ts = self.t_steps.tolist()
        k = 0 if cond is None else cond.start
        masked = cond is not None and cond.mask is not None

        def evaluate(x, sigma, flag):
            return self._evaluate(model, x, sigma, class_labels, flag, w_dev, rest)
        x = ops.scale_f32(x0, ts[0]) if cond is None else ops.state_init(x0, ts[k], cond.image)
        for i in range(k, self.num_steps):
            if masked:
                x = self._blend(x, cond, ts[i], i)
            if dps is not None:
                x = self._dps_step(model, class_labels, x, i, ts, t_dev, state, dps)
                continue
            x = self._step(evaluate, x, i, ts, t_dev, guided, w_dev, state)
        if masked:
            x = self._blend(x, cond, 0.0, self.num_steps)
        return x

    @torch.no_grad()
    def solve(self, model, x0, class_labels=None, graph: bool = False, *, start_step: int = 0, image=None, mask=None,
              degradation=None, measurement=None, operator=None, dps_scale=None):
        cond = self._conditioning(x0, start_step, image, mask)
        guided = self.guided_evaluations()
        dps = self._posterior(model, x0, guided, mask, graph, degradation, operator, measurement, dps_scale)
        rest = None if dps is not None else self._restoration(x0, mask, degradation, measurement)
        _check_gpu("DeterministicSolver", "x0", x0)
        if any(guided):
            self._check_guide(model, x0.device, class_labels)
        in_dtype = x0.dtype
        x0 = x0.float().contiguous()
        masked = False
        if cond is not None:
            k, image, mask = cond
            masked = mask is not None
            cond = _Conditioning(k, None if image is None else image.float().contiguous(), mask,
                                 ops.churn_record(self.seed, self.solve_index, x0.device) if masked else None)
        if rest is not None:
            rest = _Restoration(rest[0].scale, rest[0].gray, rest[1].float().contiguous())
        if dps is not None:
            dps = _Dps(dps[0], dps[1].float().contiguous(), dps[2])
        start = 0 if cond is None else cond.start
        if not graph:
            t_dev = self.t_steps.to(x0.device)
            w_dev = torch.full((1,), float(self.guidance), device=x0.device) if any(guided) else None
            state = self._solve_state(x0, start)
            out = self._loop(model, x0, class_labels, t_dev, guided, w_dev, state, cond, rest, dps).to(in_dtype)
            self._solve_done(masked)
            return out
        mode = _Mode(self._graph_key_extra(start), lambda: self._solve_state(x0, start),
                     lambda e: self._loop(model, e.x, e.labels, e.t_dev, guided, e.w_dev, e.state, e.cond, e.rest),
                     self._write_solve_state)
        out = self._solve_graphed(model, x0, class_labels, mode, guided, cond, rest).to(in_dtype)
        # the Heun kernels leave a bit in the device health word when the state went non-finite: a replay that ran
        # with corrupted arguments fails HERE, loudly (one host sync per solve of 2N-1 network evaluations)
        ops.check_health(x0.device, "DeterministicSolver.solve(graph=True)")
        self._solve_done(masked)
        return out

    # ------------------------------------------------------------------ inversion
    def _check_invert(self) -> None:
        """which solvers can run the ODE upwards (subclasses refuse)"""

    def _invert_loop(self, model, image, class_labels, t_dev, end_step):
        ts = self.t_steps.tolist()
        x = image
        for i in range(self.num_steps - 1, end_step, -1):        # a full Heun step t_i -> t_{i-1}
            t0, t1 = ts[i], ts[i - 1]
            D = model(x, t_dev[i], class_labels).float().contiguous()
            dx, x1 = ops.heun_euler(x, D, t0, t1)
            D1 = model(x1, t_dev[i - 1], class_labels).float().contiguous()
            x = ops.heun_correct(x, dx, x1, D1, t0, t1)
        return ops.scale_f32(x, 1.0 / ts[end_step])

    @torch.no_grad()
    def invert(self, model, image, class_labels=None, graph: bool = False, *, end_step: int = 0):
        """Encode: run the probability-flow ODE up the sigma table, image -> latent.  ``image`` is taken as the state at
        t_{N-1} (sigma_min noise is negligible), the steps t_{N-1} -> t_{N-2} -> ... -> t_k, k = ``end_step``, are
        full Heun steps (Euler + correction, the kernels of ``solve``: their algebra does not care about the
        direction), 2(N - 1 - k) network evaluations.  Returns the UNIT-SCALE latent x_k / t_k, the convention of
        ``solve``'s x0: ``solve(model, invert(model, img, end_step=k), start_step=k)`` closes the loop.  Only D_main is
        evaluated: guided inversion is not implemented, ``guide`` and ``guidance`` are ignored here."""
        self._check_invert()
        _check_step("invert", "end_step", end_step, self.num_steps)
        _check_float("invert", "image", image)
        _check_gpu("DeterministicSolver", "image", image)
        in_dtype = image.dtype
        image = image.float().contiguous()
        if not graph:
            return self._invert_loop(model, image, class_labels, self.t_steps.to(image.device), end_step).to(in_dtype)
        mode = _Mode(("invert", end_step), lambda: None,
                     lambda e: self._invert_loop(model, e.x, e.labels, e.t_dev, end_step), lambda state: None)
        out = self._solve_graphed(model, image, class_labels, mode).to(in_dtype)
        ops.check_health(image.device, "DeterministicSolver.invert(graph=True)")
        return out

    # ------------------------------------------------------------------ likelihood
    def probe_widths(self, sigma_data: float = 0.5, delta: float | None = None) -> list[float]:
        """h_i = delta * sqrt(t_i^2 + sigma_data^2) for the N table entries: the half-width of the likelihood estimator's
        central difference at noise level t_i, relative to the rms of the state there.  fp64 from the fp32 table, rounded
        to fp32, as host floats.  Host only; raises ValueError unless delta is finite and > 0."""
        delta = self.delta if delta is None else delta
        try:
            d = float(delta)
        except (TypeError, ValueError):
            d = math.nan
        if isinstance(delta, bool) or not (math.isfinite(d) and d > 0.0):
            raise ValueError(f"log_likelihood: delta must be finite and > 0, got {delta!r}")
        t = self.t_steps[:self.num_steps].double()
        return (d * (t * t + float(sigma_data) ** 2).sqrt()).float().tolist()

    def _nll_state(self, image) -> _NllState:
        return _NllState(ops.churn_record(self.seed, self.solve_index, image.device),
                         torch.zeros(image.shape[0], dtype=torch.float64, device=image.device))

    def _nll_loop(self, model, image, class_labels, t_dev, end_step, K, hs, state):
        ts = self.t_steps.tolist()
        rec, L = state
        L.zero_()
        x = image
        if end_step < self.num_steps - 1:
            E = ops.nll_probe(image, hs[-1], rec, self.num_steps - 1, 0, K)
            for i in range(self.num_steps - 1, end_step, -1):        # invert's Heun step t_i -> t_{i-1} on (x, L)
                t0, t1 = ts[i], ts[i - 1]
                D = model(E, t_dev[i], class_labels).float().contiguous()
                dx, E1 = ops.heun_euler_div(E, D, t0, t1, hs[i], hs[i - 1], rec, i, L, K)
                D1 = model(E1, t_dev[i - 1], class_labels).float().contiguous()
                E = ops.heun_correct_div(E, dx, E1, D1, t0, t1, hs[i - 1], rec, i, L, K,
                                         h_next=hs[i - 1] if i - 1 > end_step else None)
            x = E
        ops.nll_prior(x, ts[end_step], L)
        return L, ops.scale_f32(x, 1.0 / ts[end_step])

    @torch.no_grad()
    def log_likelihood(self, model, image, class_labels=None, graph: bool = False, *, end_step: int = 0,
                       num_probes: int = 1, return_latent: bool = False):
        """log p(image) in nats under the sampler's own generative ODE, a [B] float64 tensor: the density of the
        NORMALISED image as given, taken as the state at t_{N-1} (``bits_per_dim`` carries it to pixel units).  The
        state takes ``invert``'s Heun steps t_{N-1} -> ... -> t_k, k = ``end_step``, unchanged, and along them

            L += (t_{i-1} - t_i) / 2 * (g(x_i, t_i) + g(x~_{i-1}, t_{i-1})),   g(x, t) = (d - q(x, t)) / t,
            log p(image) = log N(x_k; 0, t_k^2 I) + L,

        with q ~ tr dD/dx estimated without a backward pass: Hutchinson with ``num_probes`` Rademacher probes eps and a
        central difference through the network, q = mean_p eps_p . (D(x + h eps_p) - D(x - h eps_p)) / (2h),
        h = delta * sqrt(t^2 + sigma_data^2).  The 1 + 2 * num_probes evaluations go through the network as one batch:
        2(N - 1 - k) network calls, as for ``invert``, at (1 + 2 * num_probes) times the batch.  The probes are drawn in
        the kernels from ``seed`` and ``solve_index`` as the inpainting noise is, under a Philox tag of their own;
        ``solve_index`` increments after every likelihood solve, so repeated calls average independent probes.  L and
        the prior term are accumulated in fp64 on the device in a fixed order: eager == graph and run == run bit for bit.

        The network must evaluate in fp32 (``eval_dtype`` "f32x3" or "f32"): a difference quotient at bf16 evaluation
        error is meaningless, so "bf16" raises ValueError.  Only D_main is evaluated: guided likelihoods are not
        implemented, ``guide`` and ``guidance`` are ignored here, as in ``invert``.  With ``return_latent`` the result
        is (logp, latent), latent the unit-scale x_k / t_k that ``invert`` returns, bit for bit."""
        self._check_invert()
        _check_step("log_likelihood", "end_step", end_step, self.num_steps)
        if isinstance(num_probes, bool) or not isinstance(num_probes, int) or \
                not 1 <= num_probes <= ops.NLL_MAX_PROBES:
            raise ValueError(f"log_likelihood: num_probes must be an integer in [1, {ops.NLL_MAX_PROBES}], got "
                             f"{num_probes!r}")
        _check_float("log_likelihood", "image", image)
        if image.dim() < 2 or image.numel() == 0:
            raise ValueError(f"log_likelihood: image must be a non-empty [B, ...] tensor, got {tuple(image.shape)}")
        if self.num_steps >= ops.NLL_MAX_STEPS:
            raise ValueError(f"log_likelihood: needs num_steps < {ops.NLL_MAX_STEPS}")
        self._check_stream()
        owner = getattr(model, "__self__", model)
        hs = self.probe_widths(getattr(owner, "sigma_data", 0.5))
        for m, eval_dtype in _denoisers(owner):
            if eval_dtype == "bf16":
                raise ValueError("log_likelihood: the network evaluates in bf16; a difference quotient needs the fp32 "
                                 "evaluation path (set_eval_dtype('f32x3') or 'f32')")
            if m.training:
                raise ValueError("log_likelihood: the network is in training mode; call model.eval()")
        _check_gpu("DeterministicSolver", "image", image)
        in_dtype = image.dtype
        image = image.float().contiguous()
        if class_labels is not None:        # one label row per row of the evaluation batch
            class_labels = class_labels.repeat(1 + 2 * num_probes, *([1] * (class_labels.dim() - 1)))
        if not graph:
            logp, latent = self._nll_loop(model, image, class_labels, self.t_steps.to(image.device), end_step,
                                          num_probes, hs, self._nll_state(image))
        else:
            mode = _Mode(("nll", end_step, num_probes, float(self.delta)), lambda: self._nll_state(image),
                         lambda e: self._nll_loop(model, e.x, e.labels, e.t_dev, end_step, num_probes, hs, e.state),
                         lambda state: ops.churn_record(self.seed, self.solve_index, out=state.rec))
            logp, latent = self._solve_graphed(model, image, class_labels, mode)
            ops.check_health(image.device, "DeterministicSolver.log_likelihood(graph=True)")
        self.solve_index += 1
        return (logp, latent.to(in_dtype)) if return_latent else logp

    # ------------------------------------------------------------------ hipGraph
    def _solve_graphed(self, model, x0, class_labels, mode: _Mode, guided=(), cond=None, rest=None):
        """replay (after capturing, the first time) what ``mode`` describes on x0: the solve, the inversion or the
        likelihood"""
        ent = self._graph_entry(model, x0, class_labels, mode, guided, cond, rest)
        ent.graph.replay()
        return tuple(o.clone() for o in ent.out) if isinstance(ent.out, tuple) else ent.out.clone()

    def _graph_entry(self, model, x0, class_labels, mode: _Mode, guided=(), cond=None, rest=None) -> _Captured:
        """the captured entry of what ``mode`` describes (captured now, the first time), its static tensors written for this
        call: ready to replay"""
        # graphs are cached PER MODEL OBJECT (weakly: a new model allocated at a dead one's address must not replay the
        # dead one's graph, which id(model) as a key allowed)
        owner = getattr(model, "__self__", model)        # a bound method is a fresh object per access: key on its object
        per_model = self._graphs.get(owner)
        if per_model is None:
            per_model = self._graphs[owner] = {}
            # when the model is collected its captured solves go with it: give their launch-table slots and plan pins back
            weakref.finalize(owner, _release_solves, per_model)
        # the evaluation precision of the denoiser(s) is part of the key: set_eval_dtype() between two solves must not
        # replay a graph captured with the other path's kernels
        def eval_dtypes(net):
            return tuple(d for _, d in _denoisers(net))
        key = (tuple(x0.shape), None if class_labels is None else tuple(class_labels.shape), x0.device.index,
               eval_dtypes(owner))
        # a guided solve also keys on the guide (the entry holds it, so its id cannot be reused while the graph that
        # reads its weights exists) and on which evaluations are guided; NOT on the guidance weight, which the graph
        # reads from the entry's w_dev.  An unguided solve keeps the unguided key whatever guide is set.  The model as its
        # own guide is a constant tag: the entry then holds no guide (a wrapper referencing the model would keep the
        # model, the weak key of _graphs, alive)
        guide = getattr(self.guide, "__self__", self.guide) if any(guided) else None
        if _is_unconditional(guide):
            key += ((UNCONDITIONAL,), guided)
        elif guide is not None:
            key += (id(guide), eval_dtypes(guide), guided)
        key += mode.key
        if cond is not None:        # (the plain solve keeps the key it always had)
            key += ("conditioned", cond.start, cond.image is not None,
                    None if cond.mask is None else tuple(cond.mask.shape))
        if rest is not None:        # the measurement itself is the entry's static copy: a new y replays the same graph
            key += ("restore", rest.scale, rest.gray, tuple(rest.y.shape))
        ent = ops.lru_get(per_model, key)
        fresh = ent is None
        if fresh:
            _runtime_env.require_graph_replay_safe("DeterministicSolver.solve(graph=True)")
            # the entry's own tensors: x, labels, image, mask, noise record and y are copied before every replay
            ent = _Captured(
                graph=torch.cuda.CUDAGraph(), x=x0.clone(), labels=None if class_labels is None else class_labels.clone(),
                out=None, t_dev=self.t_steps.to(x0.device), token=None,
                w_dev=None if guide is None else torch.full((1,), float(self.guidance), device=x0.device),
                guide=None if _is_unconditional(guide) else guide, state=mode.state(),
                cond=None if cond is None else _Conditioning(cond.start, *(None if v is None else v.clone()
                                                                           for v in cond[1:])),
                rest=None if rest is None else rest._replace(y=rest.y.clone()))
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):          # warm-up outside capture (weight packs, lazy inits)
                mode.loop(ent)
            torch.cuda.current_stream().wait_stream(side)
            with ops.capturing(ent.graph) as capture:
                out = mode.loop(ent)
            ent = ent._replace(out=out, token=capture.token)
            ops.lru_put(per_model, key, ent, self.MAX_GRAPHS)
        # the captured evaluations read the persistent eval-mode weight packs: refresh them (a no-op unless the
        # master weights changed since the last solve: optimizer steps, EMA swap, load_state_dict) before replaying
        for net in (model, ent.guide):
            for m, _ in _denoisers(net):
                if not m.training:
                    m._prep_all()
        # what a replay reads that this call sets: the mode's state (a fresh entry's was written when it was made), the
        # guidance weight, and every per-call input as (the entry's static tensor, this call's value)
        if not fresh:
            mode.rewrite(ent.state)
        if ent.w_dev is not None:
            ent.w_dev.fill_(float(self.guidance))
        inputs = [(ent.x, x0), (ent.labels, class_labels)]
        if ent.rest is not None:
            inputs.append((ent.rest.y, rest.y))
        if ent.cond is not None:
            inputs += [(ent.cond.image, cond.image), (ent.cond.mask, cond.mask), (ent.cond.rec, cond.rec)]
        for static, value in inputs:
            if static is not None:
                static.copy_(value)
        return ent


class ChurnSchedule(NamedTuple):
    """Per-step churn of a StochasticSolver, fp32 tensors of num_steps entries."""
    gamma: torch.Tensor     # min(S_churn / N, sqrt(2) - 1) inside S_min <= t_i <= S_max, else 0
    t_hat: torch.Tensor     # t_i + gamma_i * t_i: the sigma the step's Euler evaluation sees
    c: torch.Tensor         # S_noise * sqrt(t_hat_i^2 - t_i^2): the scale of the fresh noise


class _ChurnState(NamedTuple):
    rec: torch.Tensor       # the device record of the noise stream (ops.churn_record)
    t_hat: torch.Tensor     # device table of t_hat
    steps: tuple            # per step: (churned, t_hat_i, c_i) as host floats


def _check_uint(v, bits: int, name: str) -> None:
    try:
        ok = not isinstance(v, bool) and int(v) == v and 0 <= int(v) < 1 << bits
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"StochasticSolver: {name} must be an integer in [0, 2**{bits}), got {v!r}")


class StochasticSolver(DeterministicSolver):
    """Algorithm 2 of Karras et al. 2022: the Heun solver with "churn".  Before step i, inside S_min <= t_i <= S_max,
    the state is lifted to t_hat_i = t_i + gamma_i t_i by fresh noise,

        x_hat = x_i + S_noise * sqrt(t_hat_i^2 - t_i^2) * n,   n ~ N(0, I),   gamma_i = min(S_churn / N, sqrt(2) - 1),

    and the Heun step runs from (x_hat, t_hat_i) to t_{i+1}.  Same arguments as DeterministicSolver, guidance included,
    plus keyword-only S_churn, S_min, S_max, S_noise (EDM's names and defaults) and ``seed``.

    The noise is drawn in the kernel (ops.heun_churn) from Philox4x32-10 keyed by ``seed`` with the counter holding
    (element, sample, step, solve index): it depends neither on the batch size nor on the launch geometry.  Every
    ``solve()`` draws the noise of solve ``solve_index`` and then increments it, so consecutive batches differ and a run
    is reproducible from ``seed``; setting ``solve_index`` back reproduces a solve.  A captured solve reads the seed
    and the index from a device record written before every replay, so neither is part of the graph key; the churn
    schedule is.  ``S_churn == 0`` is the DeterministicSolver solve: same kernels, same graph key, same result."""

    def __init__(self, num_steps: int = 18, sigma_min: float = 0.002, sigma_max: float = 80.0, rho: float = 7.0,
                 dtype: str | None = None, *, guide=None, guidance: float = 1.0,
                 guidance_interval: tuple[float, float] | None = None, S_churn: float = 0.0, S_min: float = 0.0,
                 S_max: float = math.inf, S_noise: float = 1.0, seed: int = 0, sigmas=None):
        self.S_churn = S_churn
        self.S_min = S_min
        self.S_max = S_max
        self.S_noise = S_noise
        super().__init__(num_steps, sigma_min, sigma_max, rho, dtype, guide=guide, guidance=guidance,
                         guidance_interval=guidance_interval, seed=seed, sigmas=sigmas)  # (validates the churn settings too)

    def churn_schedule(self) -> ChurnSchedule:
        """gamma_i, t_hat_i and c_i of every step, computed in fp64 from the fp32 sigma table and rounded to fp32
        (c_i from the rounded t_hat_i).  Host only; raises ValueError on an invalid churn setting or seed."""
        S_churn, S_noise = float(self.S_churn), float(self.S_noise)
        S_min, S_max = float(self.S_min), float(self.S_max)
        if not (math.isfinite(S_churn) and S_churn >= 0.0):
            raise ValueError(f"StochasticSolver: S_churn must be finite and >= 0, got {self.S_churn}")
        if not (math.isfinite(S_noise) and S_noise >= 0.0):
            raise ValueError(f"StochasticSolver: S_noise must be finite and >= 0, got {self.S_noise}")
        if not 0.0 <= S_min <= S_max:
            raise ValueError(f"StochasticSolver: needs 0 <= S_min <= S_max, got S_min={self.S_min}, S_max={self.S_max}")
        self._check_stream()
        t = self.t_steps[:-1].double()
        g = min(S_churn / self.num_steps, math.sqrt(2.0) - 1.0)
        gamma = ((t >= S_min) & (t <= S_max)).double() * g
        t_hat = (t + gamma * t).float()
        c = (S_noise * (t_hat.double() ** 2 - t ** 2).sqrt()).float()
        return ChurnSchedule(gamma.float(), t_hat, c)

    def _churn_steps(self) -> tuple:
        s = self.churn_schedule()
        return tuple((g > 0.0, th, c) for g, th, c in zip(s.gamma.tolist(), s.t_hat.tolist(), s.c.tolist()))

    def _evaluation_sigmas(self) -> list[float]:
        """the Euler evaluation of step i sees t_hat_i, its correction t_{i+1}"""
        th = [s[1] for s in self._churn_steps()]
        ts = self.t_steps.tolist()
        return [th[i // 2] if i % 2 == 0 else ts[i // 2 + 1] for i in range(2 * self.num_steps - 1)]

    def _graph_key_extra(self, start_step: int = 0) -> tuple:
        steps = self._churn_steps()
        return (steps,) if any(s[0] for s in steps) else ()

    def _solve_state(self, x0, start_step: int = 0):
        steps = self._churn_steps()
        if not any(s[0] for s in steps):
            return None
        return _ChurnState(ops.churn_record(self.seed, self.solve_index, x0.device),
                           torch.tensor([s[1] for s in steps], dtype=torch.float32, device=x0.device), steps)

    def _write_solve_state(self, state) -> None:
        if state is not None:
            ops.churn_record(self.seed, self.solve_index, out=state.rec)

    def _step_start(self, x, i, ts, t_dev, state):
        if state is None or not state.steps[i][0]:
            return x, ts[i], t_dev[i]
        _, t_hat, c = state.steps[i]
        return ops.heun_churn(x, c, state.rec, i), t_hat, state.t_hat[i]

    def _solve_done(self, masked: bool) -> None:
        self.solve_index += 1           # every solve, churned or not, draws from its own index

    def _check_invert(self) -> None:
        if any(s[0] for s in self._churn_steps()):
            raise ValueError("StochasticSolver.invert: a churned solve is not an ODE and has no inverse; set S_churn = 0 "
                             "(or use DeterministicSolver)")


class _MultistepState(NamedTuple):
    hist: tuple             # the solve's history buffers: the mixed D of the last steps, a ring of `order` tensors
    steps: tuple            # per step: (effective order k_i, a_i, c0_i, c1_i, c2_i) as host floats


def _check_multistep(num_steps, order) -> None:
    if isinstance(order, bool) or order not in (1, 2, 3):
        raise ValueError(f"MultistepSolver: order must be 1, 2 or 3, got {order!r}")
    if num_steps < 2:
        raise ValueError(f"MultistepSolver: needs num_steps >= 2, got {num_steps}")


class MultistepSolver(DeterministicSolver):
    """DPM-Solver++ multistep (Lu et al. 2022) in data-prediction form on the Karras sigma table of DeterministicSolver:
    one network evaluation per step, N in all, against Heun's 2N - 1.  With lambda_i = -log sigma_i, h_i = lambda_{i+1}
    - lambda_i and m_i the D of step i (after guidance mixing), step i computes

        x_{i+1} = a_i x_i + c0_i m_i + c1_i m_{i-1} + c2_i m_{i-2},   a_i = sigma_{i+1} / sigma_i,

    at effective order k_i = min(order, i + 1): k = 1 is EDM's Euler step, k = 2 k-diffusion's dpmpp_2m, k = 3 the
    third-order multistep update.  The last step is first order (sigma_N = 0 makes h infinite): x_N = m_{N-1}.  The
    coefficients are computed once on the host (multistep_coefficients()); the update is one fused kernel per evaluation
    (ops.dpm_multistep) that also writes m_i into a history buffer the solve owns (a captured entry owns its own).

    Same arguments as DeterministicSolver, guidance included, plus keyword-only ``order`` (1, 2 or 3).  Guidance flags
    (guided_evaluations()) are per evaluation, at sigma_0 ... sigma_{N-1}.  ``order`` is a plain attribute: a new order
    captures a new graph."""

    def __init__(self, num_steps: int = 18, sigma_min: float = 0.002, sigma_max: float = 80.0, rho: float = 7.0,
                 dtype: str | None = None, *, order: int = 2, guide=None, guidance: float = 1.0,
                 guidance_interval: tuple[float, float] | None = None, seed: int = 0, sigmas=None):
        if sigmas is not None:
            num_steps = _sigma_table("MultistepSolver", sigmas).numel()
        _check_multistep(num_steps, order)
        self.order = order
        super().__init__(num_steps, sigma_min, sigma_max, rho, dtype, guide=guide, guidance=guidance,
                         guidance_interval=guidance_interval, seed=seed, sigmas=sigmas)

    def _steps(self, start_step: int = 0) -> tuple:
        """(k_i, a_i, c0_i, c1_i, c2_i) per step: the effective order and the fp32 coefficients as host floats.  A
        solve entering at start_step has no history there: k_i = min(order, i - start_step + 1) (the rows before
        start_step are those of a full solve; such a solve does not run them)"""
        _check_multistep(self.num_steps, self.order)
        N, order = self.num_steps, int(self.order)
        _check_step("MultistepSolver", "start_step", start_step, N)
        sig = self.t_steps.double().tolist()                # fp64 from the fp32 table
        lam = [-math.log(v) for v in sig[:N]]               # lambda_N = +inf
        steps = []
        for i in range(N):
            if i == N - 1:                                  # h = inf: a = 0, e = -1
                steps.append((1, 0.0, 1.0, 0.0, 0.0))
                continue
            k = min(order, i + 1 if i < start_step else i - start_step + 1)
            h = lam[i + 1] - lam[i]
            a = sig[i + 1] / sig[i]
            e = math.expm1(-h)
            if k == 1:
                row = (a, -e, 0.0, 0.0)
            elif k == 2:
                r = (lam[i] - lam[i - 1]) / h
                row = (a, -e * (1.0 + 0.5 / r), e * 0.5 / r, 0.0)
            else:
                # x_{i+1} = a x - e m_i + A D1 - B D2 with D1 = (1 + q) D1_0 - q D1_1, D2 = (D1_0 - D1_1) / (r0 + r1),
                # D1_0 = (m_i - m_{i-1}) / r0 and D1_1 = (m_{i-1} - m_{i-2}) / r1, collected per m
                r0 = (lam[i] - lam[i - 1]) / h
                r1 = (lam[i - 1] - lam[i - 2]) / h
                A, B = e / h + 1.0, (e + h) / (h * h) - 0.5
                q, s = r0 / (r0 + r1), r0 + r1
                row = (a,
                       -e + A * (1.0 + q) / r0 - B / (r0 * s),
                       -A * ((1.0 + q) / r0 + q / r1) + B * (1.0 / r0 + 1.0 / r1) / s,
                       A * q / r1 - B / (r1 * s))
            steps.append((k,) + row)
        return tuple((k,) + tuple(torch.tensor(row, dtype=torch.float64).float().tolist())
                     for k, *row in steps)

    def multistep_coefficients(self, start_step: int = 0) -> torch.Tensor:
        """(N, 4) fp32 tensor of the rows (a_i, c0_i, c1_i, c2_i): computed in fp64 from the fp32 sigma table, rounded to
        fp32.  The last row is (0, 1, 0, 0).  With start_step = k the order restarts there (row k is first order), as in
        solve(..., start_step=k).  Host only; raises ValueError on an invalid order, num_steps or start_step."""
        return torch.tensor([s[1:] for s in self._steps(start_step)], dtype=torch.float32)

    def _evaluation_sigmas(self) -> list[float]:
        """one evaluation per step, at sigma_0 ... sigma_{N-1}"""
        _check_multistep(self.num_steps, self.order)
        return self.t_steps.tolist()[:self.num_steps]

    def _graph_key_extra(self, start_step: int = 0) -> tuple:
        # the coefficients are kernel arguments baked into a capture: a new order is a new graph
        return ("multistep", self._steps(start_step))

    def _check_invert(self) -> None:
        raise ValueError("MultistepSolver.invert: a multistep inversion is not implemented; invert with "
                         "DeterministicSolver (Heun) on the same sigma table")

    def _solve_state(self, x0, start_step: int = 0):
        steps = self._steps(start_step)
        L = int(self.order) if self.order > 1 else 0
        return _MultistepState(tuple(torch.empty_like(x0) for _ in range(L)), steps)

    def _step(self, evaluate, x, i, ts, t_dev, guided, w_dev, state):
        hist, (k, a, c0, c1, c2) = state.hist, state.steps[i]
        L = len(hist)
        D, Dg = evaluate(x, t_dev[i], guided[i])    # with a restoration m_i is the projected (and mixed) evaluation
        return ops.dpm_multistep(x, D, a, c0, c1, c2, Dg=Dg, w_dev=None if Dg is None else w_dev,
                                 m1=hist[(i - 1) % L] if k >= 2 else None, m2=hist[(i - 2) % L] if k >= 3 else None,
                                 m_out=hist[i % L] if L and i < self.num_steps - 1 else None)


class _IteratedSolver(DeterministicSolver):
    """What AdaptiveSolver and ParallelSolver share on the host: both integrate the plain table's span with plain guidance
    and refuse the rest.  _REFUSAL is the subclass's one sentence, "<the ... solver> (<what it does instead>)"."""
    _REFUSAL: str

    def _refuse(self, who: str, **given) -> None:
        for name, on in given.items():
            if on:
                raise ValueError(f"{type(self).__name__}.{who}: {name} is not implemented for {self._REFUSAL}; use "
                                 "DeterministicSolver")

    def trace(self, *args, **kwargs):
        raise ValueError(f"{type(self).__name__}.trace: the recorder is not implemented for {self._REFUSAL}; use "
                         "DeterministicSolver")

    def _check_tolerances(self) -> None:
        for name in ("rtol", "atol"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"{type(self).__name__}: {name} must be a finite number >= 0, got {v!r}")

    def _check_span(self) -> None:
        lo, hi = self.t_steps[self.num_steps - 1].item(), self.t_steps[0].item()
        if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo < hi):
            raise ValueError(f"{type(self).__name__}: needs 0 < sigma_min < sigma_max, got {self.sigma_min}, "
                             f"{self.sigma_max}")

    @staticmethod
    def _check_batch(who: str, name: str, t) -> None:
        _check_float(who, name, t)
        if t.dim() < 2 or t.numel() == 0:
            raise ValueError(f"{who}: {name} must be a non-empty [B, ...] tensor, got {tuple(t.shape)}")

    def _mixed_evaluation(self, model, class_labels, guided: bool, w_dev, calls=None):
        """evaluate(x, sigma) -> D of the model, with plain guidance D = Dg + w (Dm - Dg) mixed on the device; calls
        (optional [network, guide] list) counts the batch calls"""
        def evaluate(xs, sigma):
            if calls is not None:
                calls[0] += 1
                calls[1] += int(guided)
            D = model(xs, sigma, class_labels).float().contiguous()
            if not guided:
                return D
            Dg = self._guide_eval(model, xs, sigma, class_labels)
            return ops.dpm_multistep(xs, D, 0.0, 1.0, 0.0, 0.0, Dg=Dg, w_dev=w_dev)     # (the mix, bit for bit)
        return evaluate

    @staticmethod
    def _closing_step(evaluate, x, sigma, t: float):
        """the table's closing Euler step t -> 0 (sigma: t on the device): one batch evaluation"""
        return ops.heun_euler(x, evaluate(x, sigma), t, 0.0)[1]


class AdaptiveStats(NamedTuple):
    """what the last adaptive solve did (AdaptiveSolver.last_stats)"""
    accepted: torch.Tensor      # int64 [B] on the host: accepted steps per sample
    rejected: torch.Tensor      # int64 [B] on the host: rejected steps per sample
    iterations: int             # controlled steps of the batch = max(accepted + rejected)
    evaluations: int            # calls of the network, one per batch call (2 per iteration, + 1 for solve's closing step)
    guide_evaluations: int      # calls of the guide, counted apart


class AdaptiveSolver(_IteratedSolver):
    """The probability-flow ODE integrated to a tolerance instead of on a table: the embedded Heun(2) / Euler(1) pair
    with local extrapolation, every sample at its own time and step size, the step controller on the device
    (csrc/adaptive.hip).  A trial step from t to t1 takes the Euler result x1 and the Heun result y, measures

        E = sqrt(mean_j ((y_j - x1_j) / (atol + rtol max(|x_j|, |y_j|)))^2)        (per sample, fp64, order-fixed)

    and is accepted iff E <= 1: then x <- y (the second-order result: local extrapolation), t <- t1.  Either way the
    next step is h <- (t1 - t) clamp(safety E^(-1/2), fac_min, fac_max), with fac_max replaced by 1 on a rejection and on
    the step after one; a step that would pass t_end, or come within 1 % of |h| of it, ends on t_end exactly.  One
    iteration is two network evaluations of the whole batch plus four small kernels; samples that are done ride along
    unchanged.  The loop is eager: after each iteration the host reads the 4-byte count of samples still active.

    ``solve`` starts from sigma_max * x0, integrates sigma_max -> sigma_min (the ends of the parent's Karras table for
    ``num_steps``, whose first step is also the first proposal h0) and finishes with the table's closing Euler step
    sigma_min -> 0.  ``invert`` takes the image as the state at sigma_min, integrates upwards (h0: the table's last
    step, reversed) and returns x / sigma_max, so ``solve(model, invert(model, img))`` closes the loop; only D_main is
    evaluated there.  Plain guidance (``guide``, ``guidance``) mixes D = Dg + w (Dm - Dg) before the update;
    ``guidance_interval`` raises ValueError (it would be per sample), and so do graph=True, start_step, image, mask,
    degradation, operator / dps_scale, end_step and log_likelihood, on the host before any launch.  RuntimeError when
    ``max_iterations`` is reached with samples still active or a sample's step fell under ``h_floor`` |t|.
    ``last_stats`` (AdaptiveStats) describes the last solve or inversion."""

    _REFUSAL = "the adaptive solver (it integrates sigma_max <-> sigma_min eagerly, every sample at its own sigma)"

    def __init__(self, num_steps: int = 18, sigma_min: float = 0.002, sigma_max: float = 80.0, rho: float = 7.0,
                 dtype: str | None = None, *, guide=None, guidance: float = 1.0,
                 guidance_interval: tuple[float, float] | None = None, seed: int = 0, rtol: float = 1e-3,
                 atol: float = 1e-4, max_iterations: int = 1024, safety: float = 0.9, fac_min: float = 0.2,
                 fac_max: float = 5.0, h_floor: float = 1e-6, sigmas=None):
        self._refuse("__init__", sigmas=sigmas is not None)     # (it has no table: it integrates between the table's ends)
        self.rtol, self.atol, self.max_iterations = rtol, atol, max_iterations
        self.safety, self.fac_min, self.fac_max, self.h_floor = safety, fac_min, fac_max, h_floor
        self.last_stats = None
        if isinstance(num_steps, bool) or not isinstance(num_steps, int) or num_steps < 2:
            raise ValueError(f"AdaptiveSolver: needs num_steps >= 2 (the table whose first step is h0), got {num_steps!r}")
        super().__init__(num_steps, sigma_min, sigma_max, rho, dtype, guide=guide, guidance=guidance,
                         guidance_interval=guidance_interval, seed=seed)

    def guided_evaluations(self) -> tuple[bool, ...]:
        """(whether the evaluations are guided,): all of them or none.  Host only; raises ValueError on an invalid
        guidance or tolerance setting."""
        if self.guidance_interval is not None:
            raise ValueError("AdaptiveSolver: guidance_interval is not implemented (every sample is at its own sigma, so the "
                             "interval would hold per sample)")
        flags = super().guided_evaluations()
        self._check_adaptive()
        return (any(flags),)

    def _check_adaptive(self) -> None:
        self._check_tolerances()
        if not self.rtol + self.atol > 0:
            raise ValueError("AdaptiveSolver: rtol and atol must not both be 0")
        m = self.max_iterations
        if isinstance(m, bool) or not isinstance(m, int) or m < 1:
            raise ValueError(f"AdaptiveSolver: max_iterations must be an integer >= 1, got {m!r}")
        ops.check_controller(self.safety, self.fac_min, self.fac_max, self.h_floor)
        self._check_span()

    def span(self, upwards: bool = False) -> tuple[float, float, float]:
        """(t_start, t_end, h0) of ``solve`` (or of ``invert``, upwards) as the fp32 table values"""
        ts = self.t_steps.tolist()
        N = self.num_steps
        return (ts[N - 1], ts[0], ts[N - 2] - ts[N - 1]) if upwards else (ts[0], ts[N - 1], ts[1] - ts[0])

    def _integrate(self, model, x, class_labels, span, guided, w_dev, who):
        """x (fp32, owned: advanced in place) from t_start to t_end; returns x and the counting evaluation of (x, sigma),
        guidance mix included; last_stats is written"""
        t_start, t_end, h0 = span
        B, CHW, dev = x.shape[0], x.numel() // x.shape[0], x.device
        calls = [0, 0]
        evaluate = self._mixed_evaluation(model, class_labels, guided, w_dev, calls)
        state = ops.adapt_begin(B, t_start, t_end, h0, dev)
        rows = ops.adapt_rows(state)
        active = torch.zeros(1, dtype=torch.int32, device=dev)
        part = torch.empty((B, ops.NLL_MAX_CHUNKS), dtype=torch.float64, device=dev)
        accept = torch.empty(B, dtype=torch.uint8, device=dev)
        iterations, seen, left = 0, 0, B
        while left and iterations < self.max_iterations:
            D = evaluate(x, rows.t)
            dx, x1 = ops.adapt_euler(x, D, rows.t, rows.t1)
            D1 = evaluate(x1, rows.t1)
            y, _ = ops.adapt_correct(x, dx, x1, D1, rows.t, rows.t1, self.atol, self.rtol, part)
            ops.adapt_control(part, CHW, state, t_end, active, safety=self.safety, fac_min=self.fac_min,
                              fac_max=self.fac_max, h_floor=self.h_floor, accept=accept)
            ops.adapt_commit(x, y, accept)
            iterations += 1
            total = int(active.item())          # the one host read of an iteration: 4 bytes
            seen, left = total, total - seen
        host = state.cpu()
        status, t = host[4], host.view(torch.float32)[0]
        self.last_stats = AdaptiveStats(host[5].long(), host[6].long(), iterations, calls[0], calls[1])
        failed, live = status == ops.ADAPT_FAILED, status == ops.ADAPT_ACTIVE
        if bool(failed.any()):
            ops.health(dev).zero_()             # (the controller raised the bit for the failed samples: reported here)
            raise RuntimeError(f"AdaptiveSolver.{who}: the step of {int(failed.sum())} of {B} samples fell under h_floor = "
                               f"{self.h_floor} |t| at t = {t[failed].tolist()} (a non-finite state, or a tolerance "
                               "the fp32 state cannot meet)")
        if bool(live.any()):
            raise RuntimeError(f"AdaptiveSolver.{who}: {int(live.sum())} of {B} samples are still active after "
                               f"max_iterations = {self.max_iterations}, at t = {t[live].tolist()}")
        return x, evaluate

    @torch.no_grad()
    def solve(self, model, x0, class_labels=None, graph: bool = False, *, start_step: int = 0, image=None, mask=None,
              degradation=None, measurement=None, operator=None, dps_scale=None):
        self._refuse("solve", **{"graph=True": graph, "start_step": start_step != 0, "image": image is not None,
                                 "mask": mask is not None, "degradation": degradation is not None,
                                 "measurement": measurement is not None, "operator": operator is not None,
                                 "dps_scale": dps_scale is not None})
        guided, = self.guided_evaluations()
        self._check_batch("solve", "x0", x0)
        _check_gpu("AdaptiveSolver", "x0", x0)
        if guided:
            self._check_guide(model, x0.device, class_labels)
        span = self.span()
        w_dev = torch.full((1,), float(self.guidance), device=x0.device) if guided else None
        x = ops.scale_f32(x0.float().contiguous(), span[0])
        x, evaluate = self._integrate(model, x, class_labels, span, guided, w_dev, "solve")
        out = self._closing_step(evaluate, x, torch.full((1,), span[1], device=x.device), span[1])
        self.last_stats = self.last_stats._replace(evaluations=self.last_stats.evaluations + 1,
                                                   guide_evaluations=self.last_stats.guide_evaluations + int(guided))
        ops.check_health(x.device, "AdaptiveSolver.solve")
        return out.to(x0.dtype)

    @torch.no_grad()
    def invert(self, model, image, class_labels=None, graph: bool = False, *, end_step: int = 0):
        """Encode: the image, taken as the state at sigma_min, integrated upwards to sigma_max at the solver's tolerance;
        returns the unit-scale latent x / sigma_max.  Only D_main is evaluated (``guide`` and ``guidance`` are ignored)."""
        self._refuse("invert", **{"graph=True": graph, "end_step": end_step != 0})
        self._check_adaptive()
        self._check_batch("invert", "image", image)
        _check_gpu("AdaptiveSolver", "image", image)
        span = self.span(upwards=True)
        x = image.float().contiguous().clone()
        x, _ = self._integrate(model, x, class_labels, span, False, None, "invert")
        ops.check_health(x.device, "AdaptiveSolver.invert")
        return ops.scale_f32(x, 1.0 / span[1]).to(image.dtype)

    def log_likelihood(self, *args, **kwargs):
        raise ValueError("AdaptiveSolver.log_likelihood: an adaptive likelihood is not implemented (the divergence would "
                         "have to be integrated per sample); use DeterministicSolver")


class ParallelStats(NamedTuple):
    """what the last parallel solve did (ParallelSolver.last_stats)"""
    iterations: int                         # Picard iterations of the batch = max(per_sample_iterations)
    evaluations: int                        # batched calls of the network: order * iterations, + 1 for the closing step
    guide_evaluations: int                  # calls of the guide, counted apart
    rows: int                               # network rows evaluated in all: order * iterations * window * B + B
    sequential_evaluations: int             # order * (N - 1) + 1: what the table solver takes
    per_sample_iterations: torch.Tensor     # int64 [B] on the host: iterations until the sample's window reached the end


class _PicardState(NamedTuple):
    """the device state of one parallel solve (a captured entry owns its own)"""
    X: torch.Tensor         # fp32 [P + 1, B, ...]: the window, position-major
    Xnew: torch.Tensor      # the other buffer: the scan writes it, the slide reads it
    T: torch.Tensor         # fp32 [P + 1, B]: the times of the window positions
    state: torch.Tensor     # int32 [ops.PICARD_ROWS, B]
    stride: torch.Tensor    # int32 [B]
    active: torch.Tensor    # int32 [1]: the running count the host reads after every iteration
    part: torch.Tensor      # fp64 [B, P, chunks]
    tol: torch.Tensor       # fp64 [2]: atol, rtol
    t_dev: torch.Tensor     # the sigma table on the device


class ParallelSolver(_IteratedSolver):
    """The table solver's result computed in parallel over time (ParaDiGMS: Shih et al. 2023): Picard iteration of the
    Heun step (``order=2``) or the Euler step (``order=1``) of DeterministicSolver's table t_0 .. t_N over a window of
    ``window`` = P consecutive steps.  Every sample b holds the states at table indices s_b .. s_b + P as unknowns; one
    iteration evaluates the network at the first P of them in ONE batch of P * B rows (twice for Heun), rebuilds the
    window as x_{s+j+1} = x_s + sum_{k <= j} h_k slope_k(old iterate) (ops.picard_scan, a prefix sum in index order),
    measures per position

        E_j = sqrt(mean ((new - old) / (atol + rtol max(|old|, |new|)))^2)        (fp64, order-fixed)

    and slides the window past the m leading positions with E_j <= 1 and one more: the position after a converged
    prefix is one sequential step from a converged state (ops.picard_control, ops.picard_slide; the entering positions are
    initialised along the ODE's solution for a frozen denoised image, which sets the speed of convergence, never its
    limit).  Every sample advances by at least one step per iteration, so steps 0 .. N-2 take at most N - 1 iterations:
    the sequential depth is order * iterations + 1 network calls against the table solver's order * (N - 1) + 1.  The
    closing step t_{N-1} -> 0 is the table's Euler step at batch B.  The fixed point of the iteration is the table
    solver's result, and ``rtol = atol = 0`` (converged = no element moved, bit for bit) returns it: the bits of
    DeterministicSolver.solve for a network whose rows do not depend on their batch.

    Each sample has its own window start: a result does not depend on its batch mates.  Plain guidance (``guide``,
    ``guidance``) mixes D = Dg + w (Dm - Dg) before the update.  ``solve(graph=True)`` captures ONE iteration and replays
    it, with the host's 4-byte read of the active count between replays; tolerances and the guidance weight are re-read
    from device memory.  ``guidance_interval`` raises ValueError, and so do start_step, image, mask, degradation,
    measurement, operator, dps_scale, invert and log_likelihood, on the host before any launch.
    ``last_stats`` (ParallelStats) describes the last solve."""

    _REFUSAL = "the parallel solver (it iterates the plain table solve over a window of steps)"

    def __init__(self, num_steps: int = 18, sigma_min: float = 0.002, sigma_max: float = 80.0, rho: float = 7.0,
                 dtype: str | None = None, *, window: int = 16, order: int = 2, rtol: float = 1e-3, atol: float = 1e-4,
                 guide=None, guidance: float = 1.0, guidance_interval: tuple[float, float] | None = None, seed: int = 0,
                 sigmas=None):
        self.window, self.order, self.rtol, self.atol = window, order, rtol, atol
        self.last_stats = None
        if sigmas is not None:
            num_steps = _sigma_table("ParallelSolver", sigmas).numel()
        if isinstance(num_steps, bool) or not isinstance(num_steps, int) or num_steps < 2:
            raise ValueError(f"ParallelSolver: needs num_steps >= 2 (steps 0 .. N-2 are iterated, the last one closes), got "
                             f"{num_steps!r}")
        super().__init__(num_steps, sigma_min, sigma_max, rho, dtype, guide=guide, guidance=guidance,
                         guidance_interval=guidance_interval, seed=seed, sigmas=sigmas)

    def guided_evaluations(self) -> tuple[bool, ...]:
        """(whether the evaluations are guided,): all of them or none.  Host only; raises ValueError on an invalid
        guidance, window, order or tolerance setting."""
        if self.guidance_interval is not None:
            raise ValueError("ParallelSolver: guidance_interval is not implemented (the rows of one evaluation are at "
                             "different sigmas, so the interval would hold per row)")
        flags = super().guided_evaluations()
        self._check_parallel()
        return (any(flags),)

    def _check_parallel(self) -> None:
        P = self.window
        if isinstance(P, bool) or not isinstance(P, int) or not 1 <= P <= ops.PICARD_MAX_WINDOW:
            raise ValueError(f"ParallelSolver: window must be an integer in 1 .. {ops.PICARD_MAX_WINDOW}, got {P!r}")
        if isinstance(self.order, bool) or self.order not in (1, 2):
            raise ValueError(f"ParallelSolver: order must be 1 (Euler) or 2 (Heun), got {self.order!r}")
        self._check_tolerances()
        self._check_span()

    def _picard_state(self, x0) -> _PicardState:
        """the device state of a solve from x0 (fp32 unit noise), the window at the head of the table"""
        N, P, dev = self.num_steps, int(self.window), x0.device
        B, CHW = x0.shape[0], x0.numel() // x0.shape[0]
        t_dev = self.t_steps.to(dev)
        X, T, state = ops.picard_begin(x0, t_dev, N, P)
        return _PicardState(X, torch.empty_like(X), T, state, torch.zeros(B, dtype=torch.int32, device=dev),
                            torch.zeros(1, dtype=torch.int32, device=dev),
                            torch.empty((B, P, ops.picard_chunks(CHW)), dtype=torch.float64, device=dev),
                            ops.picard_tol(self.atol, self.rtol, dev), t_dev)

    def _iterate(self, model, labels, st: _PicardState, guided: bool, w_dev):
        """one Picard iteration on the state's buffers (what a captured entry replays); labels: repeated window times"""
        N, order = self.num_steps, int(self.order)
        P, B = st.X.shape[0] - 1, st.X.shape[1]
        rows = st.X[:P].view(P * B, *st.X.shape[2:])        # positions 0 .. P-1: one contiguous network batch
        t, t1 = st.T[:P].view(-1), st.T[1:].view(-1)
        evaluate = self._mixed_evaluation(model, labels, guided, w_dev)
        D = evaluate(rows, t)
        dx, X1 = ops.adapt_euler(rows, D, t, t1)
        D1 = evaluate(X1, t1) if order == 2 else None
        ops.picard_scan(st.X, dx, X1, D1, st.T, st.state, N=N, tol=st.tol, Xnew=st.Xnew, part=st.part)
        ops.picard_control(st.part, rows[0].numel(), st.state, N, P, st.active, stride=st.stride)
        ops.picard_slide(st.Xnew, D, st.stride, st.state, st.t_dev, N=N, X=st.X, T=st.T)
        return st.X

    @torch.no_grad()
    def solve(self, model, x0, class_labels=None, graph: bool = False, *, start_step: int = 0, image=None, mask=None,
              degradation=None, measurement=None, operator=None, dps_scale=None):
        self._refuse("solve", **{"start_step": start_step != 0, "image": image is not None, "mask": mask is not None,
                                 "degradation": degradation is not None, "measurement": measurement is not None,
                                 "operator": operator is not None, "dps_scale": dps_scale is not None})
        guided, = self.guided_evaluations()
        self._check_batch("solve", "x0", x0)
        if not x0.is_cuda or (class_labels is not None and not class_labels.is_cuda):
            raise ValueError("tinyedm_amd.ParallelSolver: x0 and class_labels must be GPU tensors (there is no CPU path)")
        if guided:
            self._check_guide(model, x0.device, class_labels)
        N, P, order, B = self.num_steps, int(self.window), int(self.order), x0.shape[0]
        in_dtype, x0 = x0.dtype, x0.float().contiguous()
        labels = None if class_labels is None else class_labels.repeat(P, *([1] * (class_labels.dim() - 1)))
        if not graph:
            w_dev = torch.full((1,), float(self.guidance), device=x0.device) if guided else None
            st = self._picard_state(x0)

            def iterate():
                self._iterate(model, labels, st, guided, w_dev)
        else:
            # one iteration is the captured unit.  The key: the window, the order and the table (kernel arguments of the
            # capture); the tolerances and the guidance weight are device state a replay re-reads
            mode = _Mode(("picard", P, order, tuple(self.t_steps.tolist())), lambda: self._picard_state(x0),
                         lambda e: self._iterate(model, e.labels, e.state, guided, e.w_dev), lambda state: None)
            ent = self._graph_entry(model, x0, labels, mode, (guided,))
            st, w_dev, iterate = ent.state, ent.w_dev, ent.graph.replay
            # the warm-up and earlier solves have moved the entry's window: back to the head of the table, from ent.x
            ops.picard_begin(ent.x, st.t_dev, N, P, X=st.X, T=st.T, state=st.state)
            st.active.zero_()
            ops.picard_tol(self.atol, self.rtol, x0.device, out=st.tol)
        iterations, seen, left = 0, 0, B
        while left:
            # position 1 of a window is one sequential step from a converged state: every active sample advances
            assert iterations < N - 1, f"ParallelSolver.solve: {left} samples still active after N - 1 = {N - 1} iterations"
            iterate()
            iterations += 1
            total = int(st.active.item())           # the one host read of an iteration: 4 bytes
            seen, left = total, total - seen
        # the table's closing Euler step t_{N-1} -> 0: one evaluation at batch B
        out = self._closing_step(self._mixed_evaluation(model, class_labels, guided, w_dev), st.X[0], st.t_dev[N - 1:N],
                                 self.t_steps[N - 1].item())
        evaluations = order * iterations + 1
        self.last_stats = ParallelStats(iterations, evaluations, evaluations if guided else 0,
                                        order * iterations * P * B + B, order * (N - 1) + 1, st.state[2].cpu().long())
        ops.check_health(x0.device, "ParallelSolver.solve")
        return out.to(in_dtype)

    def invert(self, *args, **kwargs):
        raise ValueError("ParallelSolver.invert: inversion is not implemented for the parallel solver; use "
                         "DeterministicSolver on the same sigma table")

    def log_likelihood(self, *args, **kwargs):
        raise ValueError("ParallelSolver.log_likelihood: likelihood evaluation is not implemented for the parallel solver; "
                         "use DeterministicSolver")
