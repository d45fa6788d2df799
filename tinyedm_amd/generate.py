"""Sampling entry point with the reference's surface (src/tinyedm/generate.py:8-47, 50-96): the same `generate(...)`
signature and the same command-line flags (`--ckpt_path --load_ema --output_dir --num_samples --image_size
--num_classes --batch_size --num_workers --num_steps`), running the hipGraph-captured Heun sampler on the HIP path.

    python -m tinyedm.generate --ckpt_path last.ckpt --load_ema --output_dir samples --num_samples 50000 \\
        --image_size 32 --num_classes 10 --batch_size 512

Precision: the denoiser is evaluated at fp32 accuracy BY DEFAULT, as the reference does (generate.py:39-44:
`L.Trainer(accelerator="gpu")`, i.e. 32-bit precision).  `--network_dtype f32x3` (default): fp32 activations, every conv product
as three bf16 MFMA passes over (hi, lo) operand pairs accumulated in fp32 -- 32-step trajectories 2e-6 from the exact-fp32 path
and <= 1e-4 from the fp32 oracle (tests/test_evalf32_gpu.py), 158 img/s on the CIFAR-10 net; `f32`: exact fp32 products
(the f32-input matrix instruction; the checker: 3e-7 from the oracle, 58 img/s); `bf16`: the opt-in fast mode, the training
path's kernels, 540 img/s, 1.3e-3 from the fp32 trajectory.
Extensions (all optional): `--network_dtype`,
`--in_channels` (the reference's noise dataset hard-codes 3; default = the checkpoint's
denoiser.in_channels), `--mean/--std` (default: the reference's CIFAR-10 constants), `--seed`, `--no_graph`, and
`--config_name` to sample from random-init weights of a config instead of a checkpoint (plumbing runs).
Guided sampling (DeterministicSolver): `--guide_ckpt_path [--guide_load_ema]` (or `--guide_config_name`, random init) loads
a guide network, evaluated at the same `--network_dtype`, and `--guidance W` samples with D = D_guide + W*(D_main - D_guide):
classifier-free guidance with an unconditional guide, autoguidance with a smaller / less-trained conditional one.
`--guidance_interval LO HI` guides only the evaluations with LO < sigma <= HI.  `--guidance 1` (the default) leaves the guide
unused and the output byte-identical to a run without one.
`--guide_unconditional` (instead of a guide network) is classifier-free guidance from the one checkpoint: the guide is the
model's own label-free evaluation, for a conditional model trained with `model.embedding.label_dropout=p`.

    python -m tinyedm.generate --ckpt_path cond.ckpt --load_ema --guide_unconditional --guidance 2 \\
        --output_dir samples --num_samples 50000 --image_size 32 --num_classes 10 --batch_size 512

    python -m tinyedm.generate --ckpt_path cond.ckpt --load_ema --guide_ckpt_path uncond.ckpt --guide_load_ema \\
        --guidance 2.0 --guidance_interval 0.28 5.42 --output_dir samples --num_samples 50000 --image_size 32 \\
        --num_classes 10 --batch_size 512
Stochastic sampling (StochasticSolver, Algorithm 2 of Karras et al. 2022): `--S_churn`, `--S_min`, `--S_max`, `--S_noise`
(EDM's names and defaults: 0, 0, inf, 1).  With `--S_churn` > 0 every step with S_min <= t_i <= S_max first adds fresh
noise, lifting the state to t_hat_i = (1 + min(S_churn / N, sqrt(2) - 1)) t_i; the noise is drawn in the kernel from
`--seed` (per rank, as the initial noise) and differs from batch to batch.  Guidance combines with it.  `--S_churn 0`
(the default) samples with the deterministic solver, byte-identical to a run without these flags.

    python -m tinyedm.generate --ckpt_path last.ckpt --load_ema --S_churn 40 --S_min 0.05 --S_max 50 --S_noise 1.003 \\
        --output_dir samples --num_samples 50000 --image_size 64 --num_classes 1000 --batch_size 512
Multistep sampling (MultistepSolver, DPM-Solver++ of Lu et al. 2022): `--solver dpmpp` with `--solver_order` 1, 2 (the
default, DPM-Solver++(2M)) or 3 spends one network evaluation per step, N in all against Heun's 2N - 1.  It combines
with every guidance flag; a nonzero `--S_churn` with it is an error.  `--solver heun` (the default) is the Heun solver,
byte-identical to a run without these flags.
Adaptive sampling (AdaptiveSolver): `--solver adaptive` integrates sigma_max -> sigma_min of the `--num_steps` table to a
tolerance, `--rtol` (1e-3) and `--atol` (1e-4), every image at its own step size, at most `--max_iterations` (1024)
controlled steps of two network evaluations each, and ends with the table's closing step; the loop is eager.
`--solver_report FILE.json` records {"accepted", "rejected": per image, "iterations": per batch, the totals and
"rejected_share"}.  It combines with `--guidance`, `--guide_unconditional` / a guide network and `--invert_to` (the
latents then close the loop with an adaptive solve); `--guidance_interval`, `--S_churn`, `--init_dir` without
`--invert_to`, `--start_step`, `--mask_box`, `--restore_*`, `--dps_scale` and `--likelihood_to` are errors.

    python -m tinyedm.generate --ckpt_path last.ckpt --load_ema --solver dpmpp --solver_order 2 --num_steps 32 \\
        --output_dir samples --num_samples 50000 --image_size 32 --num_classes 10 --batch_size 512
Parallel-in-time sampling (ParallelSolver; ParaDiGMS, Shih et al. 2023): `--solver picard` holds `--window P` (16)
consecutive steps of the table as unknowns, evaluates the network at all of them in one batch of P x batch_size rows
and iterates until they move by less than `--rtol` (1e-3) / `--atol` (1e-4): the Heun table solve (`--solver_order 1`:
Euler) at a sequential depth of 2 x iterations + 1 network calls instead of 2N - 1, for a few images at a time.
`--rtol 0 --atol 0` iterates to the fixed point itself.  `--solver_report FILE.json` records {"iterations": per batch,
"per_sample_iterations", "evaluations", "rows", "sequential_evaluations", ...}.  It combines with `--guidance`,
`--guide_unconditional` / a guide network and the captured graph; the flags `--solver adaptive` refuses, `--init_dir`,
`--invert_to`, `--S_churn` and `--solver_order 3` are errors.

    python -m tinyedm.generate --ckpt_path last.ckpt --load_ema --solver picard --window 16 --num_steps 32 \\
        --output_dir samples --num_samples 4 --image_size 32 --num_classes 10 --batch_size 4
Image-conditioned sampling: `--init_dir DIR` reads PNGs as this program writes them (`<index>.png`, taken in numeric order
of the index, normalised with `--mean/--std`), one per sample.  `--start_step K` (SDEdit / image-to-image) noises each
image to sigma_K of the table and solves from there.  `--mask_box X0 Y0 X1 Y1` (inpainting) regenerates the pixels with
X0 <= x < X1, Y0 <= y < Y1 and keeps everything outside the box, which comes out as the input image.  Both combine
with each other, with guidance, churn and `--solver dpmpp`.  `--invert_to OUT.pt` (Heun solver only) writes no images:
it runs the ODE upwards from each image to sigma_K and saves {"latents", "class_labels", "end_step", "num_steps"}, the
unit-scale latents that `solve(..., start_step=K)` turns back into the images.  Without `--init_dir` nothing changes.
`--likelihood_to OUT.json` (Heun solver only, `--network_dtype f32x3` or `f32`) writes no images either: it evaluates
log p of each image along the same upward ODE (DeterministicSolver.log_likelihood, `--num_probes K` Rademacher probes
per evaluation) and saves {"logp", "bpd", "logp_mean", "bpd_mean", "num_steps", "end_step", "num_probes", "delta", "seed",
"network_dtype"}: nats of the normalised image and bits per dimension in pixel units.  `--dequantize` first adds
U[0, 1) / 255 in pixel units, drawn from `--seed` on the host: the usual uniform dequantisation of discrete images.

    python -m tinyedm.generate --ckpt_path last.ckpt --load_ema --init_dir photos --start_step 12 \\
        --output_dir variations --num_samples 64 --image_size 32 --num_classes 10 --batch_size 64

    python -m tinyedm.generate --ckpt_path last.ckpt --load_ema --init_dir photos --mask_box 8 8 24 24 \\
        --output_dir inpainted --num_samples 64 --image_size 32 --num_classes 10 --batch_size 64

    python -m tinyedm.generate --ckpt_path last.ckpt --load_ema --init_dir photos --invert_to latents.pt \\
        --output_dir unused --num_samples 64 --image_size 32 --num_classes 10 --batch_size 64

    python -m tinyedm.generate --ckpt_path last.ckpt --load_ema --init_dir photos --likelihood_to bpd.json --dequantize \\
        --output_dir unused --num_samples 64 --image_size 32 --num_classes 10 --batch_size 64
Zero-shot restoration (DDNM, Wang et al. 2023): `--restore_scale S` (1, 2, 4, 8: SxS box down-sampling) and / or
`--restore_gray` (the mean over the channels) take the `--init_dir` images as ground truth, measure them in the process
(y = A image, the usual simulated-measurement protocol) and sample images with A x = y: 4x super-resolution,
colourisation, or both.  The solver never sees the ground truth: with `--start_step K` > 0 the state is entered from
A+ y (the blocky / grey image), not from the image.  Restored images go to `--output_dir`, A+ y to `--save_degraded DIR`,
and `--restore_report OUT.json` receives, per rank and computed in fp32 before the uint8 conversion,
{"consistency": max |A x - y|, "max_abs": max(|x|, |y|), "psnr_restored", "psnr_degraded": mean PSNR in dB against the
ground truth in pixel units, ...}.  Exclusive with `--mask_box`, `--invert_to` and `--likelihood_to`; combines with guidance, churn,
`--solver dpmpp`, `--start_step` and `--network_dtype`.

With `--dps_scale Z` the same flags -- or `--blur_std S [--blur_radius R]`, a zero-padded Gaussian blur -- name the operator
of diffusion posterior sampling (DPS, Chung et al. 2023) instead: `--measurement_noise N` adds N * N(0, 1) noise from `--seed`
to the measurement, every Heun step is followed by x += (Z / ||y - A D||) J^T A^T (y - A D) (one backward pass through the
network, so `--network_dtype bf16`, `--solver heun`, eager), `--save_degraded` receives the noisy measurement on the image
grid and `--restore_report` the RMS of A x - y (to be read against N) and the PSNRs.

    python -m tinyedm.generate --ckpt_path last.ckpt --load_ema --init_dir photos --restore_scale 4 \\
        --save_degraded lowres --restore_report sr.json --output_dir restored --num_samples 64 --image_size 32 \\
        --num_classes 10 --batch_size 64
`--labels_to FILE.json` (plain, guided, churned and multistep sampling of a class-conditional checkpoint; not with
`--init_dir`) records the labels the samples were drawn for: rank 0 writes the JSON list of the class indices of the
written `<index>.png` files, in index order, which is what `--labels_json` of `tinyedm.evaluate` and `tinyedm.classify`
reads.  `python -m tinyedm.classify --image_dir samples --labels_json FILE.json ...` then measures how often the
sampler produced the class it was asked for.  Without the flag nothing changes.
`--sigma_table schedule.json` samples on the table that `python -m tinyedm.schedule` optimised for `--num_steps` (a file
without that N is refused, naming the N it has) instead of the Karras table; it combines with `--solver heun`, `dpmpp`
and `picard`, `--S_churn` and the guidance flags, and is an error with `--solver adaptive`, which has no table.
`--quality_report FILE.json` (with `--init_dir` and a task that keeps a ground truth: `--mask_box`, `--restore_*`,
`--dps_scale`, `--start_step`) scores every output against its init image through compare.PairedQuality, per image: MSE,
PSNR and SSIM (Wang et al. 2004; 11 taps, or the largest odd window the image holds), for restoration also those of the
degraded A+ y, for `--mask_box` inside the box only.  `--quality_perceptual` adds the denoiser-feature distance with the
sampling checkpoint as its own extractor (NOT LPIPS: tinyedm_amd/compare.py).  `--restore_report` stays as it is.
Multi-GPU = replicas only: under `python -m torch.distributed.run --nproc-per-node N` every rank samples
its own contiguous index range with its own noise seed and writes `<global index>.png`; there is no collective.
"""
from __future__ import annotations

import argparse
import functools
import inspect
import json
import os

import torch

CIFAR_MEAN = (0.49139968, 0.48215841, 0.44653091)      # generate.py:31-34 ("need to do better" in the reference)
CIFAR_STD = (0.24703223, 0.24348513, 0.26158784)


def _check_solver(solver, S_churn) -> None:
    """the sampler choices that need nothing loaded: checked before any checkpoint or network is"""
    if solver not in ("heun", "dpmpp", "adaptive", "picard"):
        raise ValueError(f"generate: solver must be 'heun', 'dpmpp', 'adaptive' or 'picard', got {solver!r}")
    if solver in ("dpmpp", "adaptive", "picard") and float(S_churn) != 0.0:
        raise ValueError(f"generate: --solver {solver} is deterministic; --S_churn must be 0, got {S_churn} (stochastic "
                         "sampling is --solver heun)")


def _check_conditioning(init_dir, start_step, mask_box, invert_to, solver, S_churn, image_size, *, likelihood_to=None,
                        network_dtype="f32x3", num_probes=1, dequantize=False) -> None:
    """the image-conditioning choices that need nothing loaded"""
    if isinstance(start_step, bool) or not isinstance(start_step, int) or start_step < 0:
        raise ValueError(f"generate: --start_step must be an integer >= 0, got {start_step!r}")
    if init_dir is None:
        for flag, on in (("--mask_box", mask_box is not None), ("--start_step", start_step > 0),
                         ("--invert_to", invert_to is not None), ("--likelihood_to", likelihood_to is not None)):
            if on:
                raise ValueError(f"generate: {flag} needs --init_dir (the images to start from)")
        return
    if mask_box is not None:
        try:
            x0, y0, x1, y1 = (int(v) for v in mask_box)
            ok = len(mask_box) == 4 and all(int(v) == v for v in mask_box)
        except (TypeError, ValueError):
            ok = False
        if not (ok and 0 <= x0 < x1 <= image_size and 0 <= y0 < y1 <= image_size):
            raise ValueError(f"generate: --mask_box X0 Y0 X1 Y1 needs integers with 0 <= X0 < X1 <= {image_size} and "
                             f"0 <= Y0 < Y1 <= {image_size}, got {mask_box}")
    if invert_to is not None:
        if solver not in ("heun", "adaptive") or float(S_churn) != 0.0:
            raise ValueError("generate: --invert_to runs the deterministic Heun solver upwards: no --solver dpmpp, no "
                             "--S_churn")
        if mask_box is not None:
            raise ValueError("generate: --invert_to and --mask_box are exclusive")
    if isinstance(num_probes, bool) or not isinstance(num_probes, int) or not 1 <= num_probes <= 32:
        raise ValueError(f"generate: --num_probes must be an integer in [1, 32], got {num_probes!r}")
    if likelihood_to is None:
        for flag, on in (("--num_probes", num_probes != 1), ("--dequantize", bool(dequantize))):
            if on:
                raise ValueError(f"generate: {flag} needs --likelihood_to")
        return
    if solver != "heun" or float(S_churn) != 0.0:
        raise ValueError("generate: --likelihood_to runs the deterministic Heun solver upwards: no --solver dpmpp, no "
                         "--S_churn")
    if mask_box is not None:
        raise ValueError("generate: --likelihood_to and --mask_box are exclusive")
    if invert_to is not None:
        raise ValueError("generate: --likelihood_to and --invert_to are exclusive (one output per run)")
    if network_dtype == "bf16":
        raise ValueError("generate: --likelihood_to needs --network_dtype f32x3 or f32 (a difference quotient at bf16 "
                         "evaluation error is meaningless)")


def _check_adaptive(solver, guidance_interval, init_dir, start_step, mask_box, invert_to, likelihood_to,
                    restore_scale, restore_gray, dps_scale, rtol, atol, max_iterations, solver_report) -> None:
    """the choices of --solver adaptive that need nothing loaded"""
    import math
    if solver == "picard":          # (_check_picard has these flags)
        return
    if solver != "adaptive":
        for flag, on in (("--rtol", rtol is not None), ("--atol", atol is not None),
                         ("--max_iterations", max_iterations is not None), ("--solver_report", solver_report is not None)):
            if on:
                raise ValueError(f"generate: {flag} needs --solver adaptive" + (
                    "" if flag == "--max_iterations" else " or --solver picard"))
        return
    for flag, on in (("--guidance_interval", guidance_interval is not None), ("--mask_box", mask_box is not None),
                     ("--restore_scale / --restore_gray", restore_scale != 1 or bool(restore_gray)),
                     ("--dps_scale", dps_scale is not None), ("--likelihood_to", likelihood_to is not None),
                     ("--start_step", start_step != 0),
                     ("--init_dir without --invert_to", init_dir is not None and invert_to is None)):
        if on:
            raise ValueError(f"generate: --solver adaptive does not take {flag} (it integrates sigma_max <-> sigma_min, every "
                             "sample at its own sigma); use --solver heun")
    for flag, v in (("--rtol", rtol), ("--atol", atol)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0):
            raise ValueError(f"generate: {flag} must be a finite number >= 0, got {v!r}")
    if rtol == 0 and atol == 0:
        raise ValueError("generate: --rtol and --atol must not both be 0")
    if max_iterations is not None and (isinstance(max_iterations, bool) or not isinstance(max_iterations, int) or
                                       max_iterations < 1):
        raise ValueError(f"generate: --max_iterations must be an integer >= 1, got {max_iterations!r}")


def _check_picard(solver, guidance_interval, init_dir, start_step, mask_box, invert_to, likelihood_to, restore_scale,
                  restore_gray, dps_scale, S_churn, rtol, atol, max_iterations, window, solver_order) -> None:
    """the choices of --solver picard that need nothing loaded"""
    import math
    if solver != "picard":
        if window is not None:
            raise ValueError("generate: --window needs --solver picard")
        return
    for flag, on in (("--guidance_interval", guidance_interval is not None), ("--mask_box", mask_box is not None),
                     ("--restore_scale / --restore_gray", restore_scale != 1 or bool(restore_gray)),
                     ("--dps_scale", dps_scale is not None), ("--likelihood_to", likelihood_to is not None),
                     ("--invert_to", invert_to is not None), ("--start_step", start_step != 0),
                     ("--init_dir", init_dir is not None), ("--S_churn", float(S_churn) != 0.0),
                     ("--max_iterations", max_iterations is not None)):
        if on:
            raise ValueError(f"generate: --solver picard does not take {flag} (it iterates the plain table solve over a "
                             "window of steps); use --solver heun")
    for flag, v in (("--rtol", rtol), ("--atol", atol)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0):
            raise ValueError(f"generate: {flag} must be a finite number >= 0, got {v!r}")
    if window is not None and (isinstance(window, bool) or not isinstance(window, int) or not 1 <= window <= 64):
        raise ValueError(f"generate: --window must be an integer in 1 .. 64, got {window!r}")
    if isinstance(solver_order, bool) or solver_order not in (1, 2):
        raise ValueError(f"generate: --solver picard takes --solver_order 1 (Euler) or 2 (Heun), got {solver_order!r}")


def _check_labels_to(labels_to, init_dir) -> None:
    """the label record's choices that need nothing loaded"""
    if labels_to is not None and init_dir is not None:
        raise ValueError("generate: --labels_to records the labels of plain sampling; it does not combine with --init_dir")


def _drawn_labels(batch_size, num_workers, image_size, num_samples, num_classes, in_channels, seed, world) -> list:
    """the class indices of samples 0 .. num_samples - 1 in index order.  A sample's label is a function of the seed, its
    rank and its batch alone (RandomNoiseDataModule), so one rank replays every rank's draws on the host: no collective"""
    from .datamodules import RandomNoiseDataModule
    per_rank = (num_samples + world - 1) // world
    labels = []
    for r in range(world):
        n_r = max(0, min(per_rank, num_samples - r * per_rank))
        dm = RandomNoiseDataModule(batch_size, num_workers, image_size, n_r, num_classes, in_channels=in_channels,
                                   seed=seed + 1000003 * r, device="cpu")
        for batch in dm.predict_dataloader():
            labels.extend(int(v) for v in batch[1].flatten())
    return labels


RESTORE_SCALES = (1, 2, 4, 8)


def _check_posterior(dps_scale, blur_std, blur_radius, measurement_noise, restore_scale, restore_gray, network_dtype,
                     solver, guided) -> bool:
    """the posterior-sampling (DPS) choices that need nothing loaded; returns whether the run samples with DPS"""
    import math
    if dps_scale is None:
        for flag, on in (("--blur_std", blur_std is not None), ("--measurement_noise", float(measurement_noise) != 0.0)):
            if on:
                raise ValueError(f"generate: {flag} needs --dps_scale (posterior sampling; DDNM takes noise-free box / grey "
                                 "measurements only)")
        return False
    if not (math.isfinite(float(dps_scale)) and float(dps_scale) >= 0.0):
        raise ValueError(f"generate: --dps_scale must be finite and >= 0, got {dps_scale}")
    if not (math.isfinite(float(measurement_noise)) and float(measurement_noise) >= 0.0):
        raise ValueError(f"generate: --measurement_noise must be finite and >= 0, got {measurement_noise}")
    box = restore_scale != 1 or bool(restore_gray)
    if box == (blur_std is not None):
        raise ValueError("generate: --dps_scale needs ONE measurement operator: --restore_scale / --restore_gray or --blur_std")
    if blur_std is not None:
        from . import ops
        ops.gaussian_taps(blur_std, blur_radius)
    if network_dtype != "bf16":
        raise ValueError("generate: --dps_scale needs --network_dtype bf16 (the path with a backward pass)")
    if solver != "heun":
        raise ValueError("generate: --dps_scale needs --solver heun")
    if guided:
        raise ValueError("generate: --dps_scale with a guide is not implemented")
    return True


def _check_restoration(init_dir, restore_scale, restore_gray, save_degraded, restore_report, mask_box, invert_to,
                       likelihood_to, image_size, blur=False) -> bool:
    """the restoration choices that need nothing loaded; returns whether the run restores (blur: a --blur_std measurement
    of posterior sampling takes the place of --restore_scale / --restore_gray)"""
    if isinstance(restore_scale, bool) or not isinstance(restore_scale, int) or restore_scale not in RESTORE_SCALES:
        raise ValueError(f"generate: --restore_scale must be one of {RESTORE_SCALES}, got {restore_scale!r}")
    active = restore_scale != 1 or bool(restore_gray) or bool(blur)
    if not active:
        for flag, on in (("--save_degraded", save_degraded is not None), ("--restore_report", restore_report is not None)):
            if on:
                raise ValueError(f"generate: {flag} needs --restore_scale > 1 or --restore_gray")
        return False
    if init_dir is None:
        flag = "--restore_scale" if restore_scale != 1 else ("--restore_gray" if restore_gray else "--blur_std")
        raise ValueError(f"generate: {flag} needs --init_dir (the ground-truth images that are measured)")
    for flag, on in (("--mask_box", mask_box is not None), ("--invert_to", invert_to is not None),
                     ("--likelihood_to", likelihood_to is not None)):
        if on:
            raise ValueError(f"generate: --restore_scale / --restore_gray and {flag} are exclusive")
    if image_size % restore_scale:
        raise ValueError(f"generate: --restore_scale {restore_scale} must divide --image_size {image_size}")
    return True


def _check_quality(quality_report, quality_perceptual, init_dir, start_step, mask_box, invert_to, likelihood_to,
                   restoring, image_size) -> None:
    """--quality_report / --quality_perceptual: the choices that need nothing loaded"""
    if quality_report is None:
        if quality_perceptual:
            raise ValueError("generate: --quality_perceptual adds a column to --quality_report: give --quality_report FILE")
        return
    if init_dir is None:
        raise ValueError("generate: --quality_report needs --init_dir (the originals the outputs are scored against)")
    for flag, on in (("--invert_to", invert_to is not None), ("--likelihood_to", likelihood_to is not None)):
        if on:
            raise ValueError(f"generate: --quality_report and {flag} are exclusive: {flag} writes no images")
    if not (restoring or mask_box is not None or start_step > 0):
        raise ValueError("generate: --quality_report needs a task that keeps a ground truth: --mask_box, --restore_scale / "
                         "--restore_gray, --dps_scale or --start_step")
    if image_size < 3:
        raise ValueError(f"generate: --quality_report needs images of at least 3 x 3 pixels, got --image_size {image_size}")
    if mask_box is not None:
        from .compare import default_win_size, region_from_box
        try:
            region_from_box(mask_box, image_size, image_size, default_win_size(image_size))
        except ValueError as e:
            raise ValueError(f"generate: --quality_report scores inside --mask_box: {e}") from None


def _psnr(x, ref, mean, std) -> torch.Tensor:
    """per-image PSNR in dB of normalised fp32 images against ``ref`` in pixel units [0, 1] (the writer's
    x * std * 2 + mean, clamped): [B] fp32 on x's device"""
    m = torch.tensor([float(v) for v in mean], device=x.device).view(1, -1, 1, 1)
    sd = torch.tensor([float(v) for v in std], device=x.device).view(1, -1, 1, 1)
    a, b = ((t.float() * sd * 2.0 + m).clamp(0.0, 1.0) for t in (x, ref))
    return -10.0 * torch.log10(((a - b) ** 2).mean(dim=(1, 2, 3)).clamp_min(1e-12))


def load_images(init_dir, mean, std, image_size, channels) -> torch.Tensor:
    """the PNGs of a directory as PreditionWriter names them (<index>.png), in numeric order of the index, normalised
    as PreditionWriter denormalises (pixel = x * std * 2 + mean): fp32 [n, C, H, W] on the host"""
    from .neighbors import read_png_dir
    m = torch.tensor([float(v) for v in mean], dtype=torch.float32).view(-1, 1, 1)
    sd = torch.tensor([float(v) for v in std], dtype=torch.float32).view(-1, 1, 1)
    # the inverse of PreditionWriter's clamp(x * std * 2 + mean, 0, 1) * 255, truncated: level u is the bin
    # [u, u + 1) / 255, read at its centre, so an image written and read back is written as the same levels
    return torch.stack([((torch.from_numpy(a.copy()).permute(2, 0, 1).float() + 0.5) / 255.0 - m) / (2.0 * sd)
                        for a in read_png_dir(init_dir, "generate", "--init_dir", image_size, channels)])


def _validate(*, solver, S_churn, init_dir, start_step, num_steps, mask_box, invert_to, likelihood_to, network_dtype,
              num_probes, dequantize, image_size, dps_scale, blur_std, blur_radius, measurement_noise, restore_scale,
              restore_gray, save_degraded, restore_report, labels_to, guided, guidance_interval=None, rtol=None, atol=None,
              max_iterations=None, solver_report=None, window=None, solver_order=2, sigma_table=None, quality_report=None,
              quality_perceptual=False) -> tuple:
    """every choice that needs nothing loaded, checked once and in one order for generate() and the command line; returns
    (posterior, restoring): whether the run samples with DPS, and whether it restores (DDNM or DPS)"""
    _check_solver(solver, S_churn)
    if sigma_table is not None and solver == "adaptive":
        raise ValueError("generate: --solver adaptive does not take --sigma_table (it integrates sigma_max <-> sigma_min, "
                         "every sample at its own sigma); use --solver heun")
    _check_adaptive(solver, guidance_interval, init_dir, start_step, mask_box, invert_to, likelihood_to,
                    restore_scale, restore_gray, dps_scale, rtol, atol, max_iterations, solver_report)
    _check_picard(solver, guidance_interval, init_dir, start_step, mask_box, invert_to, likelihood_to, restore_scale,
                  restore_gray, dps_scale, S_churn, rtol, atol, max_iterations, window, solver_order)
    _check_conditioning(init_dir, start_step, mask_box, invert_to, solver, S_churn, image_size,
                        likelihood_to=likelihood_to, network_dtype=network_dtype, num_probes=num_probes,
                        dequantize=dequantize)
    posterior = _check_posterior(dps_scale, blur_std, blur_radius, measurement_noise, restore_scale, restore_gray,
                                 network_dtype, solver, guided)
    restoring = _check_restoration(init_dir, restore_scale, restore_gray, save_degraded, restore_report, mask_box,
                                   invert_to, likelihood_to, image_size, blur=posterior and blur_std is not None)
    _check_labels_to(labels_to, init_dir)
    if start_step >= num_steps:
        raise ValueError(f"generate: --start_step must be below --num_steps = {num_steps}, got {start_step}")
    _check_quality(quality_report, quality_perceptual, init_dir, start_step, mask_box, invert_to, likelihood_to, restoring,
                   image_size)
    return posterior, restoring


def _rank_path(path, rank, world) -> str:
    """the per-rank name of an output file: root.rankN.ext when there is more than one rank"""
    root, ext = os.path.splitext(path)
    return f"{root}.rank{rank}{ext}" if world > 1 else path


def _write_json(path, obj) -> None:
    with open(path, "w") as f:
        json.dump(obj, f)


class _Collect:
    """--quality_report: keeps what a task hands to its image writers (fp32, on the device), by name"""

    def __init__(self):
        self.kept = {}

    def add(self, name, x) -> None:
        self.kept.setdefault(name, []).append(x.detach().float().clone())

    def write_on_batch_end(self, trainer, pl_module, prediction, batch_indices, batch, batch_idx, dataloader_idx) -> None:
        self.add("output", prediction)          # (a Trainer.predict callback, beside the PreditionWriter)

    def get(self, name):
        return torch.cat(self.kept[name]) if name in self.kept else None


def _write_quality(path, collect, references, model, perceptual, mean, std, mask_box, image_size, first, seed,
                   network_dtype, where) -> None:
    """--quality_report: every kept set against the init images through compare.PairedQuality"""
    from .compare import PairedQuality, default_win_size, region_from_box, report_rows
    win = default_win_size(image_size)
    region = None if mask_box is None else region_from_box(mask_box, image_size, image_size, win)
    dtype = network_dtype if network_dtype in ("f32x3", "f32") else "f32x3"     # (the taps have no bf16 form)
    pq = PairedQuality(model if perceptual else None, win_size=win, mean=mean, std=std, seed=seed, network_dtype=dtype)
    settings = {"data_range": 1.0, "window": pq.window_name, "win_size": win, "win_sigma": pq.win_sigma,
                "region_box": None if mask_box is None else [int(v) for v in mask_box], "perceptual": bool(perceptual),
                "first_index": first, "num_images": 0}
    if perceptual:
        settings.update(sigma=pq.extractor.sigma, taps=list(pq.extractor.taps), seed=seed, network_dtype=dtype)
    report = {"settings": settings}
    for name, key in (("output", "restored"), ("degraded", "degraded")):
        x = collect.get(name)
        if x is None:
            continue
        ref = references[:x.shape[0]].to(x.device)
        indices = list(range(first, first + x.shape[0]))
        scores = pq.score(x, ref, region=region, ids=indices)
        settings["num_images"] = x.shape[0]
        report[key] = {"summary": scores["summary"], "images": report_rows(scores, indices)}
    with open(path, "w") as f:
        json.dump(report, f, indent=1)
    print(f"[rank {where[0]}] wrote the paired quality of images {where[1]} to {path}", flush=True)


def _run_invert(model, datamodule, invert_to, graph, end_step, num_steps, where) -> None:
    """--invert_to.  The labels of each batch are the ones a solve of the same --seed draws: the latents close the loop"""
    model.eval()
    lat, lab = [], []
    for x0, y, img in datamodule.predict_dataloader():
        y = y if model.conditional else None
        lat.append(model.solver.invert(model, img, y, graph=graph, end_step=end_step).cpu())
        lab.append(None if y is None else y.cpu())
    torch.save({"latents": torch.cat(lat) if lat else torch.empty(0), "end_step": end_step, "num_steps": num_steps,
                "class_labels": None if not lab or lab[0] is None else torch.cat(lab)}, invert_to)
    print(f"[rank {where[0]}] wrote the latents of images {where[1]} to {invert_to}", flush=True)


def _run_likelihood(model, datamodule, likelihood_to, graph, end_step, num_probes, dequantize, rank_seed, std, dims, where,
                    report) -> None:
    """--likelihood_to: log p and bits/dim of the images, followed in the JSON by ``report``"""
    from .solvers import bits_per_dim
    model.eval()
    sd2 = [2.0 * float(v) for v in std]         # load_images normalises with x = (pixel - mean) / (2 std)
    gen = torch.Generator().manual_seed(rank_seed)
    logp = []
    for x0, y, img in datamodule.predict_dataloader():
        y = y if model.conditional else None
        if dequantize:      # level u read at its centre (load_images) -> uniform over its bin [u, u + 1) / 255
            u = torch.rand(img.shape, generator=gen, dtype=torch.float32) - 0.5
            img = img + (u / 255.0 / torch.tensor(sd2, dtype=torch.float32).view(-1, 1, 1)).to(img.device)
        logp.append(model.solver.log_likelihood(model, img, y, graph=graph, end_step=end_step,
                                                num_probes=num_probes).cpu())
    logp = torch.cat(logp) if logp else torch.empty(0, dtype=torch.float64)
    bpd = bits_per_dim(logp, dims, sd2)
    _write_json(likelihood_to, {"logp": logp.tolist(), "bpd": bpd.tolist(),
                                "logp_mean": float(logp.mean()) if logp.numel() else None,
                                "bpd_mean": float(bpd.mean()) if bpd.numel() else None, **report})
    print(f"[rank {where[0]}] wrote the likelihoods of images {where[1]} to {likelihood_to}", flush=True)


def _max_residual():
    """DDNM's residual statistic as (add, fields): max |A x - y| and the magnitude it is to be read against"""
    s = {"consistency": 0.0, "max_abs": 0.0}

    def add(res, out, meas):
        s["consistency"] = max(s["consistency"], float(res.abs().max()))
        s["max_abs"] = max(s["max_abs"], float(out.abs().max()), float(meas.abs().max()))
    return add, lambda: s


def _rms_residual(measurement_noise, dps_scale):
    """DPS's residual statistic as (add, fields): the RMS of A x - y, and the noise level it is to be read against"""
    s = [0.0, 0]

    def add(res, out, meas):
        s[:] = s[0] + float((res.double() ** 2).sum()), s[1] + res.numel()
    return add, lambda: {"measurement_rms": (s[0] / s[1]) ** 0.5 if s[1] else None, "measurement_noise": measurement_noise,
                         "dps_scale": dps_scale}


def _run_restore(model, datamodule, op, solve_kw, noise, rank_seed, back, stat, start_step, writers, mean, std, where,
                 what, output_dir, restore_report, report, collect=None) -> None:
    """restoration by DDNM or DPS: measure each ground-truth image with ``op`` (plus noise * N(0, 1) from rank_seed), solve
    with ``solve_kw`` from ``back(meas)``, the measurement on the image grid, and write both through ``writers``.
    ``stat`` = (add, fields) accumulates the residual A x - y; the JSON is fields(), the PSNRs, then ``report``"""
    add, fields = stat
    model.eval()
    gen = torch.Generator().manual_seed(rank_seed)
    psnr_out, psnr_deg = [], []
    for bi, (x0, y, img) in enumerate(datamodule.predict_dataloader()):
        y = y if model.conditional else None
        meas = op.measure(img)              # the ground truth is used for this and for the report only
        if noise > 0.0:
            meas = meas + noise * torch.randn(meas.shape, generator=gen).to(meas.device)
        deg = back(meas)
        out = model.solver.solve(model, x0, y, image=deg if start_step > 0 else None, measurement=meas, **solve_kw).float()
        add(op.measure(out) - meas, out, meas)
        psnr_out.append(_psnr(out, img, mean, std).cpu())
        psnr_deg.append(_psnr(deg, img, mean, std).cpu())
        for w, pred in zip(writers, (out, deg)):
            w.write_on_batch_end(None, model, pred, None, None, bi, 0)
        if collect is not None:
            collect.add("output", out)
            collect.add("degraded", deg)
    if restore_report is not None:
        _write_json(restore_report, {**fields(), "psnr_restored": float(torch.cat(psnr_out).mean()) if psnr_out else None,
                                     "psnr_degraded": float(torch.cat(psnr_deg).mean()) if psnr_deg else None, **report})
    print(f"[rank {where[0]}] wrote the {what} {where[1]} to {output_dir}", flush=True)


def _picard_report(stats, solver, first) -> dict:
    """--solver_report of --solver picard: the ParallelStats of every solve, in batch order, and the totals"""
    per_sample = [int(v) for s in stats for v in s.per_sample_iterations]
    return {"per_sample_iterations": per_sample, "iterations": [s.iterations for s in stats],
            "evaluations": sum(s.evaluations for s in stats), "guide_evaluations": sum(s.guide_evaluations for s in stats),
            "rows": sum(s.rows for s in stats), "sequential_evaluations": sum(s.sequential_evaluations for s in stats),
            "window": solver.window, "order": solver.order, "rtol": solver.rtol, "atol": solver.atol, "first_index": first,
            "num_images": len(per_sample)}


def _solver_report(stats, solver, first) -> dict:
    """--solver_report: per image the accepted and rejected steps of the adaptive solver, per batch its iterations, and
    the totals (``stats``: the AdaptiveStats of every solve, in batch order)"""
    accepted = [int(v) for s in stats for v in s.accepted]
    rejected = [int(v) for s in stats for v in s.rejected]
    steps = sum(accepted) + sum(rejected)
    return {"accepted": accepted, "rejected": rejected, "iterations": [s.iterations for s in stats],
            "accepted_total": sum(accepted), "rejected_total": sum(rejected),
            "rejected_share": sum(rejected) / steps if steps else None,
            "evaluations": sum(s.evaluations for s in stats), "guide_evaluations": sum(s.guide_evaluations for s in stats),
            "rtol": solver.rtol, "atol": solver.atol, "max_iterations": solver.max_iterations, "first_index": first,
            "num_images": len(accepted)}


def _run_sample(model, datamodule, writer, n_local, where, output_dir, labels_to, labels, num_samples, collect=None) -> None:
    """plain sampling through Trainer.predict; ``labels()`` (unless None) gives what --labels_to records"""
    from .trainer import Trainer
    trainer = Trainer(accelerator="gpu", strategy="auto", callbacks=[writer] + ([] if collect is None else [collect]))
    if n_local > 0:
        trainer.predict(model, datamodule=datamodule, return_predictions=False, ckpt_path=None, distributed=False)   # generate.py:45-47
    print(f"[rank {where[0]}] wrote images {where[1]} to {output_dir}", flush=True)
    if labels is not None:
        _write_json(labels_to, labels())
        print(f"[rank 0] wrote the labels of images 0..{num_samples - 1} to {labels_to}", flush=True)


def generate(ckpt_path, load_ema, output_dir, num_samples, image_size, num_classes, batch_size, num_workers=16,
             num_steps=32, *, in_channels=None, mean=None, std=None, seed=0, graph=True, model=None,
             network_dtype="f32x3", guide=None, guide_ckpt_path=None, guide_load_ema=False, guidance=1.0,
             guidance_interval=None, S_churn=0.0, S_min=0.0, S_max=float("inf"), S_noise=1.0, solver="heun",
             solver_order=2, init_dir=None, start_step=0, mask_box=None, invert_to=None, likelihood_to=None,
             num_probes=1, dequantize=False, restore_scale=1, restore_gray=False, save_degraded=None,
             restore_report=None, labels_to=None, dps_scale=None, blur_std=None, blur_radius=2,
             measurement_noise=0.0, rtol=None, atol=None, max_iterations=None, solver_report=None, window=None,
             sigma_table=None, quality_report=None, quality_perceptual=False) -> None:
    from . import _runtime_env
    from .callbacks import PreditionWriter
    from .datamodules import RandomNoiseDataModule
    from .edm import EDM
    from .solvers import (AdaptiveSolver, DeterministicSolver, GaussianBlur, LinearDegradation, MultistepSolver,
                          ParallelSolver, StochasticSolver)

    posterior, restoring = _validate(
        solver=solver, S_churn=S_churn, init_dir=init_dir, start_step=start_step, num_steps=num_steps, mask_box=mask_box,
        invert_to=invert_to, likelihood_to=likelihood_to, network_dtype=network_dtype, num_probes=num_probes,
        dequantize=dequantize, image_size=image_size, dps_scale=dps_scale, blur_std=blur_std, blur_radius=blur_radius,
        measurement_noise=measurement_noise, restore_scale=restore_scale, restore_gray=restore_gray,
        save_degraded=save_degraded, restore_report=restore_report, labels_to=labels_to,
        guided=guide is not None or guide_ckpt_path is not None, guidance_interval=guidance_interval, rtol=rtol, atol=atol,
        max_iterations=max_iterations, solver_report=solver_report, window=window, solver_order=solver_order,
        sigma_table=sigma_table, quality_report=quality_report, quality_perceptual=quality_perceptual)
    if sigma_table is not None:     # (before anything is loaded: a file without this N is refused, naming the N it has)
        from .schedule import Schedule
        sigma_table = Schedule.load(sigma_table, num_steps).sigmas
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dev = torch.device("cuda", torch.cuda.current_device())
    if model is None:
        model = EDM.load_from_checkpoint(ckpt_path, load_ema=load_ema)
    if labels_to is not None and not model.conditional:
        raise ValueError("generate: --labels_to needs a class-conditional checkpoint: this one draws no labels")
    model = model.to(dev)
    model.denoiser.set_eval_dtype(network_dtype)
    if guide_ckpt_path is not None:
        if guide is not None:
            raise ValueError("generate: pass guide or guide_ckpt_path, not both")
        guide = EDM.load_from_checkpoint(guide_ckpt_path, load_ema=guide_load_ema)
    if guide == "unconditional":
        if float(getattr(model.embedding, "label_dropout", 0.0)) == 0.0:
            print(f"[rank {rank}] warning: the model was trained with label_dropout 0: it never saw label-free samples, "
                  "its unconditional evaluation is untrained", flush=True)
    elif guide is not None:
        guide = guide.to(dev).eval()
        guide.denoiser.set_eval_dtype(network_dtype)
        if float(guidance) == 1.0:
            print(f"[rank {rank}] guidance 1.0: the guide network is unused", flush=True)
    rank_seed = seed + 1000003 * rank
    common = dict(num_steps=num_steps, guide=guide, guidance=guidance, guidance_interval=guidance_interval, seed=rank_seed)
    if sigma_table is not None:
        common["sigmas"] = sigma_table
    adaptive_stats = []
    if solver == "adaptive":
        tol = {k: v for k, v in (("rtol", rtol), ("atol", atol), ("max_iterations", max_iterations)) if v is not None}
        model.solver = AdaptiveSolver(**common, **tol)
        graph = False               # the adaptive loop is eager: the host reads the active count every iteration
        for name in ("solve", "invert"):    # every solve's statistics, in batch order, for --solver_report
            def recorded(*a, _run=getattr(model.solver, name), **kw):
                out = _run(*a, **kw)
                adaptive_stats.append(model.solver.last_stats)
                return out
            setattr(model.solver, name, recorded)
    elif solver == "picard":
        tol = {k: v for k, v in (("rtol", rtol), ("atol", atol), ("window", window)) if v is not None}
        model.solver = ParallelSolver(**common, order=solver_order, **tol)

        def recorded(*a, _run=model.solver.solve, **kw):        # every solve's statistics, for --solver_report
            out = _run(*a, **kw)
            adaptive_stats.append(model.solver.last_stats)
            return out
        model.solver.solve = recorded
    elif solver == "dpmpp":
        model.solver = MultistepSolver(order=solver_order, **common)
    elif float(S_churn) != 0.0:     # (a negative or non-finite S_churn reaches the solver's validation)
        model.solver = StochasticSolver(S_churn=S_churn, S_min=S_min, S_max=S_max, S_noise=S_noise, **common)
    else:
        model.solver = DeterministicSolver(**common)
    # the eager loop (same values) where a replay is not safe, and for DPS, whose step runs a backward pass
    graph = bool(graph and not posterior and _runtime_env.GRAPH_REPLAY_SAFE)
    if graph or init_dir is not None:
        solve = model.solver.solve
        extra = {} if init_dir is None else {"start_step": start_step}
        model.solver.solve = lambda m, x0, labels=None, **kw: solve(m, x0, labels, graph=graph, **extra, **kw)
    C = int(in_channels) if in_channels is not None else int(model.denoiser.in_channels)
    per_rank = (num_samples + world - 1) // world
    first = rank * per_rank
    n_local = max(0, min(per_rank, num_samples - first))
    if mean is None or std is None:
        mean, std = (CIFAR_MEAN, CIFAR_STD) if C == 3 else ((0.5,) * C, (0.25,) * C)
    images = mask = None
    if init_dir is not None:
        images = load_images(init_dir, mean, std, image_size, C)
        if images.shape[0] < num_samples:
            raise ValueError(f"generate: --init_dir holds {images.shape[0]} images, --num_samples asks for {num_samples}")
        images = images[first:first + n_local]
        if mask_box is not None:
            x0_, y0_, x1_, y1_ = (int(v) for v in mask_box)
            mask = torch.ones(image_size, image_size, dtype=torch.uint8)      # non-zero = known pixel, kept
            mask[y0_:y1_, x0_:x1_] = 0
    datamodule = RandomNoiseDataModule(batch_size, num_workers, image_size, n_local, num_classes, in_channels=C,
                                       seed=rank_seed, images=images, mask=mask)
    where = (rank, f"{first}..{first + n_local - 1}")       # for the line each task prints at its end
    writer = functools.partial(PreditionWriter, write_interval="batch", mean=mean, std=std, first_index=first)
    collect = None if quality_report is None else _Collect()
    if invert_to is not None:
        _run_invert(model, datamodule, _rank_path(invert_to, rank, world), graph, start_step, num_steps, where)
    elif likelihood_to is not None:
        _run_likelihood(model, datamodule, _rank_path(likelihood_to, rank, world), graph, start_step, num_probes,
                        dequantize, rank_seed, std, C * image_size * image_size, where,
                        {"num_steps": num_steps, "end_step": start_step, "num_probes": num_probes,
                         "delta": float(model.solver.delta), "seed": seed, "network_dtype": network_dtype,
                         "dequantize": bool(dequantize), "first_index": first})
    elif restoring:
        blur = blur_std is not None
        op = GaussianBlur(float(blur_std), int(blur_radius)) if blur else LinearDegradation(restore_scale, bool(restore_gray))
        if posterior:
            what, solve_kw = "posterior samples", {"operator": op, "dps_scale": float(dps_scale)}
            stat = _rms_residual(float(measurement_noise), float(dps_scale))
            blur_fields = {"blur_std": float(blur_std) if blur else None, "blur_radius": int(blur_radius) if blur else None}
        else:
            what, solve_kw, stat, blur_fields = "restored images", {"degradation": op}, _max_residual(), {}
        # back, what --save_degraded shows: the measurement on the image grid (a blur's y is an image already)
        _run_restore(model, datamodule, op, solve_kw, float(measurement_noise), rank_seed,
                     (lambda meas: meas) if blur else (lambda meas: op.pinv(meas, C)), stat, start_step,
                     [writer(d) for d in (output_dir, save_degraded) if d is not None], mean, std, where, what, output_dir,
                     None if restore_report is None else _rank_path(restore_report, rank, world),
                     {"restore_scale": restore_scale, "restore_gray": bool(restore_gray), **blur_fields, "num_steps": num_steps,
                      "start_step": start_step, "seed": seed, "network_dtype": network_dtype, "first_index": first,
                      "num_images": n_local}, collect)
    else:
        labels = None if labels_to is None or rank != 0 else functools.partial(
            _drawn_labels, batch_size, num_workers, image_size, num_samples, num_classes, C, seed, world)
        _run_sample(model, datamodule, writer(output_dir), n_local, where, output_dir, labels_to, labels, num_samples,
                    collect)
    if collect is not None and n_local > 0:
        _write_quality(_rank_path(quality_report, rank, world), collect, images, model, quality_perceptual, mean, std,
                       mask_box, image_size, first, seed, network_dtype, where)
    if solver_report is not None:
        report = _picard_report if solver == "picard" else _solver_report
        _write_json(_rank_path(solver_report, rank, world), report(adaptive_stats, model.solver, first))
        print(f"[rank {rank}] wrote the step counts of images {where[1]} to {_rank_path(solver_report, rank, world)}",
              flush=True)


def main(argv=None):
    parser = argparse.ArgumentParser(description="Run the model generation")
    parser.add_argument("--ckpt_path", type=str, default=None, help="Path to the checkpoint file")
    parser.add_argument("--load_ema", action="store_true", help="Load the exponential moving average of the weights")
    parser.add_argument("--output_dir", type=str, required=True, help="Directory for output")
    parser.add_argument("--num_samples", type=int, required=True, help="Number of samples to generate")
    parser.add_argument("--image_size", type=int, required=True, help="Image size")
    parser.add_argument("--num_classes", type=int, required=True, help="Number of classes")
    parser.add_argument("--batch_size", type=int, required=True, help="Batch size")
    parser.add_argument("--num_workers", type=int, default=16, help="Number of workers (default: 16)")
    parser.add_argument("--num_steps", type=int, default=32, help="Number of steps (default: 32)")
    # extensions
    parser.add_argument("--in_channels", type=int, default=None)
    parser.add_argument("--mean", type=float, nargs="+", default=None)
    parser.add_argument("--std", type=float, nargs="+", default=None)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--no_graph", action="store_true", help="eager Heun loop instead of the captured hipGraph")
    parser.add_argument("--network_dtype", choices=["bf16", "f32", "f32x3"], default="f32x3",
                        help="denoiser evaluation precision: f32x3 (default) = fp32-accurate (split-bf16, 3 MFMA passes), "
                             "f32 = exact fp32 products (checker, slower), bf16 = fast mode")
    parser.add_argument("--config_name", type=str, default=None,
                        help="sample from random-init weights of experiments/conf/<name>.yaml (no checkpoint)")
    parser.add_argument("--config_path", type=str, default=None)
    # guided sampling
    parser.add_argument("--guide_ckpt_path", type=str, default=None, help="checkpoint of the guide network")
    parser.add_argument("--guide_load_ema", action="store_true", help="load the EMA weights of the guide")
    parser.add_argument("--guide_config_name", type=str, default=None,
                        help="random-init guide from experiments/conf/<name>.yaml (no checkpoint)")
    parser.add_argument("--guide_unconditional", action="store_true",
                        help="classifier-free guidance from the model alone: its label-free evaluation is the guide")
    parser.add_argument("--guidance", type=float, default=1.0,
                        help="guidance weight w: D = D_guide + w*(D_main - D_guide) (default 1.0 = unguided)")
    parser.add_argument("--guidance_interval", type=float, nargs=2, metavar=("LO", "HI"), default=None,
                        help="guide only the evaluations with LO < sigma <= HI")
    # stochastic sampling (EDM's churn)
    parser.add_argument("--S_churn", type=float, default=0.0,
                        help="stochasticity strength: gamma_i = min(S_churn / num_steps, sqrt(2) - 1) (default 0 = "
                             "deterministic sampling)")
    parser.add_argument("--S_min", type=float, default=0.0, help="churn only steps with S_min <= t_i (default 0)")
    parser.add_argument("--S_max", type=float, default=float("inf"), help="churn only steps with t_i <= S_max (default inf)")
    parser.add_argument("--S_noise", type=float, default=1.0, help="scale of the churn noise (default 1)")
    # multistep sampling
    parser.add_argument("--solver", choices=["heun", "dpmpp", "adaptive", "picard"], default="heun",
                        help="heun (default): EDM's 2nd-order Heun, 2N-1 network evaluations; dpmpp: DPM-Solver++ "
                             "multistep, N evaluations; adaptive: Heun/Euler pair with per-sample step control to "
                             "--rtol / --atol; picard: the Heun (or Euler) table solve iterated in parallel over a "
                             "--window of steps until it moves by less than --rtol / --atol")
    parser.add_argument("--solver_order", type=int, choices=[1, 2, 3], default=2,
                        help="order of --solver dpmpp (default 2: DPM-Solver++(2M)); --solver picard: 2 (Heun, default) "
                             "or 1 (Euler)")
    parser.add_argument("--window", type=int, default=None, metavar="P",
                        help="--solver picard: the table steps iterated at once, 1 .. 64 (default 16); the network "
                             "batch is P times --batch_size")
    # adaptive sampling
    parser.add_argument("--rtol", type=float, default=None, help="--solver adaptive / picard: relative tolerance (default 1e-3)")
    parser.add_argument("--atol", type=float, default=None, help="--solver adaptive / picard: absolute tolerance (default 1e-4)")
    parser.add_argument("--max_iterations", type=int, default=None,
                        help="--solver adaptive: controlled steps before the solve gives up (default 1024)")
    parser.add_argument("--solver_report", type=str, default=None, metavar="FILE.json",
                        help="--solver adaptive: write the accepted and rejected steps of every image and the totals; "
                             "--solver picard: the iterations, evaluations and network rows")
    # image-conditioned sampling
    parser.add_argument("--init_dir", type=str, default=None,
                        help="directory of <index>.png images to start from (as this program writes them)")
    parser.add_argument("--start_step", type=int, default=0,
                        help="enter the sigma table at step K: the images are noised to sigma_K (default 0)")
    parser.add_argument("--mask_box", type=int, nargs=4, metavar=("X0", "Y0", "X1", "Y1"), default=None,
                        help="inpainting: regenerate the box X0 <= x < X1, Y0 <= y < Y1, keep everything outside it")
    parser.add_argument("--invert_to", type=str, default=None, metavar="OUT.pt",
                        help="write the latents of the --init_dir images (the ODE run upwards to --start_step) instead "
                             "of sampling; Heun solver only")
    parser.add_argument("--likelihood_to", type=str, default=None, metavar="OUT.json",
                        help="write log p (nats) and bits/dim of the --init_dir images, evaluated along the ODE run "
                             "upwards to --start_step, instead of sampling; Heun solver, --network_dtype f32x3 or f32")
    parser.add_argument("--num_probes", type=int, default=1,
                        help="Rademacher probes per evaluation of --likelihood_to (default 1; the batch grows to 1 + 2K)")
    parser.add_argument("--dequantize", action="store_true",
                        help="--likelihood_to: add uniform noise of one grey level to the images first")
    # zero-shot restoration
    parser.add_argument("--restore_scale", type=int, default=1, metavar="S",
                        help="restoration: sample images whose SxS block means equal those of the --init_dir images "
                             "(1, 2, 4 or 8; default 1 = off)")
    parser.add_argument("--restore_gray", action="store_true",
                        help="restoration: ... whose mean over the channels equals that of the --init_dir images "
                             "(colourisation; combines with --restore_scale)")
    parser.add_argument("--save_degraded", type=str, default=None, metavar="DIR",
                        help="restoration: write A+ y, the measurement replicated to the image grid, as <index>.png")
    parser.add_argument("--restore_report", type=str, default=None, metavar="OUT.json",
                        help="restoration: write max |A x - y| and the mean PSNR of the restored images and of A+ y")
    # posterior sampling (DPS)
    parser.add_argument("--dps_scale", type=float, default=None, metavar="Z",
                        help="diffusion posterior sampling: after every step x += (Z / ||y - A D||) J^T A^T (y - A D); the "
                             "operator A is --restore_scale / --restore_gray or --blur_std; needs --network_dtype bf16")
    parser.add_argument("--blur_std", type=float, default=None, metavar="S",
                        help="--dps_scale: A is a zero-padded Gaussian blur of standard deviation S pixels")
    parser.add_argument("--blur_radius", type=int, default=2, metavar="R",
                        help="--blur_std: 2R+1 taps, R in 1..4 (default 2)")
    parser.add_argument("--measurement_noise", type=float, default=0.0, metavar="N",
                        help="--dps_scale: add N * N(0, 1) noise (from --seed) to the measurement (default 0)")
    parser.add_argument("--labels_to", type=str, default=None, metavar="FILE.json",
                        help="write the class indices the samples were drawn for, in index order (the format "
                             "--labels_json of tinyedm.classify reads); class-conditional checkpoints, not with --init_dir")
    parser.add_argument("--sigma_table", type=str, default=None, metavar="schedule.json",
                        help="sample on the table of this file for --num_steps (python -m tinyedm.schedule writes it) "
                             "instead of the Karras table; --solver heun, dpmpp or picard")
    parser.add_argument("--quality_report", type=str, default=None, metavar="FILE.json",
                        help="with --init_dir and --mask_box, --restore_*, --dps_scale or --start_step: write per image the "
                             "MSE, PSNR and SSIM of every output (restoration: also of A+ y) against its init image; "
                             "--mask_box: inside the box")
    parser.add_argument("--quality_perceptual", action="store_true",
                        help="--quality_report: add the denoiser-feature distance, the sampling checkpoint as its extractor")
    args = parser.parse_args(argv)
    _check_solver(args.solver, args.S_churn)        # a ValueError, not a usage error: raised before _validate meets it
    try:
        # every option of _validate is a flag of the same name, but for the guide, which has three
        _validate(guided=args.guide_ckpt_path is not None or args.guide_config_name is not None or args.guide_unconditional,
                  **{k: getattr(args, k) for k in inspect.signature(_validate).parameters if k != "guided"})
    except ValueError as e:
        parser.error(str(e))
    if args.guide_ckpt_path is not None and args.guide_config_name is not None:
        parser.error("--guide_ckpt_path and --guide_config_name are exclusive")
    if args.guide_unconditional and (args.guide_ckpt_path is not None or args.guide_config_name is not None):
        parser.error("--guide_unconditional evaluates the model itself as the guide: no --guide_ckpt_path or "
                     "--guide_config_name")
    from . import networks
    from .config import compose, instantiate
    conf_dir = args.config_path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                "experiments", "conf")

    def random_init(name):
        cfg = compose(name, conf_dir)
        networks.manual_seed(cfg.seed)
        torch.manual_seed(cfg.seed)
        return instantiate(cfg.model)
    # the guide first: the main network's seeding is then the last, as without a guide
    guide = None if args.guide_config_name is None else random_init(args.guide_config_name)
    if args.guide_unconditional:
        guide = "unconditional"
    model = None
    if args.ckpt_path is None:
        if args.config_name is None:
            parser.error("--ckpt_path is required (or --config_name for a random-init plumbing run)")
        model = random_init(args.config_name)
    generate(args.ckpt_path, args.load_ema, args.output_dir, args.num_samples, args.image_size, args.num_classes,
             args.batch_size, args.num_workers, args.num_steps, in_channels=args.in_channels, mean=args.mean,
             std=args.std, seed=args.seed, graph=not args.no_graph, model=model, network_dtype=args.network_dtype,
             guide=guide, guide_ckpt_path=args.guide_ckpt_path, guide_load_ema=args.guide_load_ema,
             guidance=args.guidance, guidance_interval=args.guidance_interval, S_churn=args.S_churn, S_min=args.S_min,
             S_max=args.S_max, S_noise=args.S_noise, solver=args.solver, solver_order=args.solver_order,
             init_dir=args.init_dir, start_step=args.start_step, mask_box=args.mask_box, invert_to=args.invert_to,
             likelihood_to=args.likelihood_to, num_probes=args.num_probes, dequantize=args.dequantize,
             restore_scale=args.restore_scale, restore_gray=args.restore_gray, save_degraded=args.save_degraded,
             restore_report=args.restore_report, labels_to=args.labels_to, dps_scale=args.dps_scale,
             blur_std=args.blur_std, blur_radius=args.blur_radius, measurement_noise=args.measurement_noise,
             rtol=args.rtol, atol=args.atol, max_iterations=args.max_iterations, solver_report=args.solver_report,
             window=args.window, sigma_table=args.sigma_table, quality_report=args.quality_report,
             quality_perceptual=args.quality_perceptual)


if __name__ == "__main__":
    main()
