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

    python -m tinyedm.generate --ckpt_path last.ckpt --load_ema --solver dpmpp --solver_order 2 --num_steps 32 \\
        --output_dir samples --num_samples 50000 --image_size 32 --num_classes 10 --batch_size 512
Multi-GPU = replicas only: under `python -m torch.distributed.run --nproc-per-node N` every rank samples
its own contiguous index range with its own noise seed and writes `<global index>.png`; there is no collective.
"""
from __future__ import annotations

import argparse
import os

import torch

CIFAR_MEAN = (0.49139968, 0.48215841, 0.44653091)      # generate.py:31-34 ("need to do better" in the reference)
CIFAR_STD = (0.24703223, 0.24348513, 0.26158784)


def _check_solver(solver, S_churn) -> None:
    """the sampler choices that need nothing loaded: checked before any checkpoint or network is"""
    if solver not in ("heun", "dpmpp"):
        raise ValueError(f"generate: solver must be 'heun' or 'dpmpp', got {solver!r}")
    if solver == "dpmpp" and float(S_churn) != 0.0:
        raise ValueError(f"generate: --solver dpmpp is deterministic; --S_churn must be 0, got {S_churn} (stochastic "
                         "sampling is --solver heun)")


def generate(ckpt_path, load_ema, output_dir, num_samples, image_size, num_classes, batch_size, num_workers=16,
             num_steps=32, *, in_channels=None, mean=None, std=None, seed=0, graph=True, model=None,
             network_dtype="f32x3", guide=None, guide_ckpt_path=None, guide_load_ema=False, guidance=1.0,
             guidance_interval=None, S_churn=0.0, S_min=0.0, S_max=float("inf"), S_noise=1.0, solver="heun",
             solver_order=2) -> None:
    from .callbacks import PreditionWriter
    from .datamodules import RandomNoiseDataModule
    from .edm import EDM
    from .solvers import DeterministicSolver, MultistepSolver, StochasticSolver
    from .trainer import Trainer

    _check_solver(solver, S_churn)

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    dev = torch.device("cuda", torch.cuda.current_device())
    if model is None:
        model = EDM.load_from_checkpoint(ckpt_path, load_ema=load_ema)
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
    if solver == "dpmpp":
        model.solver = MultistepSolver(num_steps=num_steps, order=solver_order, guide=guide, guidance=guidance,
                                       guidance_interval=guidance_interval)
    elif float(S_churn) != 0.0:     # (a negative or non-finite S_churn reaches the solver's validation)
        model.solver = StochasticSolver(num_steps=num_steps, guide=guide, guidance=guidance,
                                        guidance_interval=guidance_interval, S_churn=S_churn, S_min=S_min,
                                        S_max=S_max, S_noise=S_noise, seed=seed + 1000003 * rank)
    else:
        model.solver = DeterministicSolver(num_steps=num_steps, guide=guide, guidance=guidance,
                                           guidance_interval=guidance_interval)
    from . import _runtime_env
    if graph and _runtime_env.GRAPH_REPLAY_SAFE:      # otherwise the eager Heun loop: same values
        solve = model.solver.solve
        model.solver.solve = lambda m, x0, labels=None: solve(m, x0, labels, graph=True)
    C = int(in_channels) if in_channels is not None else int(model.denoiser.in_channels)
    per_rank = (num_samples + world - 1) // world
    first = rank * per_rank
    n_local = max(0, min(per_rank, num_samples - first))
    datamodule = RandomNoiseDataModule(batch_size, num_workers, image_size, n_local, num_classes, in_channels=C,
                                       seed=seed + 1000003 * rank)
    if mean is None or std is None:
        mean, std = (CIFAR_MEAN, CIFAR_STD) if C == 3 else ((0.5,) * C, (0.25,) * C)
    writer = PreditionWriter(output_dir=output_dir, write_interval="batch", mean=mean, std=std, first_index=first)
    trainer = Trainer(accelerator="gpu", strategy="auto", callbacks=[writer])
    if n_local > 0:
        trainer.predict(model, datamodule=datamodule, return_predictions=False, ckpt_path=None, distributed=False)   # generate.py:45-47
    print(f"[rank {rank}] wrote images {first}..{first + n_local - 1} to {output_dir}", flush=True)


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
    parser.add_argument("--solver", choices=["heun", "dpmpp"], default="heun",
                        help="heun (default): EDM's 2nd-order Heun, 2N-1 network evaluations; dpmpp: DPM-Solver++ "
                             "multistep, N evaluations")
    parser.add_argument("--solver_order", type=int, choices=[1, 2, 3], default=2,
                        help="order of --solver dpmpp (default 2: DPM-Solver++(2M))")
    args = parser.parse_args(argv)
    _check_solver(args.solver, args.S_churn)
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
             S_max=args.S_max, S_noise=args.S_noise, solver=args.solver, solver_order=args.solver_order)


if __name__ == "__main__":
    main()
