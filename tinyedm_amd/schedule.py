"""Optimised sampling schedules: where to put the N steps of a table solve, computed from the model's own trajectories.

The search is the dynamic programme of Chen et al. 2024 ("On the Trajectory Regularity of ODE-based Diffusion Sampling",
GITS; DP over a per-pair cost goes back to Watson et al. 2021): a fine-grid teacher solve of a few hundred samples
(``DeterministicSolver.trace``: every state and slope kept), for every pair of grid nodes the local error of jumping from
one to the other in a single step (``ops.pair_step_errors``, one tiled kernel), and the N-step path through the grid of
least summed error.  ``order=1`` is the paper's Euler cost; ``order=2`` (the default, this project's extension) is the
trapezoid rule along the teacher trajectory, which matches the local error of the Heun solver to leading order.  A sum of
local errors is not the global error: an optimised table can be worse than the Karras one (it is, at N = 5, on the
analytic mixture of the tests), so every report prints the Karras row next to its own.

    python -m tinyedm.schedule --ckpt_path last.ckpt --load_ema --num_steps 8 12 18 --out schedule.json
    python -m tinyedm.generate --ckpt_path last.ckpt --load_ema --num_steps 12 --sigma_table schedule.json ...

The table itself goes to any table solver: ``DeterministicSolver(sigmas=schedule.sigmas)``."""
from __future__ import annotations

import argparse
import json
import os
from dataclasses import asdict, dataclass

import numpy as np
import torch

from . import ops
from .solvers import DeterministicSolver, Trajectory


# ------------------------------------------------------------------ costs
class _CostSum:
    """sum_b sqrt(d2[b]) on the host, in fp64, the samples in index order: the bits do not depend on how the samples were
    chunked"""

    def __init__(self):
        self.acc, self.count = None, 0

    def add(self, d2) -> None:
        d2 = d2.detach().cpu().numpy()
        if self.acc is None:
            self.acc = np.zeros(d2.shape[1:], dtype=np.float64)
        elif self.acc.shape != d2.shape[1:]:
            raise ValueError(f"step_costs: chunks of different grids, {self.acc.shape} and {d2.shape[1:]}")
        for b in range(d2.shape[0]):
            self.acc += np.sqrt(d2[b])
        self.count += d2.shape[0]

    def cost(self) -> np.ndarray:
        G = self.acc.shape[0]
        cost = self.acc / self.count
        cost[np.tril_indices(G, 0, G + 1)] = np.inf
        return cost


def _check_order(who, order) -> None:
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError(f"{who}: order must be 1 (Euler cost) or 2 (trapezoid cost), got {order!r}")


def _add_costs(total: _CostSum, trajectory, order, batch_size) -> None:
    x, slope, sigmas = trajectory
    if not isinstance(x, torch.Tensor) or not isinstance(slope, torch.Tensor) or x.dim() < 3:
        raise ValueError("step_costs: trajectory must be a Trajectory of DeterministicSolver.trace")
    B = x.shape[1]
    tau = torch.as_tensor(sigmas).detach().to(device=x.device, dtype=torch.float64).contiguous()
    step = B if batch_size is None else batch_size
    for b0 in range(0, B, step):
        whole = b0 == 0 and step >= B
        xs = x if whole else x[:, b0:b0 + step].contiguous()
        ss = slope if whole else slope[:, b0:b0 + step].contiguous()
        total.add(ops.pair_step_errors(xs, ss, tau, order))


def step_costs(trajectory: Trajectory, order: int = 2, *, batch_size: int | None = None) -> np.ndarray:
    """cost[i, j] = (1/B) sum_b sqrt(d2[b, i, j]) as a float64 numpy [G, G + 1]: the mean over the trajectory's samples of
    the local error norm of the single step i -> j (``ops.pair_step_errors``), inf where j <= i.  ``batch_size`` bounds
    the samples per kernel call; the samples are added on the host in index order, so the bits do not depend on it."""
    _check_order("step_costs", order)
    if batch_size is not None and (isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1):
        raise ValueError(f"step_costs: batch_size must be a positive integer, got {batch_size!r}")
    total = _CostSum()
    _add_costs(total, trajectory, order, batch_size)
    return total.cost()


# ------------------------------------------------------------------ the path
def best_path(cost, num_steps: int):
    """The path from node 0 to node G - 1 of exactly ``num_steps`` - 1 segments with the least summed cost (added along
    the path), plus the fixed closing segment G - 1 -> G, so that an optimised table keeps the ends of the grid: returns
    (indices of the N nodes, total).  cost: [G, G + 1], entry [i, j] the cost of the segment i -> j (j > i).  Ties go to
    the smaller predecessor index; 2 <= num_steps <= G; num_steps == G returns the grid.  Host numpy, O(N G^2)."""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.ndim != 2 or cost.shape[0] < 2 or cost.shape[1] != cost.shape[0] + 1:
        raise ValueError(f"best_path: cost must be a [G, G + 1] array with G >= 2, got {cost.shape}")
    G = cost.shape[0]
    if isinstance(num_steps, bool) or not isinstance(num_steps, (int, np.integer)) or not 2 <= num_steps <= G:
        raise ValueError(f"best_path: num_steps must be an integer in [2, {G}], got {num_steps!r}")
    N = int(num_steps)
    seg = np.where(np.triu(np.ones((G, G), dtype=bool), 1), cost[:, :G], np.inf)    # only i < j is a segment
    f = np.full(G, np.inf)
    f[0] = 0.0
    prev = np.zeros((N, G), dtype=np.int64)
    for m in range(1, N):
        cand = f[:, None] + seg                 # [i, j]: reach i in m - 1 segments, then i -> j
        prev[m] = np.argmin(cand, axis=0)       # (the first minimum: the smaller predecessor)
        f = cand[prev[m], np.arange(G)]
    if not np.isfinite(f[G - 1] + cost[G - 1, G]):
        raise ValueError("best_path: no path of finite cost (the costs hold inf or nan above the diagonal)")
    idx, j = [G - 1], G - 1
    for m in range(N - 1, 0, -1):
        j = int(prev[m, j])
        idx.append(j)
    return idx[::-1], float(f[G - 1] + cost[G - 1, G])


def _path_cost(cost, indices) -> float:
    total = 0.0
    for a, b in zip(indices[:-1], indices[1:]):
        total = total + cost[a, b]
    return float(total + cost[cost.shape[0] - 1, cost.shape[0]])


# ------------------------------------------------------------------ schedules
@dataclass
class Schedule:
    """one optimised table"""
    sigmas: list            # N Python floats: the fp32 table values (DeterministicSolver(sigmas=...))
    indices: list           # the N grid nodes chosen
    cost: float             # the path's summed cost, closing segment included
    karras_cost: float | None   # the same sum for the evenly subsampled grid (the N-step Karras table) where it exists
    order: int
    grid: int
    warmup: int
    seed: int

    @property
    def num_steps(self) -> int:
        return len(self.sigmas)

    def save(self, path) -> None:
        save_schedules([self], path)

    @staticmethod
    def load(path, num_steps: int | None = None):
        """the schedule of a file for ``num_steps`` (the only one when None); ValueError naming the N the file has"""
        found = load_schedules(path)
        if num_steps is None and len(found) == 1:
            return next(iter(found.values()))
        if num_steps not in found:
            raise ValueError(f"{path} holds no schedule for num_steps = {num_steps}; it has N = {sorted(found)}")
        return found[num_steps]


def save_schedules(schedules, path) -> None:
    """one JSON file of several schedules, one per N"""
    with open(path, "w") as f:
        json.dump({"schedules": [asdict(s) for s in schedules]}, f, indent=1)


def load_schedules(path) -> dict:
    """{N: Schedule} of a file written by save_schedules / Schedule.save"""
    with open(path) as f:
        raw = json.load(f)
    try:
        found = [Schedule(**{k: e[k] for k in Schedule.__dataclass_fields__}) for e in raw["schedules"]]
    except (KeyError, TypeError):
        raise ValueError(f"{path} is not a schedule file (python -m tinyedm.schedule writes one)") from None
    return {s.num_steps: s for s in found}


def schedules_from_costs(cost, sigmas, num_steps, *, order, warmup, seed) -> list:
    """the Schedule of every N of ``num_steps`` from the [G, G + 1] costs of a G-node grid with the levels ``sigmas``"""
    G = cost.shape[0]
    levels = torch.as_tensor(sigmas)[:G].tolist()
    out = []
    for N in num_steps:
        idx, total = best_path(cost, N)
        even = None
        if (G - 1) % (N - 1) == 0:
            s = (G - 1) // (N - 1)
            even = _path_cost(cost, [k * s for k in range(N)])
        out.append(Schedule([levels[i] for i in idx], idx, total, even, int(order), G, int(warmup), int(seed)))
    return out


def optimize_schedule(model, num_steps, *, shape, grid: int = 64, warmup: int = 256, batch_size: int = 64, order: int = 2,
                      seed: int = 0, class_labels=None, num_classes: int | None = None, sigma_min: float = 0.002,
                      sigma_max: float = 80.0, rho: float = 7.0, guide=None, guidance: float = 1.0, guidance_interval=None,
                      device=None, return_costs: bool = False):
    """The optimised ``num_steps``-step table of ``model`` (a list of them for a list of ``num_steps``; the costs are
    computed once).  The teacher is ``DeterministicSolver(num_steps=grid, ...)`` with the given Karras parameters and
    guidance; ``warmup`` samples of ``shape`` (without the batch axis) are traced in chunks of ``batch_size``.  The noise
    comes from ``seed`` on the host; a conditional model gets ``class_labels`` ([warmup]) or, with ``num_classes``,
    labels drawn from ``seed``.  ``return_costs`` adds the [grid, grid + 1] costs to the result."""
    many = not isinstance(num_steps, (int, np.integer))
    wanted = [int(n) for n in num_steps] if many else [int(num_steps)]
    _check_order("optimize_schedule", order)
    for name, v in (("grid", grid), ("warmup", warmup), ("batch_size", batch_size)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"optimize_schedule: {name} must be a positive integer, got {v!r}")
    if not 2 <= grid <= ops.SCHEDULE_MAX_GRID:
        raise ValueError(f"optimize_schedule: grid must be in [2, {ops.SCHEDULE_MAX_GRID}], got {grid}")
    for n in wanted:
        if not 2 <= n <= grid:
            raise ValueError(f"optimize_schedule: num_steps must be in [2, grid = {grid}], got {n}")
    if device is None:
        p = next(model.parameters(), None) if isinstance(model, torch.nn.Module) else None
        device = p.device if p is not None else torch.device("cuda", torch.cuda.current_device())
    teacher = DeterministicSolver(num_steps=grid, sigma_min=sigma_min, sigma_max=sigma_max, rho=rho, guide=guide,
                                  guidance=guidance, guidance_interval=guidance_interval)
    g = torch.Generator().manual_seed(int(seed))
    x0 = torch.randn((warmup, *shape), generator=g, dtype=torch.float32)
    if class_labels is None and num_classes is not None:
        class_labels = torch.randint(0, int(num_classes), (warmup,), generator=g)
    if class_labels is not None and class_labels.shape[0] != warmup:
        raise ValueError(f"optimize_schedule: class_labels must hold one label per warm-up sample ({warmup}), got "
                         f"{tuple(class_labels.shape)}")
    total = _CostSum()
    for b0 in range(0, warmup, batch_size):
        labels = None if class_labels is None else class_labels[b0:b0 + batch_size].to(device)
        traj = teacher.trace(model, x0[b0:b0 + batch_size].to(device), labels)
        _add_costs(total, traj, order, None)
    cost = total.cost()
    found = schedules_from_costs(cost, teacher.t_steps, wanted, order=order, warmup=warmup, seed=seed)
    result = found if many else found[0]
    return (result, cost) if return_costs else result


# ------------------------------------------------------------------ command line
def format_schedule(s: Schedule) -> str:
    karras = "n/a (the grid has no evenly spaced N-step path)" if s.karras_cost is None else f"{s.karras_cost:.6g}"
    return (f"N = {s.num_steps}: cost {s.cost:.6g}, Karras cost {karras}\n"
            f"  nodes  {s.indices}\n  sigmas {[float(f'{v:.6g}') for v in s.sigmas]}")


def build_parser():
    p = argparse.ArgumentParser(description="Optimise the sampling schedule of a checkpoint (DP over local step errors)")
    p.add_argument("--ckpt_path", type=str, default=None)
    p.add_argument("--load_ema", action="store_true")
    p.add_argument("--config_name", type=str, default=None,
                   help="random-init weights of experiments/conf/<name>.yaml instead of a checkpoint (plumbing runs)")
    p.add_argument("--config_path", type=str, default=None)
    p.add_argument("--num_steps", type=int, nargs="+", required=True, help="the N to optimise a table for")
    p.add_argument("--grid", type=int, default=64, help="steps of the teacher's Karras table (default 64)")
    p.add_argument("--warmup", type=int, default=256, help="teacher samples (default 256)")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--order", type=int, choices=[1, 2], default=2,
                   help="2 (default): trapezoid cost, for Heun; 1: the Euler cost of the paper")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--image_size", type=int, default=32)
    p.add_argument("--in_channels", type=int, default=None)
    p.add_argument("--network_dtype", choices=["bf16", "f32", "f32x3"], default="f32x3")
    p.add_argument("--sigma_min", type=float, default=0.002)
    p.add_argument("--sigma_max", type=float, default=80.0)
    p.add_argument("--rho", type=float, default=7.0)
    p.add_argument("--guide_ckpt_path", type=str, default=None)
    p.add_argument("--guide_load_ema", action="store_true")
    p.add_argument("--guide_unconditional", action="store_true")
    p.add_argument("--guidance", type=float, default=1.0)
    p.add_argument("--guidance_interval", type=float, nargs=2, metavar=("LO", "HI"), default=None)
    p.add_argument("--out", type=str, required=True, metavar="schedule.json")
    return p


def main(argv=None):
    from . import networks
    from .config import compose, instantiate
    from .edm import EDM
    parser = build_parser()
    args = parser.parse_args(argv)
    if (args.ckpt_path is None) == (args.config_name is None):
        parser.error("give --ckpt_path or --config_name (random init), one of them")
    if args.guide_unconditional and args.guide_ckpt_path is not None:
        parser.error("--guide_unconditional evaluates the model itself as the guide: no --guide_ckpt_path")
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.ckpt_path is not None:
        model = EDM.load_from_checkpoint(args.ckpt_path, load_ema=args.load_ema)
    else:
        conf_dir = args.config_path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                    "experiments", "conf")
        cfg = compose(args.config_name, conf_dir)
        networks.manual_seed(cfg.seed)
        torch.manual_seed(cfg.seed)
        model = instantiate(cfg.model)
    model = model.to(dev).eval()
    model.denoiser.set_eval_dtype(args.network_dtype)
    guide = "unconditional" if args.guide_unconditional else None
    if args.guide_ckpt_path is not None:
        guide = EDM.load_from_checkpoint(args.guide_ckpt_path, load_ema=args.guide_load_ema).to(dev).eval()
        guide.denoiser.set_eval_dtype(args.network_dtype)
    C = int(args.in_channels) if args.in_channels is not None else int(model.denoiser.in_channels)
    try:
        found = optimize_schedule(model, list(args.num_steps), shape=(C, args.image_size, args.image_size), grid=args.grid,
                                  warmup=args.warmup, batch_size=args.batch_size, order=args.order, seed=args.seed,
                                  num_classes=model.num_classes if model.conditional else None, sigma_min=args.sigma_min,
                                  sigma_max=args.sigma_max, rho=args.rho, guide=guide, guidance=args.guidance,
                                  guidance_interval=args.guidance_interval, device=dev)
    except ValueError as e:
        parser.error(str(e))
    for s in found:
        print(format_schedule(s), flush=True)
    save_schedules(found, args.out)
    print(f"wrote {len(found)} schedule(s) to {args.out}", flush=True)


if __name__ == "__main__":
    main()
