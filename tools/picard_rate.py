"""Iterations, network rows and latency of the parallel-in-time solver against the table solver on the CIFAR-10 net:
python tools/picard_rate.py [--dtypes bf16,f32x3] [--batches 1,4,16] [--windows 8,16,31] [--rtols 1e-2,1e-3,0]
                            [--num_steps 32] [--reps 3] [--out_gain G]

The net is the RANDOM-INIT cifar10 config (bench.build_model): no trained checkpoint is in the tree, so the iteration
counts are those of an untrained denoiser, not of a model one would sample from.  More than that: the net's output gain
is initialised to 0, so as initialised it computes D(x, sigma) = c_skip(sigma) x exactly, the denoiser of Gaussian data,
at the full cost of the network.  `--out_gain G` sets the gain to G instead, which puts the random network's output
into D (an arbitrary, rough denoiser: the other extreme).  Per precision and batch size B the
yardstick is DeterministicSolver (Heun, 2N - 1 evaluations), graph=True and eager; then per window and tolerance (atol =
rtol / 10) ParallelSolver: iterations, sequential depth (2 iterations + 1 batched evaluations), network rows, ms per
solve graph=True and eager, and the worst per-sample RMS distance of its result to the sequential one.  A solve is timed
with device events around `reps` solves after a warm-up solve of the same shape (the warm-up captures); the parallel
solver's host reads of the active count are inside the window, as they are in use.  One GPU process."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import tinyedm  # noqa: E402


def timed(run, reps):
    """ms per call of run(), device events around `reps` calls after one warm-up call; returns (ms, the last result)"""
    out = run()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        out = run()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps, out


def rms(a, b):
    return float(((a.double() - b.double()) ** 2).flatten(1).mean(dim=1).sqrt().max())


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--dtypes", default="bf16,f32x3")
    p.add_argument("--batches", default="1,4,16")
    p.add_argument("--windows", default="8,16,31")
    p.add_argument("--rtols", default="1e-2,1e-3,0")
    p.add_argument("--num_steps", type=int, default=32)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--out_gain", type=float, default=None, help="set the denoiser's output gain (0 as initialised)")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("picard_rate: needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    model, _ = bench.build_model(dev)
    if args.out_gain is not None:
        with torch.no_grad():
            model.denoiser.gain_out.fill_(args.out_gain)
    model.eval()
    N = args.num_steps
    print(f"# {torch.cuda.get_device_name(0)}, random-init net (cifar10 config, no trained checkpoint), output gain "
          f"{float(model.denoiser.gain_out.detach()):g}, N = {N} steps, {args.reps} timed solves per figure", flush=True)
    print("| dtype | B | solver | window | rtol | iterations | depth (evaluations) | rows | graph ms | eager ms | rms to "
          "sequential |", flush=True)
    print("|---|---|---|---|---|---|---|---|---|---|---|", flush=True)
    for dtype in args.dtypes.split(","):
        model.denoiser.set_eval_dtype(dtype)
        for B in (int(v) for v in args.batches.split(",")):
            x0 = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(7)).to(dev)
            heun = tinyedm.DeterministicSolver(num_steps=N)
            tg, seq = timed(lambda: heun.solve(model, x0, None, graph=True), args.reps)
            te, seq_e = timed(lambda: heun.solve(model, x0, None), args.reps)
            assert torch.equal(seq, seq_e)
            print(f"| {dtype} | {B} | heun | - | - | - | {2 * N - 1} | {(2 * N - 1) * B} | {tg:.2f} | {te:.2f} | 0 |", flush=True)
            for P in (int(v) for v in args.windows.split(",")):
                for rtol in (float(v) for v in args.rtols.split(",")):
                    sol = tinyedm.ParallelSolver(num_steps=N, window=P, rtol=rtol, atol=rtol / 10)
                    pg, out = timed(lambda: sol.solve(model, x0, None, graph=True), args.reps)
                    st = sol.last_stats
                    pe, out_e = timed(lambda: sol.solve(model, x0, None), args.reps)
                    assert torch.equal(out, out_e) and sol.last_stats.iterations == st.iterations
                    print(f"| {dtype} | {B} | picard | {P} | {rtol:g} | {st.iterations} | {st.evaluations} | {st.rows} | "
                          f"{pg:.2f} | {pe:.2f} | {rms(out, seq):.3g} |", flush=True)


if __name__ == "__main__":
    main()
