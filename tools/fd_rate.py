"""The fp64 moments and polynomial-kernel sums (csrc/moments.hip, ops.moments / ops.poly_kernel_sums) against the same
quantities formed in torch on the same device, which is what a user can do without them:
    moments:  X.double() -> s = Xd.sum(0), G = Xd.T @ Xd          (an fp64 copy of the set, one fp64 GEMM)
    KID sums: per subset the three fp64 grams of the gathered rows, (gamma G + coef0) ** degree, .sum()
and against the fp64 matrix rate this device sustains (tools/mfma_shape/mfma_f64.hip: a bare MFMA loop over a tile resident
in LDS; built on demand with hipcc, skipped with --no_mfma).
    python tools/fd_rate.py [--rows 50000] [--subsets 100] [--subset_size 1000] [--out fd_rate.json]
Protocol of tools/microbench_knn.py: both forms are warmed up, then timed in alternating rounds in one process; a round is
a batch of calls between two device events, sized from the warm-up to last about --window seconds.  Peak extra memory: the
allocator's high-water mark above the resident inputs during one call.  Prints, per workload: the two times per call
(median and min over the rounds), the peak extra memory of both, the fp64 TFLOP/s of both forms on the nominal count
(2 N D^2 for the full gram: the rate a user sees), the share of the measured MFMA rate that the new path reaches on the
FLOPs it executes (the moments compute only the tiles on and above the diagonal, T (T + 1) / 2 of T^2), and the largest
difference between the two results."""
import argparse
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from microbench_knn import alternate  # noqa: E402
from tinyedm_amd import ops  # noqa: E402
from tinyedm_amd.frechet import subset_indices  # noqa: E402

dev = "cuda"


def mfma_rate():
    """TFLOP/s of the bare fp64 MFMA loop (None if it cannot be built or run)"""
    src, exe = os.path.join(HERE, "mfma_shape", "mfma_f64.hip"), os.path.join(HERE, "mfma_shape", "mfma_f64")
    try:
        if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
            subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-o", exe, src],
                           check=True, capture_output=True, timeout=600)
        out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=300).stdout
        return json.loads(out.strip().splitlines()[-1])
    except (OSError, subprocess.SubprocessError, ValueError) as e:
        print(f"mfma_f64: not measured ({e})", flush=True)
        return None


def peak_extra(fn):
    """bytes the allocator holds at most during fn() above what it holds before"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def torch_moments(x):
    xd = x.double()
    return xd.sum(0), xd.t() @ xd


def torch_kernel_sums(x, ix, y, iy, gamma, coef0, degree):
    """[S, 3]: the xx (diagonal left out by index), yy and xy sums of every subset"""
    out = torch.empty(ix.shape[0], 3, dtype=torch.float64, device=x.device)
    for s in range(ix.shape[0]):
        a, b = x[ix[s]].double(), y[iy[s]].double()
        for c, (u, v, diag) in enumerate(((a, a, True), (b, b, True), (a, b, False))):
            k = (gamma * (u @ v.t()) + coef0) ** degree
            out[s, c] = k.sum() - (k.diagonal().sum() if diag else 0.0)
    return out


def hip_kernel_sums(x, ix, y, iy, gamma, coef0, degree):
    return torch.stack([ops.poly_kernel_sums(x, ix, x, ix, gamma, coef0, degree, True),
                        ops.poly_kernel_sums(y, iy, y, iy, gamma, coef0, degree, True),
                        ops.poly_kernel_sums(x, ix, y, iy, gamma, coef0, degree, False)], dim=1)


def row(name, shape, flops, executed, new, old, new_fn, old_fn, diff, mfma):
    (_, n_med, n_min, n_calls), (_, o_med, o_min, o_calls) = new, old
    res = {"workload": name, "shape": shape, "hip_s_median": n_med, "hip_s_min": n_min, "torch_s_median": o_med,
           "torch_s_min": o_min, "calls_per_round": [n_calls, o_calls], "hip_fp64_tflops": flops / n_med / 1e12,
           "torch_fp64_tflops": flops / o_med / 1e12, "speedup_over_torch": o_med / n_med,
           "hip_peak_extra_bytes": peak_extra(new_fn), "torch_peak_extra_bytes": peak_extra(old_fn), "max_rel_difference": diff,
           "hip_executed_fp64_tflops": executed / n_med / 1e12,
           "share_of_mfma_rate": None if mfma is None else executed / n_med / 1e12 / mfma["tflops"]}
    share = f" nominal, {res['hip_executed_fp64_tflops']:.1f} executed"
    share += "" if mfma is None else f" = {100 * res['share_of_mfma_rate']:.0f} % of the bare MFMA loop"
    print(f"{name} {shape}: hip {n_med * 1e3:.2f} ms (min {n_min * 1e3:.2f}), {res['hip_fp64_tflops']:.1f} fp64 TFLOP/s{share}, "
          f"peak extra {res['hip_peak_extra_bytes'] / 2 ** 20:.0f} MiB   torch {o_med * 1e3:.2f} ms (min {o_min * 1e3:.2f}), "
          f"peak extra {res['torch_peak_extra_bytes'] / 2 ** 20:.0f} MiB  -> {res['speedup_over_torch']:.2f}x   "
          f"largest relative difference {diff:.2e}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--subset_size", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed batch")
    ap.add_argument("--no_mfma", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    mfma = None if args.no_mfma else mfma_rate()       # (a process of its own, before this one holds the device busy)
    if mfma is not None:
        print(f"bare v_mfma_f64_16x16x4_f64 loop: {mfma['tflops']:.1f} TFLOP/s on {mfma['cus']} CUs", flush=True)
    g = torch.Generator(device=dev).manual_seed(0)
    results = []
    N = args.rows
    for name, D, make in (("moments uint8", 3072, lambda D: torch.randint(0, 256, (N, D), dtype=torch.uint8, device=dev, generator=g)),
                          ("moments float32", 2048, lambda D: torch.randn(N, D, device=dev, generator=g).abs_())):
        x = make(D)
        new_fn, old_fn = (lambda: ops.moments(x)), (lambda: torch_moments(x))
        new, old = alternate([new_fn, old_fn], args.rounds, args.window)
        diff = max(float(((a - b).abs().max() / b.abs().max())) for a, b in zip(new[0], old[0]))
        T = (D + 63) // 64
        results.append(row(name, f"{N} x {D}, splits {ops.moments_splits(N, D)}", 2.0 * N * D * D,
                           2.0 * N * 64 * 64 * (T * (T + 1) // 2), new, old, new_fn, old_fn, diff, mfma))
        del x, new, old
        torch.cuda.empty_cache()
    S, m, D = args.subsets, args.subset_size, 3072
    x = torch.randint(0, 256, (max(N, m), D), dtype=torch.uint8, device=dev, generator=g)
    y = torch.randint(0, 256, (max(N // 5, m), D), dtype=torch.uint8, device=dev, generator=g)
    hx, hy = subset_indices(x.shape[0], y.shape[0], S, m, 0)
    ix, iy = torch.from_numpy(hx).to(dev), torch.from_numpy(hy).to(dev)
    gamma = 1.0 / D / 255.0 ** 2
    new_fn = lambda: hip_kernel_sums(x, ix, y, iy, gamma, 1.0, 3)        # noqa: E731
    old_fn = lambda: torch_kernel_sums(x, ix, y, iy, gamma, 1.0, 3)      # noqa: E731
    new, old = alternate([new_fn, old_fn], args.rounds, args.window)
    diff = float(((new[0] - old[0]).abs() / old[0].abs()).max())
    results.append(row("KID sums uint8", f"{S} x {m} of {x.shape[0]} and {y.shape[0]} x {D}", 3 * 2.0 * S * m * m * D,
                       3 * 2.0 * S * (((m + 63) // 64) * 64) ** 2 * D, new, old, new_fn, old_fn, diff, mfma))
    out = {"device": torch.cuda.get_device_name(0), "mfma_f64": mfma, "results": results}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
