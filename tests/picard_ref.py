"""numpy restatement of the parallel-in-time solver (tinyedm_amd.ParallelSolver, csrc/picard.hip): the scan, the error
norm, the stride rule, the slide with its extrapolation, the solve loop around any callable D(x [rows, ...], t [rows]),
and the sequential Heun / Euler solve on the same table.  ``dtype`` is the precision of the state arithmetic (float64, or
float32 with the kernels' operation order: every fma is one rounding, emulated through fp64); the error norm is fp64
always, as on the device.  Host only."""
from typing import NamedTuple

import numpy as np


def fma(a, b, c, dtype):
    """a * b + c with one rounding to dtype (float32: through the exact fp64 product; float64: numpy's two roundings)"""
    if dtype == np.float32:
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
    return a * b + c


def _col(t, x):
    return np.asarray(t).reshape(-1, *([1] * (x.ndim - 1)))


def euler_stage(x, D, t0, t1, dtype):
    """ops.adapt_euler: (dx, x1); a row with t1 == t0 rides along"""
    t0, t1 = _col(t0, x).astype(dtype), _col(t1, x).astype(dtype)
    with np.errstate(all="ignore"):
        dx = ((x - D) / t0).astype(dtype)
        x1 = fma(t1 - t0, dx, x, dtype)
    idle = np.broadcast_to(t1 == t0, x.shape)
    return np.where(idle, dtype(0), dx), np.where(idle, x, x1)


def heun_slope(dx, x1, D1, t1, dtype):
    dp = ((x1 - D1) / _col(t1, x1).astype(dtype)).astype(dtype)
    return (dtype(0.5) * dx + dtype(0.5) * dp).astype(dtype)


def live_length(s, N, P):
    return int(min(P, N - 1 - s))


def times(s, ts, N, P):
    """T[P + 1, B]: T[j, b] = t[min(s_b + j, N - 1)]"""
    s = np.asarray(s)
    return np.stack([np.asarray(ts)[np.minimum(s + j, N - 1)] for j in range(P + 1)])


def error_sums(new, old, atol, rtol):
    """sum over a sample's elements of ((new - old) / (atol + rtol max(|old|, |new|)))^2, fp64; a zero scale contributes 0
    where new == old and +inf otherwise.  new, old: [B, ...] -> [B]"""
    n, o = np.asarray(new, np.float64), np.asarray(old, np.float64)
    sc = rtol * np.maximum(np.abs(o), np.abs(n)) + atol
    d = n - o
    with np.errstate(all="ignore"):
        r = d / sc
    r = np.where(sc == 0.0, np.where(d == 0.0, 0.0, np.inf), r)
    return (r * r).reshape(len(r), -1).sum(axis=1)


def error_norm(new, old, atol, rtol):
    n = np.asarray(new)
    return np.sqrt(error_sums(new, old, atol, rtol) / (n.size // len(n)))


def scan(X, slopes, T, L, atol, rtol, dtype):
    """One prefix sum.  X [P + 1, B, ...] the old iterate, slopes [P, B, ...] from it, L [B] the live lengths:
    (Xnew, S) with Xnew[j + 1] = fma(T[j + 1] - T[j], slopes[j], Xnew[j]) over the live j (inactive: copies of Xnew[L]) and
    S [B, P] the error sums of position j + 1 (0 where it is not live)."""
    P, B = X.shape[0] - 1, X.shape[1]
    Xnew = np.empty_like(X)
    Xnew[0] = X[0]
    S = np.zeros((B, P))
    for j in range(P):
        dt = (T[j + 1].astype(dtype) - T[j].astype(dtype)).astype(dtype)
        step = fma(_col(dt, X[0]), slopes[j], Xnew[j], dtype)
        live = np.asarray(L) > j
        Xnew[j + 1] = np.where(_col(live, X[0]), step, Xnew[j])
        S[:, j] = np.where(live, error_sums(Xnew[j + 1], X[j + 1], atol, rtol), 0.0)
    return Xnew, S


def stride_rule(E, L):
    """E: E_1 .. of the live positions (at least L entries); the stride min(m + 1, L), m the leading E_j <= 1 (a NaN is
    not converged)"""
    m = 0
    for j in range(L):
        if not E[j] <= 1.0:
            break
        m += 1
    return min(m + 1, L)


def control(S, CHW, s, status, iters, N, P):
    """picard_control on error sums S [B, P]: (stride, s, status, iters, still_active), arrays of B"""
    B = len(s)
    stride, s, status, iters = np.zeros(B, np.int64), np.array(s, np.int64), np.array(status, np.int64), np.array(iters, np.int64)
    for b in range(B):
        if status[b] != 0:
            continue
        L = live_length(s[b], N, P)
        stride[b] = stride_rule(np.sqrt(S[b] / CHW), L)
        s[b] += stride[b]
        iters[b] += 1
        status[b] = int(s[b] >= N - 1)
    return stride, s, status, iters, int((status == 0).sum())


def slide(Xnew, D, stride, s_old, ts, N, P, dtype):
    """picard_slide: X with X[j] = Xnew[j + r] while j + r <= L; entering positions at table index i <= N - 1 are
    fma(Xnew[L] - Dh, t_i / t_{s+L}, Dh), Dh = D[L - 1]; indices past N - 1 copy Xnew[L]"""
    ts = np.asarray(ts, dtype)
    X = np.empty_like(Xnew)
    for b in range(Xnew.shape[1]):
        r, so = int(stride[b]), int(s_old[b])
        L, sn = live_length(so, N, P), so + r
        for j in range(P + 1):
            i = sn + j
            if j + r <= L:
                X[j, b] = Xnew[j + r, b]
            elif i <= N - 1:
                ratio = dtype(ts[i] / ts[so + L])
                X[j, b] = fma((Xnew[L, b] - D[L - 1, b]).astype(dtype), ratio, D[L - 1, b], dtype)
            else:
                X[j, b] = Xnew[L, b]
    return X


def begin(x0, ts, N, P, dtype):
    """picard_begin: X[j] = t_j x0 (copies of X[0] past the table's end)"""
    ts = np.asarray(ts, dtype)
    x0 = np.asarray(x0, dtype)
    return np.stack([(ts[j if j <= N - 1 else 0] * x0).astype(dtype) for j in range(P + 1)])


class Result(NamedTuple):
    x: np.ndarray                   # the result at t = 0
    x_min: np.ndarray               # the state at t_{N-1}, before the closing Euler step
    iterations: int
    per_sample_iterations: np.ndarray
    strides: list                   # per iteration, the [B] strides
    evaluations: int                # order * iterations + 1
    rows: int


def _close(D, x, ts, N, dtype):
    t = np.full(len(x), ts[N - 1], dtype)
    dx = ((x - np.asarray(D(x, t), dtype)) / dtype(ts[N - 1])).astype(dtype)
    return fma(dtype(0.0) - dtype(ts[N - 1]), dx, x, dtype)


def solve(D, x0, ts, window, order=2, rtol=1e-3, atol=1e-4, dtype=np.float64):
    """The parallel solve of ParallelSolver around D(x [rows, ...], t [rows]); ts: the N + 1 table values (t_N = 0)"""
    ts = np.asarray(ts, dtype)
    N, P, B = len(ts) - 1, int(window), len(x0)
    X = begin(x0, ts, N, P, dtype)
    CHW = X[0].size // B
    s, status, iters = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    strides, iterations = [], 0
    while (status == 0).any():
        assert iterations < N - 1
        T = times(s, ts, N, P)
        L = np.array([live_length(v, N, P) if st == 0 else 0 for v, st in zip(s, status)])
        Dn, slopes = np.zeros_like(X[:P]), np.zeros_like(X[:P])
        for j in range(int(L.max())):
            Dn[j] = np.asarray(D(X[j], T[j]), dtype)
            dx, x1 = euler_stage(X[j], Dn[j], T[j], T[j + 1], dtype)
            if order == 2:
                with np.errstate(all="ignore"):
                    slopes[j] = heun_slope(dx, x1, np.asarray(D(x1, T[j + 1]), dtype), T[j + 1], dtype)
            else:
                slopes[j] = dx
        Xnew, S = scan(X, slopes, T, L, atol, rtol, dtype)
        s_old = s
        stride, s, status, iters, _ = control(S, CHW, s, status, iters, N, P)
        X = slide(Xnew, Dn, stride, s_old, ts, N, P, dtype)
        strides.append(stride)
        iterations += 1
    x_min = X[0]
    return Result(_close(D, x_min, ts, N, dtype), x_min, iterations, iters, strides, order * iterations + 1,
                  order * iterations * P * B + B)


def sequential(D, x0, ts, order=2, dtype=np.float64):
    """DeterministicSolver's table solve (order 1: ops.heun_euler stepped over the table): (x at 0, x at t_{N-1})"""
    ts = np.asarray(ts, dtype)
    N = len(ts) - 1
    x = (ts[0] * np.asarray(x0, dtype)).astype(dtype)
    for i in range(N - 1):
        t0, t1 = np.full(len(x), ts[i], dtype), np.full(len(x), ts[i + 1], dtype)
        dx, x1 = euler_stage(x, np.asarray(D(x, t0), dtype), t0, t1, dtype)
        if order == 2:
            x = fma(_col(t1 - t0, x), heun_slope(dx, x1, np.asarray(D(x1, t1), dtype), t1, dtype), x, dtype)
        else:
            x = x1
    return _close(D, x, ts, N, dtype), x
