"""The parallel-in-time solver on the GPU (ParallelSolver, ops.picard_*, csrc/picard.hip):

 * picard_scan against fp64 from the same fp32 operands under a bound derived from the rounding count, and against the
   fp32 restatement of tests/picard_ref.py; the partials and E; inactive positions; the batch; the zero scale;
 * picard_control against the reference on hand-made partials, two waves; picard_slide and picard_begin;
 * the bitwise fixed point: at rtol = atol = 0 the solver returns DeterministicSolver's bits on row-wise analytic
   denoisers; tolerances against the reference; a sample alone;
 * tiny nets against picard_ref run around the oracle's forward, "f32" and bf16, unguided and CFG at w = 2;
 * graph == eager; the generate CLI, EDM.predict_step and guidance 1 end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import picard_ref as R
from parity_log import record
from test_adaptive_solver_cpu import gaussian, mixture, setting
from test_adaptive_solver_gpu import _gaussian_gpu, _mixture_gpu, _oracle_callable, _rowwise, _tiny_case
from test_multistep_solver_gpu import _edm, _oracle_D, rel

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
N_ = 18
ATOL, RTOL_K = 1e-4, 1e-3                       # the tolerances of the kernel tests
SHAPES = [(1, 5, 1), (3, 4099, 4), (7, 3072, 8), (2, 1024, 64)]         # (B, CHW, P)
SHAPE_IDS = ["1x5-P1", "3x4099-P4-tail-misaligned", "7x3072-P8", "2x1024-P64"]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def _table():
    import tinyedm_amd as T
    return T.DeterministicSolver(num_steps=N_).t_steps


def _starts(B):
    """a different window start per sample, the first at N - 2 (one live position: the window touches the table end)"""
    return np.array([N_ - 2]) if B == 1 else np.linspace(N_ - 2, 0, B).round().astype(np.int64)


def _state(s, status=None, iters=None):
    s = np.asarray(s, np.int32)
    rows = np.stack([s, np.zeros_like(s) if status is None else np.asarray(status, np.int32),
                     np.zeros_like(s) if iters is None else np.asarray(iters, np.int32)])
    return torch.from_numpy(rows).to(DEV)


def _window(ops, B, CHW, P, seed, s=None):
    """a window with real Euler-stage operands: X at the noise level of its positions, D and D1 ~ 0.5 N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    ts = _table()
    s = _starts(B) if s is None else np.asarray(s)
    Tn = R.times(s, ts.numpy(), N_, P).astype(np.float32)                       # [P + 1, B]
    T = torch.from_numpy(Tn).to(DEV)
    X = (torch.randn(P + 1, B, CHW, generator=g) * torch.from_numpy(Tn)[:, :, None]).to(DEV)
    D, D1 = (0.5 * torch.randn(P, B, CHW, generator=g).to(DEV) for _ in range(2))
    dx, X1 = ops.adapt_euler(X[:P].view(P * B, CHW), D.view(P * B, CHW), T[:P].view(-1), T[1:].view(-1))
    L = np.array([R.live_length(v, N_, P) for v in s])
    return dict(X=X, D=D, D1=D1, dx=dx.view(P, B, CHW), X1=X1.view(P, B, CHW), T=T, s=s, L=L, state=_state(s), ts=ts.to(DEV))


def _scan(ops, w, order, atol=ATOL, rtol=RTOL_K):
    return ops.picard_scan(w["X"], w["dx"], w["X1"] if order == 2 else None, w["D1"] if order == 2 else None, w["T"],
                           w["state"], atol, rtol, N=N_)


def _errors(ops, w, part, CHW):
    """E [B, P] of the live positions through picard_control (on a copy of the state)"""
    B, P = part.shape[0], part.shape[1]
    err = torch.full((B, P), -1.0, dtype=torch.float64, device=DEV)
    ops.picard_control(part, CHW, w["state"].clone(), N_, P, torch.zeros(1, dtype=torch.int32, device=DEV), err=err)
    return err.cpu().numpy()


def _np(t):
    return t.double().cpu().numpy()


# ------------------------------------------------------------------ the scan
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("B,CHW,P", SHAPES, ids=SHAPE_IDS)
def test_scan_vs_reference(ops, B, CHW, P, order):
    w = _window(ops, B, CHW, P, 100 * B + P + order)
    assert w["L"][0] == 1 and (B == 1 or w["L"].max() == min(P, N_ - 1))
    ops.check_health(DEV, "before")
    Xnew, part = _scan(ops, w, order)
    E = _errors(ops, w, part, CHW)
    ops.check_health(DEV, "picard_scan")
    X, DX, X1, D1, T = (_np(w[k]) for k in ("X", "dx", "X1", "D1", "T"))
    got = _np(Xnew)
    assert np.array_equal(got[0], X[0])
    # (1) Xnew against fp64 from the same fp32 operands.  A step is new' = fma(dt, s, new): dt = t1 - t0 (1 rounding, eps
    # |dt|), for order 2 dp = (x1 - D1) / t1 (2 roundings, each <= eps A, A = (|x1| + |D1|) / |t1|) and s = 0.5 dx + 0.5 dp
    # (1 rounding, <= eps S, S = |dx| / 2 + A / 2), and the final rounding eps |new'|: a step adds at most
    # eps (|new'| + |dt| (A + 3 S)) <= 5 eps (|new'| + |dt| S), taken as 6 eps for the second-order terms; order 1 has the
    # roundings of dt and of the fma only: 3 eps (|new'| + |dt| |dx|).  The errors of the steps add up along the chain.
    new64, bound = np.zeros_like(got), np.zeros_like(got)
    new64[0] = X[0]
    c = 6 if order == 2 else 3
    for j in range(P):
        dt = (T[j + 1] - T[j])[:, None]
        with np.errstate(all="ignore"):
            A = (np.abs(X1[j]) + np.abs(D1[j])) / np.abs(T[j + 1])[:, None]
            slope = 0.5 * DX[j] + 0.5 * (X1[j] - D1[j]) / T[j + 1][:, None] if order == 2 else DX[j]
        S = 0.5 * np.abs(DX[j]) + 0.5 * A if order == 2 else np.abs(DX[j])
        live = (w["L"] > j)[:, None]
        new64[j + 1] = np.where(live, new64[j] + dt * slope, new64[j])
        bound[j + 1] = np.where(live, bound[j] + c * EPS32 * (np.abs(new64[j + 1]) + np.abs(dt) * S), bound[j])
    worst = (np.abs(got - new64) / np.maximum(bound, 1e-300))[1:].max()
    print(f"Xnew vs fp64: worst |diff| / bound {worst:.3f}")
    assert np.all(np.abs(got - new64) <= bound), worst
    # the fp32 restatement (every fma one rounding) gives the bits, but for the double rounding of its emulated fma
    f = np.float32
    X32, DX32, X132, D132, T32 = (v.astype(f) for v in (X, DX, X1, D1, T))
    with np.errstate(all="ignore"):
        slopes = np.stack([R.heun_slope(DX32[j], X132[j], D132[j], T32[j + 1], f) for j in range(P)]) if order == 2 else DX32
    ref32, _ = R.scan(X32, slopes, T32, w["L"], ATOL, RTOL_K, f)
    ulps = np.abs(got - ref32) / np.spacing(np.abs(ref32).astype(np.float32))
    print(f"Xnew vs the fp32 restatement: {int((ulps > 0).sum())} of {ulps.size} elements differ, worst {ulps.max():.1f} ulp")
    assert ulps.max() <= 1.0
    # (2) the partials are the fp64 sum over the kernel's own fp32 values: every term is computed in fp64 (a handful of
    # roundings of 2^-53 each) and CHW <= 4099 non-negative terms are added in a fixed order: relative error < 1e-11
    n = ops.picard_chunks(CHW)
    assert part.shape == (B, P, n)
    s_dev = part.sum(dim=2).cpu().numpy()
    for j in range(P):
        s_ref = np.where(w["L"] > j, R.error_sums(got[j + 1], X[j + 1], ATOL, RTOL_K), 0.0)
        assert np.all(np.abs(s_dev[:, j] - s_ref) <= 1e-11 * s_ref), (j, s_dev[:, j], s_ref)
        # (3) E against fp64 from the fp64 chain: a term q = (new - old) / sc moves by at most dq = bound / sc (1 + rtol |q|)
        # (sc depends on |new| too), and E is an RMS: |E - E64| <= sqrt(mean dq^2); E stays fp64 on the device (1e-11 E)
        sc = ATOL + RTOL_K * np.maximum(np.abs(X[j + 1]), np.abs(new64[j + 1]))
        q64 = (new64[j + 1] - X[j + 1]) / sc
        E64 = np.sqrt((q64 * q64).mean(axis=1))
        dq = bound[j + 1] / sc * (1 + RTOL_K * np.abs(q64))
        lim = np.sqrt((dq * dq).mean(axis=1)) + 1e-11 * E64
        live = w["L"] > j
        assert np.all(np.abs(E[live, j] - E64[live]) <= lim[live]), (j, E[live, j], E64[live], lim[live])
        assert np.all(lim[live] <= 0.05 * E64[live])            # (the bound is a statement about E, not a blank cheque)
        assert np.all(E[~live, j] == -1.0)                      # E of a position that is not live is not written
    # inactive positions are copies of the last live one
    for b in range(B):
        for j in range(w["L"][b] + 1, P + 1):
            assert torch.equal(Xnew[j, b], Xnew[w["L"][b], b])


def test_inactive_positions_are_never_read(ops):
    B, CHW, P = 3, 1028, 4
    w = _window(ops, B, CHW, P, 7, s=[N_ - 2, 0, N_ - 3])              # live lengths 1, 4, 2
    assert w["L"].tolist() == [1, 4, 2]
    clean = _scan(ops, w, 2)
    stride = torch.tensor([1, 2, 1], dtype=torch.int32, device=DEV)
    after = _state(w["s"] + np.array([1, 2, 1]))
    clean_slide = ops.picard_slide(clean[0], w["D"].view(P * B, CHW), stride, after, w["ts"], N=N_)
    for b, L in enumerate(w["L"]):
        for j in range(L, P):
            w["dx"][j, b, 3], w["X1"][j, b, 1027], w["D1"][j, b, 0] = float("nan"), float("inf"), float("nan")
            w["D"][j, b, 5] = float("nan")
    ops.check_health(DEV, "before")
    Xnew, part = _scan(ops, w, 2)
    assert torch.equal(Xnew, clean[0]) and torch.equal(part, clean[1])
    X, T = ops.picard_slide(Xnew, w["D"].view(P * B, CHW), stride, after, w["ts"], N=N_)
    assert torch.equal(X, clean_slide[0]) and torch.equal(T, clean_slide[1])
    ops.check_health(DEV, "an inactive position's operands must not matter")
    # a non-finite LIVE state raises bit 2 of the health word
    w["D1"][1, 1, 1027] = float("inf")
    _scan(ops, w, 2)
    with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
        ops.check_health(DEV, "picard_scan")
    ops.check_health(DEV, "after")                  # the read cleared the word


@pytest.mark.parametrize("CHW", [3 * 32 * 32, 4099])
def test_scan_does_not_depend_on_the_batch(ops, CHW):
    B, P = 7, 8
    w = _window(ops, B, CHW, P, 23)
    Xnew, part = _scan(ops, w, 2)
    E = _errors(ops, w, part, CHW)
    one = {k: w[k][:, 5:6].contiguous() for k in ("X", "D", "D1", "dx", "X1", "T")}
    one["state"] = _state(w["s"][5:6])
    Xnew1, part1 = _scan(ops, one, 2)
    E1 = _errors(ops, one, part1, CHW)
    assert torch.equal(Xnew1[:, 0], Xnew[:, 5]) and torch.equal(part1[0], part[5])
    assert np.array_equal(E1[0], E[5]) and w["L"][5] > 1


def test_zero_scale(ops):
    B, CHW, P = 2, 1028, 4
    w = _window(ops, B, CHW, P, 31, s=[0, N_ - 4])                       # live lengths 4, 3
    Xnew, _ = _scan(ops, w, 2, atol=0.0, rtol=0.0)
    w["X"] = Xnew.clone()                   # the slopes are operands: the new iterate is the old one again
    Xnew2, part = _scan(ops, w, 2, atol=0.0, rtol=0.0)
    assert torch.equal(Xnew2, Xnew)
    E = _errors(ops, w, part, CHW)
    assert np.all(E[0, :4] == 0.0) and np.all(E[1, :3] == 0.0)
    stride = ops.picard_control(part, CHW, w["state"].clone(), N_, P, torch.zeros(1, dtype=torch.int32, device=DEV))
    assert stride.tolist() == [4, 3]
    w["X"][2, 0, 1027] = torch.nextafter(w["X"][2, 0, 1027], torch.tensor(float("inf"), device=DEV))      # one ulp
    _, part = _scan(ops, w, 2, atol=0.0, rtol=0.0)
    E = _errors(ops, w, part, CHW)
    assert E[0, 0] == 0.0 and E[0, 1] == np.inf and E[0, 2] == 0.0 and np.all(E[1, :3] == 0.0)
    stride = ops.picard_control(part, CHW, w["state"].clone(), N_, P, torch.zeros(1, dtype=torch.int32, device=DEV))
    assert stride.tolist() == [2, 3]
    ops.check_health(DEV, "zero scale")


# ------------------------------------------------------------------ the controller
def test_control_against_the_reference(ops):
    B, CHW, P, N = 70, 3 * 32 * 32, 5, 12
    n = ops.picard_chunks(CHW)
    assert n == 3
    g = np.random.default_rng(5)
    s = g.integers(0, N - 1, B)
    s[:7] = [0, N - 2, N - 3, N - 1, 1, 2, 3]
    status = (s == N - 1).astype(np.int64)
    iters = g.integers(0, 9, B)
    # E^2 CHW split over the three chunks; every pattern of converged / not converged, NaN and inf among them
    E = np.where(g.random((B, P)) < 0.6, g.uniform(0.0, 1.0, (B, P)), g.uniform(1.0, 50.0, (B, P)))
    E[0], E[1], E[2] = 0.5, [0.5, 9, 9, 9, 9], [0.5, 0.5, 0.5, 9, 9]                # all converged; clamped at the end
    E[4], E[5], E[6] = [5, 0.1, 0.1, 0.1, 0.1], [0.1, np.nan, 0.1, 0.1, 0.1], [1.0, np.inf, 0.1, 0.1, 0.1]
    part = np.stack([0.5 * E * E * CHW, 0.25 * E * E * CHW, 0.25 * E * E * CHW], axis=2)
    S = (part[:, :, 0] + part[:, :, 1]) + part[:, :, 2]                              # the device's order
    part[s == N - 1] = np.nan                                                        # a done sample's partials are not read
    active = torch.full((1,), 100, dtype=torch.int32, device=DEV)
    state = _state(s, status, iters)
    err = torch.full((B, P), -1.0, dtype=torch.float64, device=DEV)
    stride = ops.picard_control(torch.from_numpy(part).to(DEV), CHW, state, N, P, active, err=err)
    r_stride, r_s, r_status, r_iters, still = R.control(S, CHW, s, status, iters, N, P)
    got = state.cpu().numpy()
    assert stride.cpu().numpy().tolist() == r_stride.tolist()
    assert got[0].tolist() == r_s.tolist() and got[1].tolist() == r_status.tolist() and got[2].tolist() == r_iters.tolist()
    assert int(active.item()) == 100 + still and 0 < still < B
    assert r_stride[:7].tolist() == [5, 1, 2, 0, 1, 2, 2]
    e = err.cpu().numpy()
    for b in range(B):
        L = R.live_length(s[b], N, P) if status[b] == 0 else 0
        assert np.allclose(e[b, :L], np.sqrt(S[b, :L] / CHW), rtol=4e-16, atol=0.0, equal_nan=True) and np.all(e[b, L:] == -1.0)


# ------------------------------------------------------------------ the slide and the begin
@pytest.mark.parametrize("B,CHW,P", SHAPES[1:], ids=SHAPE_IDS[1:])
def test_slide(ops, B, CHW, P):
    g = torch.Generator().manual_seed(B + CHW + P)
    ts = _table()
    s_old = _starts(B)
    L = np.array([R.live_length(v, N_, P) for v in s_old])
    stride = np.array([max(1, (int(l) * (b + 1)) // B) for b, l in enumerate(L)])     # 1 .. L, the last sample slides by L
    assert (stride >= 1).all() and (stride <= L).all() and stride[-1] == L[-1]
    Xnew = (ts[0] * torch.randn(P + 1, B, CHW, generator=g)).to(DEV)
    D = (0.5 * torch.randn(P, B, CHW, generator=g)).to(DEV)
    state = _state(s_old + stride)
    X, T = ops.picard_slide(Xnew, D, torch.from_numpy(stride.astype(np.int32)).to(DEV), state, ts.to(DEV), N=N_)
    assert X.data_ptr() != Xnew.data_ptr()
    ref = R.slide(Xnew.cpu().numpy(), D.cpu().numpy(), stride, s_old, ts.numpy(), N_, P, np.float32)
    assert np.array_equal(T.cpu().numpy(), R.times(s_old + stride, ts.numpy(), N_, P).astype(np.float32))
    got = X.cpu().numpy()
    entered = 0
    for b in range(B):
        for j in range(P + 1):
            i = s_old[b] + stride[b] + j
            if j + stride[b] <= L[b]:
                assert torch.equal(X[j, b], Xnew[j + stride[b], b])              # shifted: bit for bit
            elif i <= N_ - 1:
                ulp = np.spacing(np.abs(ref[j, b]))
                assert np.all(np.abs(got[j, b].astype(np.float64) - ref[j, b]) <= 2 * ulp), (b, j)
                entered += 1
            else:
                assert torch.equal(X[j, b], Xnew[L[b], b])                       # past the table's end: copies
    assert (entered > 0) == (P < N_ - 1)            # (a window over the whole table has nothing left to enter)
    with pytest.raises(ValueError, match="alias"):
        ops.picard_slide(Xnew, D, torch.from_numpy(stride.astype(np.int32)).to(DEV), state, ts.to(DEV), N=N_, X=Xnew)


@pytest.mark.parametrize("B,CHW,P", SHAPES, ids=SHAPE_IDS)
def test_begin(ops, B, CHW, P):
    g = torch.Generator().manual_seed(B + CHW + P)
    ts = _table()
    x0 = torch.randn(B, CHW, generator=g).to(DEV)
    X, T, state = ops.picard_begin(x0, ts.to(DEV), N_, P)
    assert X.shape == (P + 1, B, CHW) and T.shape == (P + 1, B) and state.shape == (ops.PICARD_ROWS, B)
    assert torch.equal(X[0], ops.scale_f32(x0, ts[0].item()))                  # the table solver's first state
    x64 = x0.double().cpu().numpy()
    for j in range(1, P + 1):
        want = ts[j].double().item() * x64 if j <= N_ - 1 else ts[0].double().item() * x64
        assert np.all(np.abs(_np(X[j]) - want) <= np.spacing(np.abs(want).astype(np.float32))), j
    assert np.array_equal(T.cpu().numpy(), R.times(np.zeros(B, np.int64), ts.numpy(), N_, P).astype(np.float32))
    rows = ops.picard_rows(state)
    assert not rows.start.any() and not rows.status.any() and not rows.iterations.any()


# ------------------------------------------------------------------ the solver on analytic denoisers
@pytest.fixture(scope="module")
def analytic(ops):
    means, x0 = setting()
    return torch.from_numpy(x0).float().to(DEV), x0, \
        {"gaussian": (_rowwise(_gaussian_gpu), gaussian), "mixture": (_rowwise(_mixture_gpu(means)), mixture(means))}


@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_zero_tolerance_returns_the_bits_of_the_table_solver(analytic, name):
    """the central test: the fixed point of the iteration IS the sequential solve, bit for bit"""
    import tinyedm_amd as T
    x0, _, dens = analytic
    D = dens[name][0]
    heun = T.DeterministicSolver(num_steps=N_).solve(D, x0)
    for P in (1, 5, 17):
        sol = T.ParallelSolver(num_steps=N_, window=P, order=2, rtol=0.0, atol=0.0)
        out = sol.solve(D, x0)
        st = sol.last_stats
        assert torch.equal(out, heun), (P, (out - heun).abs().max().item())
        assert st.iterations <= N_ - 1 and st.evaluations == 2 * st.iterations + 1 and st.guide_evaluations == 0
        assert st.sequential_evaluations == 2 * (N_ - 1) + 1 and st.rows == 2 * st.iterations * P * x0.shape[0] + x0.shape[0]
        assert st.per_sample_iterations.shape == (x0.shape[0],) and not st.per_sample_iterations.is_cuda
        assert st.per_sample_iterations.dtype == torch.int64 and int(st.per_sample_iterations.max()) == st.iterations
        if P == 1:
            assert st.iterations == N_ - 1 and (st.per_sample_iterations == N_ - 1).all()
        print(f"{name} window {P}: {st.iterations} iterations to the fp32 fixed point")
    # order 1: ops.heun_euler stepped over the table
    ts = T.DeterministicSolver(num_steps=N_).t_steps
    t_dev, tl = ts.to(DEV), ts.tolist()
    x = T.ops.scale_f32(x0, tl[0])
    for i in range(N_):
        x = T.ops.heun_euler(x, D(x, t_dev[i:i + 1]), tl[i], tl[i + 1])[1]
    sol = T.ParallelSolver(num_steps=N_, window=5, order=1, rtol=0.0, atol=0.0)
    assert torch.equal(sol.solve(D, x0), x)
    assert sol.last_stats.evaluations == sol.last_stats.iterations + 1 and sol.last_stats.sequential_evaluations == N_


# The Picard allowance: dist(parallel solve at rtol, sequential Heun solve), the worst per-sample RMS in data units,
# of the reference itself (picard_ref, dtype=float32, window 5, order 2, atol = rtol / 10, the seeds of setting()), measured
# on the CPU:
#   gaussian: 1.936e-3 at rtol 1e-2 (6 iterations), 1.612e-4 at 1e-3 (7); mixture: 7.048e-4 at 1e-2 (11), 1.086e-4 at 1e-3 (12)
PICARD_DISTANCE = {("gaussian", 1e-2): 1.936e-3, ("gaussian", 1e-3): 1.612e-4,
                   ("mixture", 1e-2): 7.048e-4, ("mixture", 1e-3): 1.086e-4}
WINDOW = 5


def _f32(D):
    return lambda x, t: D(x.astype(np.float64), t).astype(np.float32)


def _rms(a, b):
    return np.sqrt(((a.double().cpu().numpy() - b.astype(np.float64)) ** 2).reshape(len(b), -1).mean(axis=1))


@pytest.mark.parametrize("rtol", [1e-2, 1e-3])
@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_tolerances_against_the_reference(analytic, name, rtol):
    import tinyedm_amd as T
    x0, x0_np, dens = analytic
    D, D_np = dens[name]
    ts = T.DeterministicSolver(num_steps=N_).t_steps.double().numpy()
    ref = R.solve(_f32(D_np), x0_np, ts, WINDOW, rtol=rtol, atol=rtol / 10, dtype=np.float32)
    seq = R.sequential(_f32(D_np), x0_np, ts, dtype=np.float32)[0]
    sol = T.ParallelSolver(num_steps=N_, window=WINDOW, rtol=rtol, atol=rtol / 10)
    # the strides: the solver's own iteration, driven from here
    st = sol._picard_state(x0.float().contiguous())
    strides, left, seen = [], x0.shape[0], 0
    while left:
        sol._iterate(D, None, st, False, None)
        strides.append(st.stride.cpu().numpy().tolist())
        total = int(st.active.item())
        seen, left = total, total - seen
    assert strides == [s.tolist() for s in ref.strides], (strides, [s.tolist() for s in ref.strides])
    out = sol.solve(D, x0)
    stats = sol.last_stats
    assert stats.iterations == ref.iterations == len(strides) < N_ - 1
    assert stats.per_sample_iterations.tolist() == ref.per_sample_iterations.tolist()
    assert stats.evaluations == ref.evaluations and stats.rows == ref.rows
    e, lim = _rms(out, seq).max(), 2 * PICARD_DISTANCE[name, rtol]
    print(f"{name} rtol {rtol:g}: {stats.iterations} iterations against {N_ - 1}, worst rms distance to the sequential solve "
          f"{e:.3g}, limit {lim:.3g}; the reference's own {_rms(torch.from_numpy(ref.x), seq).max():.3g}")
    record(f"picard/{name}_rtol{rtol:g}_rms_vs_sequential", e, lim)
    assert e <= lim, e


@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_a_sample_alone_gives_the_bits_of_the_batch(analytic, name):
    import tinyedm_amd as T
    x0, _, dens = analytic
    D = dens[name][0]
    sol = T.ParallelSolver(num_steps=N_, window=WINDOW, rtol=1e-2, atol=1e-3)
    batch = sol.solve(D, x0)
    st = sol.last_stats
    for b in (0, 5):
        assert torch.equal(sol.solve(D, x0[b:b + 1].clone()), batch[b:b + 1])
        assert sol.last_stats.per_sample_iterations[0] == st.per_sample_iterations[b]


# ------------------------------------------------------------------ tiny nets vs the reference around the oracle
SCHED = dict(num_steps=6, sigma_min=0.01, sigma_max=20.0, rho=5.0)
RTOL, TINY_WINDOW = 1e-2, 3
# The Picard allowance of the tiny nets: rel(the reference's parallel solve at RTOL, its sequential Heun solve) through the
# fp32 oracle, measured on the CPU (picard_ref, dtype=float32, window 3, atol = RTOL / 10, the seeds of _tiny_case).  On this
# 6-step table no position but the first ever meets E <= 1 (E_1 = 4.5 .. 14.9, E_2 = 13.6 .. 34.3 over the first three
# iterations, unguided and CFG at w = 2): every stride is 1, the solve takes N - 1 = 5 iterations and IS the sequential
# one: the distance is 0 in both cases.
PICARD_TINY_DISTANCE = {"plain": 0.0, "cfg": 0.0}


def reference_solve(guided, bf16):
    """picard_ref around the oracle's forward (host only; also what measured PICARD_TINY_DISTANCE)"""
    import tinyedm_amd as T
    (Pm, em, dm), guide, x0, labels = _tiny_case(guided)
    ts = T.DeterministicSolver(**SCHED).t_steps.double().numpy()
    D = _oracle_callable(_oracle_D(Pm, em, dm, bf16, guide), labels)
    return R.solve(D, x0.numpy(), ts, TINY_WINDOW, rtol=RTOL, atol=RTOL / 10, dtype=np.float32), \
        R.sequential(D, x0.numpy(), ts, dtype=np.float32)[0]


@pytest.mark.parametrize("case", ["f32", "bf16", "cfg_f32", "cfg_bf16"])
def test_tiny_net_vs_reference(ops, case):
    import tinyedm_amd as T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    guided, bf16 = case.startswith("cfg"), case.endswith("bf16")
    dtype = "bf16" if bf16 else "f32"
    (Pm, em, dm), guide, x0, labels = _tiny_case(guided)
    main = _edm(Pm, em, dm, dtype)
    kw = dict(guide=_edm(guide[0], guide[1], guide[2], dtype), guidance=2.0) if guided else {}
    sol = T.ParallelSolver(**SCHED, window=TINY_WINDOW, rtol=RTOL, atol=RTOL / 10, **kw)
    x_hip = sol.solve(main, x0.to(DEV), labels.to(DEV)).cpu()
    st = sol.last_stats
    ref, seq = reference_solve(guided, bf16)
    which = "cfg" if guided else "plain"
    if not bf16:
        d = rel(torch.from_numpy(ref.x), torch.from_numpy(seq))
        record(f"picard/{which}_tiny_distance_parallel_vs_sequential", d, PICARD_TINY_DISTANCE[which])
        assert d <= PICARD_TINY_DISTANCE[which]         # (the recorded allowance is what the reference gives)
    assert st.guide_evaluations == (st.evaluations if guided else 0) and st.evaluations == 2 * st.iterations + 1
    assert st.iterations == ref.iterations and st.per_sample_iterations.tolist() == ref.per_sample_iterations.tolist()
    e = rel(x_hip, torch.from_numpy(ref.x))
    lim = (1e-2 if bf16 else 2e-4) * (3 if guided else 1) + 2 * PICARD_TINY_DISTANCE[which]
    print(f"{case}: gpu {st.per_sample_iterations.tolist()} iterations, reference {ref.per_sample_iterations.tolist()}, "
          f"rel {e:.3g}, limit {lim:.3g}")
    record(f"picard/{case}_vs_reference_around_{'bf16' if bf16 else 'fp32'}_oracle", e, lim)
    assert e <= lim, e
    if guided:
        # the guidance must matter at this size: the unguided solve is far from the guided reference
        x_main = T.ParallelSolver(**SCHED, window=TINY_WINDOW, rtol=RTOL, atol=RTOL / 10).solve(
            main, x0.to(DEV), labels.to(DEV)).cpu()
        assert rel(x_main, torch.from_numpy(ref.x)) > 2 * lim


def test_guidance_one_is_the_unguided_solve(ops):
    import tinyedm_amd as T
    (Pm, em, dm), _, x0, labels = _tiny_case(False)
    main = _edm(Pm, em, dm, "bf16")
    calls = []
    spy = lambda x, s, c: calls.append(1) or main(x, s, c)         # noqa: E731
    kw = dict(**SCHED, window=TINY_WINDOW, rtol=RTOL, atol=RTOL / 10)
    x_g = T.ParallelSolver(**kw, guide=spy, guidance=1.0).solve(main, x0.to(DEV), labels.to(DEV))
    x_u = T.ParallelSolver(**kw).solve(main, x0.to(DEV), labels.to(DEV))
    assert torch.equal(x_g, x_u) and not calls
    # the network is handed the window's rows: P * B of them with their own times, but for the closing step's batch
    seen = []
    spy = lambda x, s, c: seen.append((x.shape[0], tuple(s.shape), c.shape[0])) or main(x, s, c)      # noqa: E731
    sol = T.ParallelSolver(**kw)
    assert torch.equal(sol.solve(spy, x0.to(DEV), labels.to(DEV)), x_u)
    assert seen == [(6, (6,), 6)] * (2 * sol.last_stats.iterations) + [(2, (1,), 2)]
    # the model's own label-free evaluation as the guide
    sol = T.ParallelSolver(**kw, guide="unconditional", guidance=2.0)
    x_c = sol.solve(main, x0.to(DEV), labels.to(DEV))
    assert sol.last_stats.guide_evaluations == sol.last_stats.evaluations
    x_l = T.ParallelSolver(**kw, guide=lambda x, s, c: main(x, s, None), guidance=2.0).solve(main, x0.to(DEV), labels.to(DEV))
    assert torch.equal(x_c, x_l) and not torch.equal(x_c, x_u)


# ------------------------------------------------------------------ the captured iteration
def test_graph_equals_eager(ops, monkeypatch):
    import tinyedm_amd as T
    (Pm, em, dm), guide, x0, labels = _tiny_case(True)
    main = _edm(Pm, em, dm, "f32")
    captures = []
    graph_cls = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda *a, **k: captures.append(1) or graph_cls(*a, **k))
    kw = dict(**SCHED, window=TINY_WINDOW, rtol=RTOL, atol=RTOL / 10)
    sol = T.ParallelSolver(**kw)
    x0, labels = x0.to(DEV), labels.to(DEV)
    eager = sol.solve(main, x0, labels)
    st = sol.last_stats
    graphed = sol.solve(main, x0, labels, graph=True)
    assert torch.equal(graphed, eager) and len(captures) == 1

    def same(a, b):
        return a[:5] == b[:5] and torch.equal(a.per_sample_iterations, b.per_sample_iterations)
    assert same(sol.last_stats, st)
    # another x0 replays the same graph
    x1 = torch.randn(x0.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    assert torch.equal(sol.solve(main, x1, labels, graph=True), sol.solve(main, x1, labels)) and len(captures) == 1
    assert torch.equal(sol.solve(main, x0, labels, graph=True), eager) and len(captures) == 1
    # the tolerances are device state: zero tolerance replays the same graph
    sol.rtol = sol.atol = 0.0
    fixed = sol.solve(main, x0, labels, graph=True)
    assert len(captures) == 1 and torch.equal(fixed, sol.solve(main, x0, labels))
    # a guided solver: the guidance weight is device state too
    g_net = _edm(guide[0], guide[1], guide[2], "f32")
    gsol = T.ParallelSolver(**kw, guide=g_net, guidance=2.0)
    a = gsol.solve(main, x0, labels, graph=True)
    assert torch.equal(a, gsol.solve(main, x0, labels)) and len(captures) == 2
    gsol.guidance = 1.5
    b = gsol.solve(main, x0, labels, graph=True)
    assert len(captures) == 2 and torch.equal(b, gsol.solve(main, x0, labels)) and not torch.equal(a, b)
    # order and window are kernel arguments of the capture: new ones capture anew
    sol.order = 1
    assert torch.equal(sol.solve(main, x0, labels, graph=True), sol.solve(main, x0, labels)) and len(captures) == 3
    ops.check_health(DEV, "graph")


# ------------------------------------------------------------------ end to end
def test_predict_step_with_parallel_solver(ops):
    import tinyedm_amd as T
    (Pm, em, dm), _, x0, labels = _tiny_case(False)
    main = _edm(Pm, em, dm, "bf16")
    sol = T.ParallelSolver(**SCHED, window=TINY_WINDOW, rtol=RTOL, atol=RTOL / 10)
    main.solver = sol
    try:
        with torch.no_grad():
            out = main.predict_step((x0.to(DEV), labels.to(DEV)), 0)
            assert torch.equal(out, sol.solve(main, x0.to(DEV), labels.to(DEV)))
            with pytest.raises(ValueError, match="not implemented for the parallel solver"):
                main.predict_step((x0.to(DEV), labels.to(DEV), x0.to(DEV)), 0)          # an image-conditioned batch
    finally:
        del main.solver
    for kw in ({"start_step": 2}, {"image": x0.to(DEV)}, {"mask": torch.ones(8, 8, device=DEV)},
               {"degradation": T.LinearDegradation(2)}, {"operator": T.GaussianBlur()}, {"dps_scale": 1.0}):
        with pytest.raises(ValueError, match="not implemented for the parallel solver"):
            sol.solve(main, x0.to(DEV), labels.to(DEV), **kw)
    with pytest.raises(ValueError, match="inversion"):
        sol.invert(main, x0.to(DEV), labels.to(DEV))
    with pytest.raises(ValueError, match="likelihood"):
        sol.log_likelihood(main, x0.to(DEV), labels.to(DEV))


def test_generate_cli_picard(ops, tmp_path):
    from PIL import Image
    report = tmp_path / "report.json"
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "generate.py"), "--config_name", "cifar10_cond",
           "--output_dir", str(tmp_path / "out"), "--num_samples", "4", "--batch_size", "2", "--num_steps", "8",
           "--num_classes", "10", "--image_size", "32", "--num_workers", "0", "--network_dtype", "bf16", "--solver", "picard",
           "--window", "4", "--rtol", "1e-2", "--atol", "1e-3", "--solver_report", str(report)]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "out")) == [f"{i}.png" for i in range(4)]
    for i in range(4):
        assert Image.open(tmp_path / "out" / f"{i}.png").size == (32, 32)
    rep = json.loads(report.read_text())
    assert len(rep["per_sample_iterations"]) == rep["num_images"] == 4 and len(rep["iterations"]) == 2
    assert rep["evaluations"] <= rep["sequential_evaluations"] == 2 * (2 * 7 + 1)
    assert rep["evaluations"] == sum(2 * i + 1 for i in rep["iterations"]) and rep["guide_evaluations"] == 0
    assert rep["rows"] == sum(2 * i * 4 * 2 + 2 for i in rep["iterations"])
    assert (rep["window"], rep["order"], rep["rtol"], rep["atol"]) == (4, 2, 1e-2, 1e-3)
    for i, b in zip(rep["iterations"], (slice(0, 2), slice(2, 4))):
        assert i == max(rep["per_sample_iterations"][b]) <= 7
