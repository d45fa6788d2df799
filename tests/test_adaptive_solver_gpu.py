"""The adaptive solver on the GPU (AdaptiveSolver, ops.adapt_*, csrc/adaptive.hip):

 * adapt_euler / adapt_correct with every sample at (t_5, t_6) of the 18-step table against heun_euler / heun_correct,
   bit for bit, on the dwordx4 path, the scalar tail and misaligned operands; per-sample times against single-sample
   calls; inactive samples ride along; a NaN raises the health bit;
 * the error partials and E against fp64 from the same fp32 operands, under a bound derived from the rounding count;
   E is bit-identical whatever the batch;
 * adapt_control against the controller of tests/adaptive_ref.py on hand-made rows; adapt_commit on both memory paths;
 * the solver on the two analytic denoisers of tests/test_adaptive_solver_cpu.py, as GPU callables with fp32 state;
 * tiny nets against adaptive_ref run around the oracle's forward, "f32" and bf16, unguided and CFG at w = 2;
 * the generate CLI, EDM.predict_step and the refusals end to end."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adaptive_ref as R
from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs
from parity_log import record
from test_adaptive_solver_cpu import B_, D_, MIX_S, MIX_W, SPAN, gaussian_exact, setting
from test_multistep_solver_gpu import _edm, _oracle_D, rel

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
SHAPES = [(7, 3 * 32 * 32, 0), (3, 4099, 0), (3, 4099, 1), (1, 5, 0), (2, 1024, 1)]
SHAPE_IDS = ["7x3072", "3x4099-tail", "3x4099-misaligned", "1x5", "2x1024-misaligned"]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def _operand(B, CHW, offset, g, scale=1.0):
    """contiguous fp32 [B, CHW] on the GPU; offset 1: it starts one float past a 16-byte boundary"""
    flat = (scale * torch.randn(B * CHW + 1, generator=g)).to(DEV)
    t = flat[offset:offset + B * CHW].view(B, CHW)
    assert t.is_contiguous() and (t.data_ptr() % 16 == 0) == (offset == 0)
    return t


def _table_pair():
    import tinyedm_amd as T
    ts = T.DeterministicSolver(num_steps=18).t_steps.tolist()
    return ts[5], ts[6]


def _times(B, t0, t1):
    return torch.full((B,), t0, device=DEV), torch.full((B,), t1, device=DEV)


# ------------------------------------------------------------------ kernel bits
@pytest.mark.parametrize("B,CHW,offset", SHAPES, ids=SHAPE_IDS)
def test_euler_and_correct_equal_the_heun_kernels(ops, B, CHW, offset):
    g = torch.Generator().manual_seed(B * CHW + offset)
    x, D, D1 = (_operand(B, CHW, offset, g) for _ in range(3))
    t0, t1 = _table_pair()
    t, tn = _times(B, t0, t1)
    dx, x1 = ops.adapt_euler(x, D, t, tn)
    dx_h, x1_h = ops.heun_euler(x, D, t0, t1)
    assert torch.equal(dx, dx_h) and torch.equal(x1, x1_h)
    y, _ = ops.adapt_correct(x, dx, x1, D1, t, tn, 1e-4, 1e-3)
    assert torch.equal(y, ops.heun_correct(x, dx, x1, D1, t0, t1))
    # upwards (invert's direction) as well
    t, tn = _times(B, t1, t0)
    dx, x1 = ops.adapt_euler(x, D, t, tn)
    dx_h, x1_h = ops.heun_euler(x, D, t1, t0)
    assert torch.equal(dx, dx_h) and torch.equal(x1, x1_h)
    y, _ = ops.adapt_correct(x, dx, x1, D1, t, tn, 1e-4, 1e-3)
    assert torch.equal(y, ops.heun_correct(x, dx, x1, D1, t1, t0))
    ops.check_health(x.device, "adapt_euler / adapt_correct")


@pytest.mark.parametrize("B,CHW,offset", [(5, 3 * 8 * 8, 0), (3, 4099, 0)], ids=["5x192", "3x4099"])
def test_per_sample_times_equal_single_sample_calls(ops, B, CHW, offset):
    import tinyedm_amd as T
    g = torch.Generator().manual_seed(17)
    x, D, D1 = (_operand(B, CHW, offset, g) for _ in range(3))
    ts = T.DeterministicSolver(num_steps=18).t_steps
    t, tn = ts[2:2 + B].contiguous().to(DEV), ts[3:3 + B].contiguous().to(DEV)
    dx, x1 = ops.adapt_euler(x, D, t, tn)
    y, part = ops.adapt_correct(x, dx, x1, D1, t, tn, 1e-4, 1e-3)
    n = ops.adapt_chunks(CHW)
    for b in range(B):
        s = slice(b, b + 1)
        dx_b, x1_b = ops.adapt_euler(x[s].clone(), D[s].clone(), t[s].clone(), tn[s].clone())
        assert torch.equal(dx_b, dx[s]) and torch.equal(x1_b, x1[s])
        assert torch.equal(x1_b, ops.heun_euler(x[s].clone(), D[s].clone(), t[b].item(), tn[b].item())[1])
        y_b, part_b = ops.adapt_correct(x[s].clone(), dx_b, x1_b, D1[s].clone(), t[s].clone(), tn[s].clone(), 1e-4, 1e-3)
        assert torch.equal(y_b, y[s]) and torch.equal(part_b[0, :n], part[b, :n])


def test_inactive_samples_ride_along(ops):
    g = torch.Generator().manual_seed(3)
    B, CHW = 3, 1028
    x, D, D1 = (_operand(B, CHW, 0, g) for _ in range(3))
    t0, t1 = _table_pair()
    t, tn = _times(B, t0, t1)
    tn[1] = t[1]                                    # sample 1 is not active
    D[1, 7] = float("nan")
    D1[1, 1027] = float("inf")
    ops.check_health(x.device, "before")
    dx, x1 = ops.adapt_euler(x, D, t, tn)
    assert torch.equal(x1[1], x[1]) and not dx[1].any()
    y, part = ops.adapt_correct(x, dx, x1, D1, t, tn, 1e-4, 1e-3)
    assert torch.equal(y[1], x[1]) and not part[1, :ops.adapt_chunks(CHW)].any()
    ops.check_health(x.device, "an inactive sample's D must not matter")
    for b in (0, 2):
        assert torch.equal(x1[b], ops.heun_euler(x[b], D[b], t0, t1)[1])
        assert torch.equal(y[b], ops.heun_correct(x[b], dx[b], x1[b], D1[b], t0, t1))


def test_nonfinite_d_sets_health(ops):
    g = torch.Generator().manual_seed(5)
    B, CHW = 2, 4099
    x, D, D1 = (_operand(B, CHW, 0, g) for _ in range(3))
    t, tn = _times(B, *_table_pair())
    ops.check_health(x.device, "before")
    D[1, 4097] = float("nan")                       # in the scalar tail of the last quad
    dx, x1 = ops.adapt_euler(x, D, t, tn)
    with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
        ops.check_health(x.device, "adapt_euler")
    D1[0, 17] = float("inf")
    ops.adapt_correct(x, dx.nan_to_num(), x1.nan_to_num(), D1, t, tn, 1e-4, 1e-3)
    with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
        ops.check_health(x.device, "adapt_correct")
    ops.check_health(x.device, "after")             # the read cleared the word


# ------------------------------------------------------------------ error partials and E
def _begin(ops, B, t0, t1):
    """a device state with every sample active at (t0, t1)"""
    state = ops.adapt_begin(B, t0, 0.5 * min(t0, t1) if t1 < t0 else 2.0 * max(t0, t1), t1 - t0, DEV)
    rows = ops.adapt_rows(state)
    rows.t1.fill_(t1)
    return state, rows


@pytest.mark.parametrize("B,CHW,offset", SHAPES, ids=SHAPE_IDS)
def test_error_norm_vs_fp64(ops, B, CHW, offset):
    g = torch.Generator().manual_seed(11 + B * CHW + offset)
    t0, t1 = _table_pair()
    atol, rtol = 1e-4, 1e-3
    x = _operand(B, CHW, offset, g, scale=t0)       # a state at noise level t0
    D, D1 = (_operand(B, CHW, offset, g, scale=0.5) for _ in range(2))
    state, rows = _begin(ops, B, t0, t1)
    dx, x1 = ops.adapt_euler(x, D, rows.t, rows.t1)
    y, part = ops.adapt_correct(x, dx, x1, D1, rows.t, rows.t1, atol, rtol)
    active = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.adapt_control(part, CHW, state, 0.5 * t1, active)
    E = rows.err.double().cpu().numpy()
    n = ops.adapt_chunks(CHW)
    X, DX, X1, DD1, Y = (v.double().cpu().numpy() for v in (x, dx, x1, D1, y))
    # (1) the partials are the fp64 sum over the kernel's own fp32 y: every term is computed in fp64 (a handful of
    # roundings of 2^-53 each) and CHW <= 4099 positive terms are added in a fixed order: relative error < 1e-11
    q = (Y - X1) / (atol + rtol * np.maximum(np.abs(X), np.abs(Y)))
    s_ref = (q * q).sum(axis=1)
    s = part[:, :n].sum(dim=1).cpu().numpy()
    assert np.all(np.abs(s - s_ref) <= 1e-11 * s_ref), np.abs(s / s_ref - 1).max()
    # (2) E against fp64 from the same fp32 operands (x, dx, x1, D1, t0, t1).  The kernel's y = fma(dt, s, x) with
    # dp = (x1 - D1) / t1 (2 roundings, each <= eps A with A = (|x1| + |D1|) / |t1|), s = fma(0.5, dx, 0.5 dp) (1 rounding,
    # <= eps S with S = |dx| / 2 + A / 2), dt = t1 - t0 (1 rounding, eps |dt|) and the final rounding eps |y|:
    #   |y - y64| <= eps (|x| + |dt| (A + 3 S)) <= 5 eps (|x| + |dt| S) =: 5 eps mag      (A <= 2 S),
    # taken as 6 eps mag for the second-order terms.  A term q = (y - x1) / sc moves by at most dq = dy / sc (1 + rtol |q|)
    # (sc depends on |y| too), and E is an RMS, so by the triangle inequality |E - E64| <= sqrt(mean dq^2); the device
    # stores E as fp32 (one more rounding, 2^-24 E).
    dt = t1 - t0
    A = (np.abs(X1) + np.abs(DD1)) / abs(t1)
    S = 0.5 * np.abs(DX) + 0.5 * A
    Y64 = X + dt * (0.5 * DX + 0.5 * (X1 - DD1) / t1)
    E64 = R.error_norm(X, X1, Y64, atol, rtol)
    sc = atol + rtol * np.maximum(np.abs(X), np.abs(Y64))
    q64 = (Y64 - X1) / sc
    dq = 6 * EPS32 * (np.abs(X) + abs(dt) * S) / sc * (1 + rtol * np.abs(q64))
    bound = np.sqrt((dq * dq).mean(axis=1)) + 2 * EPS32 * E64
    print(f"E {E64}, |E - E64| {np.abs(E - E64)}, bound {bound}")
    assert np.all(np.abs(E - E64) <= bound), (np.abs(E - E64) / bound).max()
    assert np.all(bound <= 0.05 * E64)              # (the bound is a statement about E, not a blank cheque)


def test_error_norm_does_not_depend_on_the_batch(ops):
    g = torch.Generator().manual_seed(23)
    t0, t1 = _table_pair()
    for CHW in (3 * 32 * 32, 4099):
        x = _operand(7, CHW, 0, g, scale=t0)
        D, D1 = (_operand(7, CHW, 0, g, scale=0.5) for _ in range(2))
        out = []
        for rows_of in (slice(0, 7), slice(6, 7)):
            xs, Ds, D1s = (v[rows_of].clone() for v in (x, D, D1))
            state, rows = _begin(ops, xs.shape[0], t0, t1)
            dx, x1 = ops.adapt_euler(xs, Ds, rows.t, rows.t1)
            y, part = ops.adapt_correct(xs, dx, x1, D1s, rows.t, rows.t1, 1e-4, 1e-3)
            ops.adapt_control(part, CHW, state, 0.5 * t1, torch.zeros(1, dtype=torch.int32, device=DEV))
            out.append((part[-1, :ops.adapt_chunks(CHW)].clone(), rows.err[-1].clone(), rows.h[-1].clone()))
        for a, b in zip(*out):
            assert torch.equal(a, b)
        # and a misaligned copy of the sample (the scalar path at CHW % 4 == 0) gives the same partials
        if CHW % 4 == 0:
            xm, Dm, D1m = (torch.cat([v.new_zeros(1), v[6]])[1:].view(1, CHW) for v in (x, D, D1))
            assert xm.data_ptr() % 16 != 0
            state, rows = _begin(ops, 1, t0, t1)
            dx, x1 = ops.adapt_euler(xm, Dm, rows.t, rows.t1)
            _, part = ops.adapt_correct(xm, dx, x1, D1m, rows.t, rows.t1, 1e-4, 1e-3)
            assert torch.equal(part[0, :ops.adapt_chunks(CHW)], out[0][0])


# ------------------------------------------------------------------ the controller
def _ulp_equal(a, b):
    a, b = np.float32(a), np.float32(b)
    return a == b or abs(np.float64(a) - np.float64(b)) <= np.spacing(np.abs(b))


def test_control_against_the_reference(ops):
    CHW, t_end, f32 = 48, 0.1, np.float32
    c = R.Controller()
    cases = [                                               # (row before, E)
        (R.Row(f32(1.0), f32(0.8), f32(-0.2)), 0.25),                               # well under 1
        (R.Row(f32(1.0), f32(0.8), f32(-0.2)), 1e-6),                               # growth capped at fac_max, then a snap
        (R.Row(f32(1.0), f32(0.8), f32(-0.2)), 4.0),                                # well over 1
        (R.Row(f32(1.0), f32(0.8), f32(-0.2)), 1.0),                                # exactly 1 accepts
        (R.Row(f32(1.0), f32(0.8), f32(-0.2)), float("nan")),                       # NaN rejects, at fac_min
        (R.Row(f32(1.0), f32(0.91), f32(-0.09), after_reject=True, rejected=1), 0.01),      # the step after a rejection
        (R.Row(f32(0.3), f32(0.1), f32(-0.2), accepted=7), 0.5),                    # a snapped step arrives: done
        (R.Row(f32(0.3), f32(0.15), f32(-0.15)), 0.81),                             # the next step snaps (passes t_end)
        (R.Row(f32(0.1), f32(0.1), f32(-0.05), status=R.DONE, accepted=9, rejected=2, err=f32(0.5)), 123.0),   # already done
        (R.Row(f32(1.0), f32(1.0) - f32(2e-6), f32(-2e-6)), 100.0),                 # under the floor: failed
    ]
    B = len(cases)
    f = np.zeros((ops.ADAPT_ROWS, B), dtype=np.float32)
    u = f.view(np.int32)
    for b, (r, _) in enumerate(cases):
        f[0, b], f[1, b], f[2, b], f[3, b] = r.t, r.t1, r.h, r.err
        u[4, b], u[5, b], u[6, b], u[7, b] = r.status, r.accepted, r.rejected, int(r.after_reject)
    state = torch.from_numpy(u.copy()).to(DEV)
    part = torch.full((B, ops.NLL_MAX_CHUNKS), float("nan"), dtype=torch.float64, device=DEV)     # (only chunk 0 is read)
    part[:, 0] = torch.tensor([E * E * CHW for _, E in cases], dtype=torch.float64)
    active = torch.full((1,), 100, dtype=torch.int32, device=DEV)
    ops.check_health(DEV, "before")
    accept = ops.adapt_control(part, CHW, state, t_end, active, safety=c.safety, fac_min=c.fac_min, fac_max=c.fac_max,
                               h_floor=c.h_floor).cpu().numpy()
    with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
        ops.check_health(DEV, "the failed row raises the health bit")
    got = state.cpu().numpy()
    gf = got.view(np.float32)
    still = 0
    for b, (row, E) in enumerate(cases):
        E_dev = np.sqrt(np.float64(E * E * CHW) / CHW)
        ok, ref = R.control(row, E_dev, t_end, c, dtype=np.float32)
        assert bool(accept[b]) == ok, b
        assert (got[4, b], got[5, b], got[6, b], got[7, b]) == (ref.status, ref.accepted, ref.rejected, int(ref.after_reject)), b
        for k, v in ((0, ref.t), (1, ref.t1), (2, ref.h)):
            assert _ulp_equal(gf[k, b], v), (b, k, gf[k, b], v)
        if row.status == R.ACTIVE:
            assert np.isnan(gf[3, b]) if math.isnan(E) else _ulp_equal(gf[3, b], np.float32(E_dev))
        else:
            assert gf[3, b] == row.err and gf[2, b] == row.h
        still += ref.status == R.ACTIVE
    assert [bool(a) for a in accept] == [True, True, False, True, False, True, True, True, False, False]
    assert got[4].tolist() == [0, 0, 0, 0, 0, 0, R.DONE, 0, R.DONE, R.FAILED]
    assert gf[1, 1] == np.float32(t_end) and gf[1, 7] == np.float32(t_end)         # the snaps land exactly
    assert int(active.item()) == 100 + still == 107


@pytest.mark.parametrize("B,CHW,offset", SHAPES, ids=SHAPE_IDS)
def test_commit(ops, B, CHW, offset):
    g = torch.Generator().manual_seed(29)
    x, y = (_operand(B, CHW, offset, g) for _ in range(2))
    keep = x.clone()
    accept = (torch.arange(B) % 2 == 0).to(torch.uint8).to(DEV)
    out = ops.adapt_commit(x, y, accept)
    assert out.data_ptr() == x.data_ptr()
    for b in range(B):
        assert torch.equal(x[b], y[b] if b % 2 == 0 else keep[b])
    with pytest.raises(ValueError):
        ops.adapt_commit(x, x, accept)
    with pytest.raises(ValueError):
        ops.adapt_commit(x, y, accept[:-1] if B > 1 else accept.int())


# ------------------------------------------------------------------ the solver on analytic denoisers
def _gaussian_gpu(x, s, labels=None):
    s = s.double().reshape(-1, *([1] * (x.dim() - 1)))
    return (0.25 / (0.25 + s * s) * x.double()).float()


def _mixture_gpu(means):
    means = torch.from_numpy(means).to(DEV)
    logw = torch.tensor(MIX_W, dtype=torch.float64, device=DEV).log()

    def D(x, s, labels=None):
        v = MIX_S ** 2 + s.double().reshape(-1, 1) ** 2
        d = x.double()[:, None, :] - means[None]
        logp = logw[None] - 0.5 * (d * d).sum(-1) / v - 0.5 * means.shape[1] * v.log()
        p = torch.softmax(logp, dim=1)
        return (p[:, :, None] * (means[None] + (MIX_S ** 2 / v)[:, :, None] * d)).sum(1).float()
    return D


def _rowwise(D):
    """D evaluated one sample at a time: a callable whose rows cannot depend on each other, whatever torch's reductions do"""
    def run(x, s, labels=None):
        s = s.reshape(-1).expand(x.shape[0])
        return torch.cat([D(x[b:b + 1], s[b:b + 1]) for b in range(x.shape[0])])
    return run


@pytest.fixture(scope="module")
def analytic(ops, golden_dir):
    means, x0 = setting()
    truth = np.load(os.path.join(golden_dir, "adaptive_mixture_truth.npz"))
    assert np.array_equal(truth["span"], np.array(SPAN))
    return torch.from_numpy(x0).float().to(DEV), means, \
        {"gaussian": (_gaussian_gpu, gaussian_exact(x0)), "mixture": (_mixture_gpu(means), truth["truth"])}


def _rms(a, b):
    return np.sqrt(((a.double().cpu().numpy() - b) ** 2).reshape(len(b), -1).mean(axis=1))


@pytest.mark.parametrize("rtol", [1e-2, 1e-3])
@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_solver_on_analytic_denoisers(analytic, name, rtol):
    import tinyedm_amd as T
    x0, means, dens = analytic
    D, ref = dens[name]
    sol = T.AdaptiveSolver(rtol=rtol, atol=rtol / 10)
    assert sol.span() == SPAN
    out = sol.solve(D, x0)
    st = sol.last_stats
    assert out.shape == x0.shape and out.dtype == x0.dtype
    assert st.accepted.shape == (B_,) and not st.accepted.is_cuda and (st.accepted > 0).all()
    assert st.iterations == int((st.accepted + st.rejected).max()) <= 1024
    assert st.evaluations == 2 * st.iterations + 1 and st.guide_evaluations == 0
    e = _rms(out, ref).max()
    print(f"{name} rtol {rtol:g}: {st.iterations} iterations, worst rms error {e:.3g} = {e / rtol:.2f} rtol; rejected "
          f"{int(st.rejected.sum())} of {int((st.accepted + st.rejected).sum())}")
    record(f"adaptive/{name}_rtol{rtol:g}_rms_vs_truth", e, 4 * rtol)
    assert e <= 4 * rtol, e
    if name == "mixture":
        assert len(set(st.accepted.tolist())) > 1
    # invert, then solve: the image comes back
    g = np.random.default_rng(1)
    img = 0.5 * g.standard_normal((B_, D_)) if name == "gaussian" else \
        means[g.integers(0, 4, B_)] + MIX_S * g.standard_normal((B_, D_))
    lat = sol.invert(D, torch.from_numpy(img).float().to(DEV))
    up = sol.last_stats
    assert up.evaluations == 2 * up.iterations and up.iterations == int((up.accepted + up.rejected).max())
    e = _rms(sol.solve(D, lat), img).max()
    record(f"adaptive/{name}_rtol{rtol:g}_round_trip", e, 8 * rtol)
    assert e <= 8 * rtol, e


@pytest.mark.parametrize("name", ["gaussian", "mixture"])
def test_a_sample_alone_gives_the_bits_of_the_batch(analytic, name):
    import tinyedm_amd as T
    x0, _, dens = analytic
    D = _rowwise(dens[name][0])
    sol = T.AdaptiveSolver(rtol=1e-2, atol=1e-3)
    batch = sol.solve(D, x0)
    st = sol.last_stats
    for b in (0, 5):
        assert torch.equal(sol.solve(D, x0[b:b + 1].clone()), batch[b:b + 1])
        assert (sol.last_stats.accepted[0], sol.last_stats.rejected[0]) == (st.accepted[b], st.rejected[b])


def test_solver_reports_what_did_not_finish(analytic):
    import tinyedm_amd as T
    x0, _, dens = analytic
    with pytest.raises(RuntimeError, match=r"8 of 8 samples are still active after max_iterations = 3, at t = \["):
        T.AdaptiveSolver(max_iterations=3).solve(dens["gaussian"][0], x0)
    ops_ = T.ops
    ops_.check_health(x0.device, "a solve that ran out of iterations leaves the health word alone")

    def broken(x, s, labels=None):          # sample 2's denoiser is NaN: its every step is rejected until h hits the floor
        D = dens["gaussian"][0](x, s)
        D[2] = float("nan")
        return D
    with pytest.raises(RuntimeError, match=r"the step of 1 of 8 samples fell under h_floor"):
        T.AdaptiveSolver().solve(broken, x0)
    ops_.check_health(x0.device, "the failure was reported; the word is clear again")


# ------------------------------------------------------------------ tiny nets vs the reference around the oracle
SCHED = dict(num_steps=6, sigma_min=0.01, sigma_max=20.0, rho=5.0)
RTOL = 1e-2
# ODE allowance: accept decisions may differ near E = 1 between the GPU and the reference, which moves the result by no
# more than the solve's own truncation error.  It is taken as twice rel(reference at rtol, reference at rtol / 100) on the
# same net through the fp32 oracle, measured on the CPU (adaptive_ref, dtype=float32, the seeds below):
#   unguided 4.03e-3 (57 iterations at rtol, 316 at rtol / 100), CFG at w = 2 2.24e-3 (73 and 504 iterations)
ODE_DISTANCE = {"plain": 4.03e-3, "cfg": 2.24e-3}


def _oracle_callable(D, labels):
    def run(x, t):
        with torch.no_grad():
            return D(torch.from_numpy(np.asarray(x, dtype=np.float32)), torch.from_numpy(np.asarray(t, dtype=np.float32)),
                     labels).double().numpy()
    return run


def _tiny_case(guided):
    em, dm = tiny_cfgs(10)
    Pm = O.init_params(em, dm, torch.Generator().manual_seed(7))
    guide = None
    if guided:
        eg, dg = tiny_cfgs(None)
        guide = (O.init_params(eg, dg, torch.Generator().manual_seed(11)), eg, dg, 2.0)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 3, 8, 8, generator=g)
    labels = torch.randint(0, 10, (2,), generator=g)
    return (Pm, em, dm), guide, x0, labels


def reference_solve(guided, bf16, rtol):
    """adaptive_ref around the oracle's forward (host only; also what measured ODE_DISTANCE)"""
    import tinyedm_amd as T
    (Pm, em, dm), guide, x0, labels = _tiny_case(guided)
    span = T.AdaptiveSolver(**SCHED).span()
    return R.solve(_oracle_callable(_oracle_D(Pm, em, dm, bf16, guide), labels), x0.numpy(), span, rtol=rtol, atol=rtol / 10,
                   dtype=np.float32)


@pytest.mark.parametrize("case", ["f32", "bf16", "cfg_f32", "cfg_bf16"])
def test_tiny_net_vs_reference(ops, case):
    import tinyedm_amd as T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    guided, bf16 = case.startswith("cfg"), case.endswith("bf16")
    dtype = "bf16" if bf16 else "f32"
    (Pm, em, dm), guide, x0, labels = _tiny_case(guided)
    main = _edm(Pm, em, dm, dtype)
    kw = dict(guide=_edm(guide[0], guide[1], guide[2], dtype), guidance=2.0) if guided else {}
    sol = T.AdaptiveSolver(**SCHED, rtol=RTOL, atol=RTOL / 10, **kw)
    x_hip = sol.solve(main, x0.to(DEV), labels.to(DEV)).cpu()
    st = sol.last_stats
    ref = reference_solve(guided, bf16, RTOL)
    assert (ref.status == R.DONE).all()
    assert st.guide_evaluations == (st.evaluations if guided else 0) and st.evaluations == 2 * st.iterations + 1
    e = rel(x_hip, torch.from_numpy(ref.x))
    lim = (1e-2 if bf16 else 2e-4) * (3 if guided else 1) + 2 * ODE_DISTANCE["cfg" if guided else "plain"]
    print(f"{case}: gpu {st.accepted.tolist()} + {st.rejected.tolist()}, reference {ref.accepted.tolist()} + "
          f"{ref.rejected.tolist()}, rel {e:.3g}, limit {lim:.3g}")
    record(f"adaptive/{case}_vs_reference_around_{'bf16' if bf16 else 'fp32'}_oracle", e, lim)
    record(f"adaptive/{'cfg' if guided else 'plain'}_ode_distance_rtol_vs_rtol_over_100", ODE_DISTANCE["cfg" if guided else "plain"],
           ODE_DISTANCE["cfg" if guided else "plain"])
    assert e <= lim, e
    if guided:
        # the guidance must matter at this size: the unguided solve is far from the guided reference
        x_main = T.AdaptiveSolver(**SCHED, rtol=RTOL, atol=RTOL / 10).solve(main, x0.to(DEV), labels.to(DEV)).cpu()
        assert rel(x_main, torch.from_numpy(ref.x)) > 2 * lim


def test_guidance_one_is_the_unguided_solve(ops):
    import tinyedm_amd as T
    (Pm, em, dm), _, x0, labels = _tiny_case(False)
    main = _edm(Pm, em, dm, "bf16")
    calls = []
    spy = lambda x, s, c: calls.append(1) or main(x, s, c)         # noqa: E731
    kw = dict(**SCHED, rtol=RTOL, atol=RTOL / 10)
    x_g = T.AdaptiveSolver(**kw, guide=spy, guidance=1.0).solve(main, x0.to(DEV), labels.to(DEV))
    x_u = T.AdaptiveSolver(**kw).solve(main, x0.to(DEV), labels.to(DEV))
    assert torch.equal(x_g, x_u) and not calls
    # the network is handed the per-sample times: [B] tensors, but for the closing step's single sigma_min
    seen = []
    spy = lambda x, s, c: seen.append(tuple(s.shape)) or main(x, s, c)      # noqa: E731
    sol = T.AdaptiveSolver(**kw)
    assert torch.equal(sol.solve(spy, x0.to(DEV), labels.to(DEV)), x_u)
    assert seen == [(2,)] * (2 * sol.last_stats.iterations) + [(1,)]


def test_unconditional_guide_is_the_models_label_free_evaluation(ops):
    import tinyedm_amd as T
    (Pm, em, dm), _, x0, labels = _tiny_case(False)
    main = _edm(Pm, em, dm, "bf16")
    kw = dict(**SCHED, rtol=RTOL, atol=RTOL / 10, guidance=2.0)
    sol = T.AdaptiveSolver(**kw, guide="unconditional")
    x_u = sol.solve(main, x0.to(DEV), labels.to(DEV))
    assert sol.last_stats.guide_evaluations == sol.last_stats.evaluations
    x_g = T.AdaptiveSolver(**kw, guide=lambda x, s, c: main(x, s, None)).solve(main, x0.to(DEV), labels.to(DEV))
    assert torch.equal(x_u, x_g)
    assert not torch.equal(x_u, T.AdaptiveSolver(**SCHED, rtol=RTOL, atol=RTOL / 10).solve(main, x0.to(DEV), labels.to(DEV)))
    with pytest.raises(ValueError, match="needs class_labels"):
        sol.solve(main, x0.to(DEV))


# ------------------------------------------------------------------ end to end
def test_predict_step_with_adaptive_solver(ops):
    import tinyedm_amd as T
    (Pm, em, dm), _, x0, labels = _tiny_case(False)
    main = _edm(Pm, em, dm, "bf16")
    sol = T.AdaptiveSolver(**SCHED, rtol=RTOL, atol=RTOL / 10)
    main.solver = sol
    try:
        with torch.no_grad():
            out = main.predict_step((x0.to(DEV), labels.to(DEV)), 0)
            assert torch.equal(out, sol.solve(main, x0.to(DEV), labels.to(DEV)))
            with pytest.raises(ValueError, match="not implemented for the adaptive solver"):
                main.predict_step((x0.to(DEV), labels.to(DEV), x0.to(DEV)), 0)          # an image-conditioned batch
    finally:
        del main.solver
    for kw in ({"graph": True}, {"start_step": 2}, {"image": x0.to(DEV)}, {"mask": torch.ones(8, 8, device=DEV)},
               {"degradation": T.LinearDegradation(2)}, {"operator": T.GaussianBlur()}, {"dps_scale": 1.0}):
        with pytest.raises(ValueError, match="not implemented for the adaptive solver"):
            sol.solve(main, x0.to(DEV), labels.to(DEV), **kw)
    with pytest.raises(ValueError, match="not implemented for the adaptive solver"):
        sol.invert(main, x0.to(DEV), labels.to(DEV), end_step=1)
    with pytest.raises(ValueError, match="likelihood"):
        sol.log_likelihood(main, x0.to(DEV), labels.to(DEV))
    with pytest.raises(ValueError, match="guidance_interval"):
        T.AdaptiveSolver(**SCHED, guide=main, guidance=2.0, guidance_interval=(0.1, 5.0))


def test_generate_cli_adaptive(ops, tmp_path):
    from PIL import Image
    report = tmp_path / "report.json"
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "generate.py"), "--config_name", "cifar10_cond",
           "--output_dir", str(tmp_path / "out"), "--num_samples", "4", "--batch_size", "2", "--num_steps", "8",
           "--num_classes", "10", "--image_size", "32", "--num_workers", "0", "--network_dtype", "bf16", "--solver", "adaptive",
           "--rtol", "1e-2", "--atol", "1e-3", "--max_iterations", "500", "--solver_report", str(report)]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "out")) == [f"{i}.png" for i in range(4)]
    for i in range(4):
        assert Image.open(tmp_path / "out" / f"{i}.png").size == (32, 32)
    rep = json.loads(report.read_text())
    assert len(rep["accepted"]) == len(rep["rejected"]) == rep["num_images"] == 4 and len(rep["iterations"]) == 2
    assert all(a > 0 for a in rep["accepted"])
    assert rep["accepted_total"] == sum(rep["accepted"]) and rep["rejected_total"] == sum(rep["rejected"])
    assert rep["evaluations"] == sum(2 * i + 1 for i in rep["iterations"]) and rep["guide_evaluations"] == 0
    assert (rep["rtol"], rep["atol"], rep["max_iterations"]) == (1e-2, 1e-3, 500)
    for i, b in zip(rep["iterations"], (slice(0, 2), slice(2, 4))):
        assert i == max(a + r_ for a, r_ in zip(rep["accepted"][b], rep["rejected"][b]))
    # --invert_to with the adaptive solver: the images just written, run upwards to sigma_max
    up = tmp_path / "up.json"
    i0 = cmd.index("--output_dir") + 1
    cmd2 = cmd[:i0] + [str(tmp_path / "unused")] + cmd[i0 + 1:-1] + [str(up), "--init_dir", str(tmp_path / "out"),
                                                                    "--invert_to", str(tmp_path / "latents.pt")]
    r = subprocess.run(cmd2, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lat = torch.load(tmp_path / "latents.pt")
    assert lat["latents"].shape == (4, 3, 32, 32) and lat["end_step"] == 0 and bool(torch.isfinite(lat["latents"]).all())
    rep = json.loads(up.read_text())
    assert rep["num_images"] == 4 and rep["evaluations"] == sum(2 * i for i in rep["iterations"])
