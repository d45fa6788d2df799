"""Guarded optimizer step on the GPU (csrc/grad_guard.hip, FusedAdam.set_guard, Trainer(gradient_clip_val=,
skip_nonfinite_steps=)) against tests/grad_guard_ref.py, against the unguarded kernels, and at the step level.

The arena of the kernel tests: tensors of 1, 3, 64, 65, 4097 and 70 001 elements at 64-element-aligned offsets (FlatArena's
rule), once as allocated and once as a view that starts one element in, so that its base is not 16-byte aligned.

Limits.
* sums of squares: every fp32 * fp32 product is exact in fp64 and all terms are >= 0, so the kernel and the reference
  (math.fsum) differ by the rounding of each square (2^-53) and by the order of the additions ((n - 1) * 2^-53 at the
  most): n * 2^-52 relative for n summed elements, per tensor and in total.
* norm and coef: one fp64 square root / division of such a sum, rounded to fp32: 1 fp32 ulp.
* guarded Adam against ops.adam_ema called with the scale fp32(grad_scale) * fp32(coef): two kernels evaluating the same
  fp32 expressions on the same operands: 2 ulp on the conditioned state, and on the any-sign state a largest error
  against fp64 of at most twice the unguarded kernel's (both derived in tests/test_fused_opt_gpu.py).
* the sums do not depend on the chunk length of the table: they are taken over 1024-element blocks counted from each
  tensor's start, so tables with different chunk lengths must give the same bits."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import grad_guard_ref as G
from parity_log import record
from test_fused_opt_gpu import (B1, B2, EMA_BETA, EPS, GRAD_SCALE, LR, STEP, _batches, random_state, random_theta,
                                step_record, ulps)

DEV = "cuda"
NUMELS = [1, 3, 64, 65, 4097, 70001]
SCALES = [1e-20, 1e-12, 1e-3, 1.0, 1e9, 1e18]      # an fp32 sum of squares would flush (1e-40) or overflow (7e40)
OFFSETS, N = [], 0
for _c in NUMELS:
    OFFSETS.append(N)
    N += (_c + 63) // 64 * 64
PAD_VALUE = 1.0e30                                  # what the padding holds: reading it would show in every sum


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def host_arena():
    """the fp32 arena on the host (never modified: tests that plant values copy it)"""
    g = torch.Generator().manual_seed(1234)
    a = torch.full((N,), PAD_VALUE, dtype=torch.float32)
    for o, c, s in zip(OFFSETS, NUMELS, SCALES):
        a[o:o + c] = (torch.randn(c, generator=g, dtype=torch.float64) * s).float()
    a.requires_grad_(False)
    return a


@pytest.fixture(scope="module")
def reference(host_arena):
    """per-tensor and total fp64 sums of squares of the arena at GRAD_SCALE, computed once"""
    per, total = G.sumsq(host_arena.numpy(), OFFSETS, NUMELS, GRAD_SCALE)
    return per, total


def on_device(host, shift):
    """the arena on the GPU; shift = 1: a view one element into its buffer (4-byte aligned only)"""
    buf = torch.full((host.numel() + 4,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[shift:shift + host.numel()]
    view.copy_(host)
    assert view.data_ptr() % 16 == (4 * shift) % 16
    return view


def run_guard(ops, grad, chunk=None, **kw):
    tab = ops.grad_guard_table(OFFSETS, NUMELS, N, DEV, **({} if chunk is None else {"chunk": chunk}))
    sumsq = torch.full((len(NUMELS),), -1.0, dtype=torch.float64, device=DEV)
    rec = ops.guard_record(DEV)
    ops.grad_guard(grad, tab, sumsq, rec, **kw)
    torch.cuda.synchronize()
    return sumsq.cpu().numpy(), ops.read_guard_record(rec), rec.cpu().numpy().tobytes()


def f32_ulps(a, b):
    return ulps(torch.tensor([a], dtype=torch.float32), torch.tensor([b], dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ 1. norm against fp64
@pytest.mark.parametrize("shift", [0, 1])
def test_norm_matches_fp64(ops, host_arena, reference, shift):
    per_ref, total_ref = reference
    norm_ref = math.sqrt(total_ref)
    max_norm = float(np.float32(0.3 * norm_ref))
    _, coef_ref = G.coef(total_ref, max_norm)
    sumsq, r, _ = run_guard(ops, on_device(host_arena, shift), grad_scale=GRAD_SCALE, max_norm=max_norm)
    worst = 0.0
    for p, (c, got, ref) in enumerate(zip(NUMELS, sumsq, per_ref)):
        err, lim = abs(got - ref) / ref, c * 2.0 ** -52
        print(f"[shift {shift}] tensor {p} ({c} elements): rel err {err:.3e}, limit {lim:.3e}")
        worst = max(worst, err / lim)
        assert err <= lim, f"tensor {p}: {err:.3e} > {lim:.3e}"
    n_all = sum(NUMELS)
    err = abs(r["sumsq"] - total_ref) / total_ref
    print(f"[shift {shift}] total: rel err {err:.3e}, limit {n_all * 2.0 ** -52:.3e}")
    record(f"grad_guard/sumsq_err_over_limit[shift={shift}]", max(worst, err / (n_all * 2.0 ** -52)), 1.0)
    assert err <= n_all * 2.0 ** -52
    u_norm, u_coef = f32_ulps(r["norm"], norm_ref), f32_ulps(r["coef"], coef_ref)
    print(f"[shift {shift}] norm {r['norm']:.6e} ({u_norm} ulp), coef {r['coef']:.6f} ({u_coef} ulp)")
    record(f"grad_guard/norm_coef_ulp[shift={shift}]", max(u_norm, u_coef), 1)
    assert u_norm <= 1 and u_coef <= 1 and 0.29 < r["coef"] < 0.31
    assert r["skip"] == 0 and (r["steps"], r["skipped"], r["clipped"], r["consecutive_skips"]) == (1, 0, 1, 0)
    assert r["clip_value"] == float("inf")


def test_coef_is_exactly_one_under_the_limit_and_with_the_limit_off(ops, host_arena, reference):
    norm_ref = math.sqrt(reference[1])
    grad = on_device(host_arena, 0)
    for max_norm in (float(np.float32(1.5 * norm_ref)), None, float("inf")):
        _, r, _ = run_guard(ops, grad, grad_scale=GRAD_SCALE, max_norm=max_norm)
        assert r["coef"] == 1.0 and r["clipped"] == 0, max_norm
    _, r, _ = run_guard(ops, grad, grad_scale=GRAD_SCALE, max_norm=float(np.float32(0.999 * norm_ref)))
    assert r["coef"] < 1.0 and r["clipped"] == 1


# ------------------------------------------------------------------------------------------------ 2. determinism
@pytest.mark.parametrize("shift", [0, 1])
def test_two_runs_and_two_chunk_lengths_give_the_same_bits(ops, host_arena, shift):
    grad = on_device(host_arena, shift)
    runs = [run_guard(ops, grad, chunk=chunk, grad_scale=GRAD_SCALE, max_norm=1.0, count=False)
            for chunk in (None, None, 1024, 8192, 1 << 20)]
    for sumsq, r, raw in runs[1:]:
        assert sumsq.tobytes() == runs[0][0].tobytes(), "per-tensor sums differ between runs / chunk lengths"
        assert raw == runs[0][2], "the record differs between runs / chunk lengths"
    assert runs[0][1]["steps"] == 0                         # count=False: a reduction for its own sake counts no step


# ------------------------------------------------------------------------------------------------ 3. non-finite detection
# first element, last element, the single-element tail of a tensor whose length is no multiple of 4 (65, 4097, 70001), and
# the last element before a padding gap (tensor 1: 3 elements, then 61 of padding)
PLACES = {"first": OFFSETS[0], "last": OFFSETS[5] + NUMELS[5] - 1, "tail-of-65": OFFSETS[3] + 64,
          "tail-of-4097": OFFSETS[4] + 4096, "before-padding": OFFSETS[1] + 2, "inside": OFFSETS[5] + 33333}


@pytest.mark.parametrize("shift", [0, 1])
def test_nonfinite_elements_are_found_and_padding_is_not_read(ops, host_arena, shift):
    grad = on_device(host_arena, shift)
    clean = grad.clone()
    tab = ops.grad_guard_table(OFFSETS, NUMELS, N, DEV)
    sumsq = torch.zeros(len(NUMELS), dtype=torch.float64, device=DEV)
    rec_on, rec_off = ops.guard_record(DEV), ops.guard_record(DEV)
    ops.grad_guard(grad, tab, sumsq, rec_on, skip_nonfinite=True)
    assert ops.read_guard_record(rec_on)["skip"] == 0
    expect_skipped = 0
    for name, at in PLACES.items():
        for bad in (float("nan"), float("inf"), float("-inf")):
            grad[at] = bad
            assert G.nonfinite(grad.cpu().numpy(), OFFSETS, NUMELS, 1.0)
            ops.grad_guard(grad, tab, sumsq, rec_on, skip_nonfinite=True)
            ops.grad_guard(grad, tab, sumsq, rec_off, skip_nonfinite=False)
            expect_skipped += 1
            on, off = ops.read_guard_record(rec_on), ops.read_guard_record(rec_off)
            assert on["skip"] == 1 and on["skipped"] == expect_skipped and on["consecutive_skips"] == expect_skipped, (name, bad)
            assert off["skip"] == 0 and off["skipped"] == 0, (name, bad)
            assert not math.isfinite(off["norm"])           # without the flag the non-finite gradient goes through as it is
            grad.copy_(clean)
    # a NaN / an infinity in the PADDING trips nothing and changes no sum
    ops.grad_guard(grad, tab, sumsq, rec_on, skip_nonfinite=True)
    before = (sumsq.cpu().numpy().tobytes(), ops.read_guard_record(rec_on)["sumsq"])
    for o, c in zip(OFFSETS, NUMELS):
        end = (o + c + 63) // 64 * 64
        if end > o + c:
            grad[o + c] = float("nan")
            grad[end - 1] = float("inf")
    assert not G.nonfinite(grad.cpu().numpy(), OFFSETS, NUMELS, 1.0)
    ops.grad_guard(grad, tab, sumsq, rec_on, skip_nonfinite=True)
    r = ops.read_guard_record(rec_on)
    assert r["skip"] == 0 and r["consecutive_skips"] == 0 and r["skipped"] == expect_skipped
    assert (sumsq.cpu().numpy().tobytes(), r["sumsq"]) == before
    # beyond 3e38 only after the scale: |g * grad_scale| counts too
    grad.copy_(clean)
    grad[PLACES["inside"]] = 2.0e38
    ops.grad_guard(grad, tab, sumsq, rec_on, skip_nonfinite=True, grad_scale=1.0)
    assert ops.read_guard_record(rec_on)["skip"] == 0
    ops.grad_guard(grad, tab, sumsq, rec_on, skip_nonfinite=True, grad_scale=2.0)
    assert ops.read_guard_record(rec_on)["skip"] == 1


# ------------------------------------------------------------------------------------------------ 4. guarded Adam, clipping
N_ADAM = 70001 + 4097           # more than one pass of the grid-stride loop's tail: n % 4 == 2


def _adam_case(seed, conditioned):
    g = torch.Generator().manual_seed(seed)
    grad = torch.randn(N_ADAM, generator=g)
    st = random_state(g, random_theta(g, N_ADAM, conditioned), grad, conditioned)
    st["grad"] = grad
    return st


def _adam_table(ops):
    # two tensors with padding between them inside the arena the optimizer kernel sweeps whole
    offs, numels = [0, 70016], [70001, N_ADAM - 70016]
    return ops.grad_guard_table(offs, numels, N_ADAM, DEV), offs, numels


def _adam64(st, scale, clip_value=None, profiles=(), betas=()):
    rec = step_record("cpu").numpy().view(np.float32).astype(np.float64)
    lr, beta, _gs, bc1, bc2s = rec[4:9]
    b1, b2, eps = (float(np.float32(x)) for x in (B1, B2, EPS))
    d = {k: st[k].double().numpy() for k in ("theta", "grad", "m", "v", "ema")}
    return G.guarded_adam64(d["theta"], d["grad"], d["m"], d["v"], d["ema"], lr=lr, b1=b1, b2=b2, eps=eps, bc1=bc1,
                            bc2sqrt=bc2s, ema_beta=beta, scale=scale, clip_value=clip_value,
                            profiles=[p.double().numpy() for p in profiles], profile_betas=betas)


def _guarded(ops, S, tab, numels, max_norm=None, clip_value=None, skip_nonfinite=False, profiles=None, betas=None,
             rec=None, dyn=None):
    sumsq = torch.zeros(len(numels), dtype=torch.float64, device=DEV)
    rec = ops.guard_record(DEV) if rec is None else rec
    args = (LR, B1, B2, EPS, STEP, EMA_BETA, GRAD_SCALE)
    ops.grad_guard(S["grad"], tab, sumsq, rec, grad_scale=GRAD_SCALE, dyn=dyn, max_norm=max_norm, clip_value=clip_value,
                   skip_nonfinite=skip_nonfinite)
    if profiles is None:
        ops.adam_ema_guarded(S["theta"], S["grad"], S["m"], S["v"], S["ema"], rec, *args, dyn=dyn, zero_grad=True)
    else:
        ops.adam_ema_phema_guarded(S["theta"], S["grad"], S["m"], S["v"], S["ema"], profiles, betas, rec, *args, dyn=dyn,
                                   zero_grad=True)
    torch.cuda.synchronize()
    return ops.read_guard_record(rec), rec


@pytest.mark.parametrize("form", ["plain", "plain-dyn", "phema"])
def test_guarded_adam_clips_like_adam_ema_with_the_scaled_gradient(ops, form):
    tab, offs, numels = _adam_table(ops)
    args = (LR, B1, B2, EPS, STEP, EMA_BETA)
    keys = ("theta", "m", "v", "ema")
    worst_ulp = 0
    for conditioned in (True, False):
        st = _adam_case(77, conditioned)
        _, total = G.sumsq(st["grad"].numpy(), offs, numels, GRAD_SCALE)
        max_norm = float(np.float32(0.3 * math.sqrt(total)))
        A = {k: t.clone().to(DEV) for k, t in st.items()}
        Bq = {k: t.clone().to(DEV) for k, t in st.items()}
        prof0 = [st["theta"] * (0.8 + 0.1 * k) for k in range(2)] if form == "phema" else None
        betas = torch.tensor([0.75, 0.9375], dtype=torch.float32, device=DEV) if form == "phema" else None
        pa = None if prof0 is None else [p.clone().to(DEV) for p in prof0]
        pb = None if prof0 is None else [p.clone().to(DEV) for p in prof0]
        r, _ = _guarded(ops, Bq, tab, numels, max_norm=max_norm, profiles=pb, betas=betas,
                        dyn=step_record() if form == "plain-dyn" else None)
        assert 0.29 < r["coef"] < 0.31 and r["skip"] == 0 and r["clipped"] == 1
        scale = float(np.float32(GRAD_SCALE) * np.float32(r["coef"]))      # the fp32 product the guarded kernel forms
        if form == "phema":
            ops.adam_ema_phema(A["theta"], A["grad"], A["m"], A["v"], A["ema"], pa, betas, *args, scale, zero_grad=True)
        else:
            ops.adam_ema(A["theta"], A["grad"], A["m"], A["v"], A["ema"], *args, scale, zero_grad=True)
        torch.cuda.synchronize()
        ops.check_health(DEV, "guarded Adam on finite operands")
        assert float(Bq["grad"].abs().max()) == 0.0
        ref = _adam64(st, scale, profiles=prof0 or (), betas=(0.75, 0.9375))
        pairs = [(k, A[k], Bq[k], ref[i]) for i, k in enumerate(keys)]
        if form == "phema":
            pairs += [(f"profile{k}", pa[k], pb[k], ref[4][k]) for k in range(2)]
        for k, a, b, r64 in pairs:
            u = ulps(a, b)
            ea = float(np.abs(a.cpu().double().numpy() - r64).max())
            eb = float(np.abs(b.cpu().double().numpy() - r64).max())
            print(f"[{form}, conditioned={conditioned}] {k}: guarded vs unguarded {u} ulp; max abs err vs fp64 "
                  f"unguarded {ea:.3e} guarded {eb:.3e}")
            if conditioned:
                worst_ulp = max(worst_ulp, u)
                assert u <= 2, f"{k}: {u} ulp"
            else:
                record(f"grad_guard/adam_err_over_unguarded_err[{form}/{k}]", eb / max(ea, 1e-300), 2.0)
                assert eb <= 2.0 * ea, f"{k}: guarded error {eb:.3e} > 2 x unguarded {ea:.3e}"
    record(f"grad_guard/adam_vs_adam_ema_ulp[{form}]", worst_ulp, 2)


def test_guarded_adam_under_the_limit_equals_the_unscaled_step(ops):
    """coef == 1 exactly when the norm is under max_norm: the step is that of grad_scale alone"""
    tab, offs, numels = _adam_table(ops)
    st = _adam_case(78, True)
    A = {k: t.clone().to(DEV) for k, t in st.items()}
    Bq = {k: t.clone().to(DEV) for k, t in st.items()}
    _, total = G.sumsq(st["grad"].numpy(), offs, numels, GRAD_SCALE)
    r, _ = _guarded(ops, Bq, tab, numels, max_norm=float(np.float32(1.01 * math.sqrt(total))))
    assert r["coef"] == 1.0 and r["clipped"] == 0
    ops.adam_ema(A["theta"], A["grad"], A["m"], A["v"], A["ema"], LR, B1, B2, EPS, STEP, EMA_BETA, GRAD_SCALE, zero_grad=True)
    torch.cuda.synchronize()
    for k in ("theta", "m", "v", "ema"):
        assert ulps(A[k], Bq[k]) <= 2, k


def test_guarded_adam_clip_value_matches_fp64(ops):
    """gradient_clip_algorithm="value": every scaled element limited to +-clip_value.  The yardstick is ops.adam_ema fed the
    gradient clipped on the host (scale 1): largest error against fp64 at most twice its, and 2 ulp on the conditioned state"""
    tab, offs, numels = _adam_table(ops)
    clip = 0.25                                             # of N(0, 1) * 0.5: about 62 % of the elements are limited
    for conditioned in (True, False):
        st = _adam_case(79, conditioned)
        clipped = (st["grad"] * np.float32(GRAD_SCALE)).clamp(-clip, clip)
        assert 0.5 < float((clipped.abs() == clip).float().mean()) < 0.7
        if conditioned:                                     # (m keeps the sign of the gradient: clipping does not flip it)
            assert bool((torch.sign(clipped) == torch.sign(st["grad"])).all())
        A = {k: t.clone().to(DEV) for k, t in st.items()}
        A["grad"] = clipped.to(DEV)
        Bq = {k: t.clone().to(DEV) for k, t in st.items()}
        r, _ = _guarded(ops, Bq, tab, numels, clip_value=clip)
        assert r["coef"] == 1.0 and r["clip_value"] == clip and r["skip"] == 0
        ops.adam_ema(A["theta"], A["grad"], A["m"], A["v"], A["ema"], LR, B1, B2, EPS, STEP, EMA_BETA, 1.0, zero_grad=True)
        torch.cuda.synchronize()
        ops.check_health(DEV, "clip_value on finite operands")
        ref = _adam64(st, float(np.float32(GRAD_SCALE)), clip_value=clip)
        for i, k in enumerate(("theta", "m", "v", "ema")):
            u = ulps(A[k], Bq[k])
            ea = float(np.abs(A[k].cpu().double().numpy() - ref[i]).max())
            eb = float(np.abs(Bq[k].cpu().double().numpy() - ref[i]).max())
            print(f"[clip_value, conditioned={conditioned}] {k}: {u} ulp; max abs err vs fp64 unguarded {ea:.3e} guarded {eb:.3e}")
            if conditioned:
                record(f"grad_guard/clip_value_vs_adam_ema_ulp[{k}]", u, 2)
                assert u <= 2, f"{k}: {u} ulp"
            else:
                record(f"grad_guard/clip_value_err_over_unguarded_err[{k}]", eb / max(ea, 1e-300), 2.0)
                assert eb <= 2.0 * ea, f"{k}: {eb:.3e} > 2 x {ea:.3e}"


# ------------------------------------------------------------------------------------------------ 5. guarded Adam, skip
@pytest.mark.parametrize("form", ["plain", "phema"])
def test_a_skipped_step_changes_nothing_but_the_gradient_arena(ops, form):
    tab, offs, numels = _adam_table(ops)
    st = _adam_case(80, True)
    S = {k: t.clone().to(DEV) for k, t in st.items()}
    prof0 = [st["theta"] * 0.9, st["theta"] * 1.1] if form == "phema" else None
    prof = None if prof0 is None else [p.clone().to(DEV) for p in prof0]
    betas = torch.tensor([0.75, 0.9375], dtype=torch.float32, device=DEV) if form == "phema" else None
    S["grad"][12345] = float("nan")
    ops.check_health(DEV, "before")
    r, rec = _guarded(ops, S, tab, numels, max_norm=1.0, skip_nonfinite=True, profiles=prof, betas=betas)
    assert r["skip"] == 1 and (r["steps"], r["skipped"], r["consecutive_skips"], r["clipped"]) == (1, 1, 1, 0)
    for k in ("theta", "m", "v", "ema"):
        assert torch.equal(S[k].cpu(), st[k]), f"{k} changed in a skipped step"
    if prof is not None:
        assert all(torch.equal(p.cpu(), p0) for p, p0 in zip(prof, prof0))
    assert float(S["grad"].abs().max()) == 0.0 and not bool(torch.isnan(S["grad"]).any())
    ops.check_health(DEV, "a skipped step leaves the health word alone")        # does not raise
    # a clean step follows: it updates as an unguarded one does and ends the run of skips
    S["grad"].copy_(st["grad"])
    A = {k: t.clone().to(DEV) for k, t in st.items()}
    r, _ = _guarded(ops, S, tab, numels, max_norm=None, skip_nonfinite=True, profiles=prof, betas=betas, rec=rec)
    assert r["skip"] == 0 and (r["steps"], r["skipped"], r["consecutive_skips"]) == (2, 1, 0) and r["coef"] == 1.0
    ops.adam_ema(A["theta"], A["grad"], A["m"], A["v"], A["ema"], LR, B1, B2, EPS, STEP, EMA_BETA, GRAD_SCALE, zero_grad=True)
    torch.cuda.synchronize()
    for k in ("theta", "m", "v", "ema"):
        assert ulps(A[k], S[k]) <= 2 and not torch.equal(S[k].cpu(), st[k]), k
    if prof is not None:
        assert not torch.equal(prof[0].cpu(), prof0[0])


def test_without_the_flag_a_nonfinite_gradient_goes_through_and_sets_the_health_bit(ops):
    tab, offs, numels = _adam_table(ops)
    st = _adam_case(81, True)
    S = {k: t.clone().to(DEV) for k, t in st.items()}
    S["grad"][7] = float("nan")
    ops.check_health(DEV, "before")
    r, _ = _guarded(ops, S, tab, numels, max_norm=1.0, skip_nonfinite=False)
    assert r["skip"] == 0 and math.isnan(r["norm"])
    with pytest.raises(ops.GraphCorruptionError, match="non-finite gradient"):
        ops.check_health(DEV, "non-finite gradient without skip_nonfinite")


# ------------------------------------------------------------------------------------------------ 7. data parallel, emulated
def test_half_the_grad_scale_gives_half_the_norm(ops, host_arena):
    """1/world rides in grad_scale: a power of two scales every fp64 product exactly, so the norm halves to the bit"""
    grad = on_device(host_arena, 0)
    s1, r1, _ = run_guard(ops, grad, grad_scale=1.0, max_norm=1.0e9)
    s2, r2, _ = run_guard(ops, grad, grad_scale=0.5, max_norm=1.0e9)
    assert r2["sumsq"] == 0.25 * r1["sumsq"] and (s2 == 0.25 * s1).all()
    assert r2["norm"] == 0.5 * r1["norm"]
    for r in (r1, r2):
        assert f32_ulps(r["coef"], G.coef(r["sumsq"], 1.0e9)[1]) <= 1
    # the same through the device record (dyn) as through the by-value argument
    dyn = step_record()                                     # grad_scale = GRAD_SCALE = 0.5
    assert GRAD_SCALE == 0.5
    s3, r3, _ = run_guard(ops, grad, grad_scale=123.0, dyn=dyn, max_norm=1.0e9)
    assert s3.tobytes() == s2.tobytes() and (r3["sumsq"], r3["coef"]) == (r2["sumsq"], r2["coef"])


# ------------------------------------------------------------------------------------------------ 6. step level
def _setup(monkeypatch):
    from test_graph_gpu import _build, _opt
    monkeypatch.setenv("EDM_FUSED_OPT", "1")
    model, _ = _build()
    opt, base, sched = _opt(model)
    return model, opt, base, sched


def test_captured_guarded_step_matches_the_eager_one_and_takes_the_unfused_path(monkeypatch):
    """6a: tiny max_norm (every step clips), six batches, captured against eager, the limits of
    test_captured_step_fused_matches_unfused; the path is "unfused" while the guard is set and "fused" again without it"""
    from test_graph_gpu import rel
    from tinyedm_amd.graph import CapturedTrainStep
    batches = _batches(6)
    # ---- eager
    model_e, opt_e, base_e, sched_e = _setup(monkeypatch)
    base_e.fuse_zero_grad = True
    base_e.set_guard(max_norm=1e-3)
    opt_e.zero_grad()
    for b in batches:
        loss = model_e.training_step(b, 0)
        loss.backward()
        opt_e.step()
        opt_e.zero_grad()
        sched_e.step()
    stats_e = opt_e.guard_stats()                           # (EMAOptimizer passes the guard's surface through)
    # ---- captured
    model_g, opt_g, base_g, sched_g = _setup(monkeypatch)
    base_g.fuse_zero_grad = True
    opt_g.set_guard(max_norm=1e-3)
    opt_g.zero_grad()
    step = CapturedTrainStep(model_g, opt_g)
    assert step.path() == "unfused"
    paths = []
    for b in batches:
        step(b)
        sched_g.step()
        paths.append(step.last_path)
    torch.cuda.synchronize()
    assert paths == ["unfused"] * 6 and len(step._graphs) == 1
    stats_g = base_g.guard_stats()
    assert stats_e["clipped_steps"] == stats_g["clipped_steps"] == 6 and stats_g["skipped_steps"] == 0
    assert stats_g["clip_coef"] < 1.0 and stats_e["clip_coef"] < 1.0
    assert (base_g.step_count, opt_g.current_step) == (base_e.step_count, opt_e.current_step)
    for name, a, b, lim in (("theta", base_g.arena.theta, base_e.arena.theta, 2e-3), ("adam_m", base_g.m, base_e.m, 2e-2),
                            ("adam_v", base_g.v, base_e.v, 2e-2), ("ema", opt_g.ema_arena, opt_e.ema_arena, 2e-3)):
        e = rel(a, b)
        print(f"guarded captured vs guarded eager step, {name}: rel {e:.3e}")
        record(f"grad_guard/captured_step/{name}_vs_eager", e, lim)
        assert e <= lim, f"{name}: rel {e:.3e}"
    assert float(base_g.arena.grad.abs().max()) == 0.0
    assert "guard" in base_g.state_dict() and base_g.state_dict()["guard"]["clipped"] == 6
    opt_g.set_guard()
    assert base_g.guard is None and "guard" not in base_g.state_dict() and step.path() == "fused"
    step(batches[0])
    assert step.last_path == "fused"
    step(batches[1])
    assert step.last_path == "fused" and len(step._graphs) == 2


def test_guard_stats_equal_the_norm_of_the_arena_before_the_step(monkeypatch):
    """6b: eager, fuse_zero_grad off: the gradient stays in the arena, so torch can take its norm"""
    model, opt, base, _ = _setup(monkeypatch)
    assert base.fuse_zero_grad is False
    base.set_guard(max_norm=1e6)
    opt.zero_grad()
    b = _batches(1, seed=12)[0]
    model.training_step(b, 0).backward()
    torch.cuda.synchronize()
    g64 = base.arena.grad.double()
    want = float(torch.linalg.vector_norm(g64))
    want_per = [float(torch.linalg.vector_norm(g64[o:o + p.numel()])) for p, o in zip(base.arena.params, base.arena.offsets)]
    alone, alone_per = base.grad_norm(), base.grad_norm(per_tensor=True)        # the reduction alone: device tensors, no step
    assert alone.is_cuda and alone.dtype == torch.float64 and alone_per.shape == (len(base.arena.params),)
    opt.step()
    st = base.guard_stats()
    u = f32_ulps(st["grad_norm"], want)
    print(f"guard_stats grad_norm {st['grad_norm']:.8e} vs torch {want:.8e}: {u} ulp")
    record("grad_guard/step/grad_norm_ulp", u, 1)
    assert u <= 1 and st["clip_coef"] == 1.0 and st["steps"] == 1 and st["skipped_steps"] == 0
    assert f32_ulps(float(alone), want) <= 1
    per = base.per_tensor_grad_norms().cpu().numpy()
    worst = max(f32_ulps(float(a), w) for a, w in zip(per, want_per))
    record("grad_guard/step/per_tensor_norm_ulp", worst, 1)
    assert worst <= 1 and per.tobytes() == alone_per.cpu().numpy().tobytes()
    assert float(base.arena.grad.abs().max()) > 0.0         # torch semantics: step() left .grad for the caller to clear


class _Snapshots:
    """weights, moments and EMA after every optimizer step, through the Trainer's on_train_batch_end hook"""

    def __init__(self):
        self.states = []

    def on_train_batch_end(self, trainer, pl_module, *args):
        opt = trainer.optimizers[0]
        base = opt.optimizer
        torch.cuda.synchronize()
        self.states.append({"theta": base.arena.theta.clone(), "m": base.m.clone(), "v": base.v.clone(),
                            "ema": opt.ema_arena.clone()})


def _fit(monkeypatch, graph, poisoned, n_batches=3, seed=6, **trainer_kw):
    import tinyedm_amd as T
    from test_graph_gpu import _build
    monkeypatch.setenv("EDM_GRAPH", graph)
    model, _ = _build(seed=seed)
    g = torch.Generator().manual_seed(8)
    xs = 0.5 * torch.randn(n_batches, 8, 3, 16, 16, generator=g)
    for i in poisoned:
        xs[i, 0, 0, 0, 0] = float("nan")                    # one NaN pixel
    loader = [(xs[i], torch.randint(0, 10, (8,), generator=g)) for i in range(n_batches)]
    snaps = _Snapshots()
    tr = T.Trainer(max_epochs=1, log_every_n_steps=1, callbacks=[snaps], **trainer_kw)
    tr.fit(model, train_dataloaders=loader)
    torch.cuda.synchronize()
    return tr, snaps


def _after_a_forward_alone(theta, seed=6):
    """What a training-mode forward ALONE makes of the weights `theta`: every weight-normalised layer rewrites its master
    weight with its normalised self before it is used (the reference's forced weight normalisation, networks.py:32-34), a
    function of the weights only.  A second model of the same layout, no backward pass, no optimizer step."""
    from test_graph_gpu import _build
    from tinyedm_amd import networks as N
    model, _ = _build(seed=seed)
    base = model.configure_optimizers()["optimizer"]        # (re-homes the parameters into a flat arena of the same layout)
    assert base.arena.theta.shape == theta.shape
    base.arena.theta.copy_(theta)
    N.bump_weight_epoch()
    with torch.no_grad():
        model.training_step(_batches(1, seed=99)[0], 0)
    torch.cuda.synchronize()
    return base.arena.theta.clone()


@pytest.mark.parametrize("n_batches,poisoned", [(3, 1), (6, 4)])     # (6, 4): the poisoned step is a REPLAY of the graph
def test_fit_skips_a_poisoned_batch_in_the_replay_and_in_the_eager_loop(monkeypatch, n_batches, poisoned):
    """6c.  On the parent the keyword is swallowed and the run ends in GraphCorruptionError.

    "Bitwise equal before and after the bad step" holds as stated for the moments and the EMA, which only the optimizer
    writes.  The master weights are also rewritten by every training-mode FORWARD (the forced weight normalisation, which
    reads nothing of the batch), so a snapshot taken after the previous step differs from one taken after the skipped step by
    exactly that: the weights after the skipped step must be bit for bit what a forward alone makes of the previous ones --
    the optimizer has not moved a bit (the kernel-level test above shows the same without a network)."""
    from tinyedm_amd import ops
    final = {}
    for graph in ("1", "0"):
        tr, snaps = _fit(monkeypatch, graph, [poisoned], n_batches=n_batches, skip_nonfinite_steps=True)
        assert tr.step_launch == ("hipGraph replay" if graph == "1" else "eager loop")
        assert tr.callback_metrics["skipped_steps"] == 1 and len(snaps.states) == n_batches
        stats = tr.optimizers[0].guard_stats()
        assert stats["skipped_steps"] == 1 and stats["steps"] == n_batches and stats["consecutive_skips"] == 0
        for k in ("theta", "m", "v", "ema"):
            assert all(bool(torch.isfinite(s[k]).all()) for s in snaps.states), k
            before = snaps.states[poisoned - 1][k]
            if k == "theta":
                before = _after_a_forward_alone(before)
            assert torch.equal(snaps.states[poisoned][k], before), f"{k} changed in the skipped step"
            assert not torch.equal(snaps.states[poisoned + 1][k], snaps.states[poisoned][k]), f"{k}: the next step did not update"
        ops.check_health(DEV, "after a fit with a skipped step")
        final[graph] = snaps.states
    from test_graph_gpu import rel
    for k, lim in (("theta", 2e-3), ("m", 2e-2), ("v", 2e-2), ("ema", 2e-3)):
        e = rel(final["1"][-1][k], final["0"][-1][k])
        record(f"grad_guard/fit_skip/{k}_graph_vs_eager[{n_batches}]", e, lim)
        assert e <= lim, f"{k}: EDM_GRAPH=1 vs 0 rel {e:.3e}"


def test_fit_raises_after_max_consecutive_skips(monkeypatch):
    """6d"""
    from tinyedm_amd import ops
    with pytest.raises(ops.GraphCorruptionError, match="max_consecutive_skips=2"):
        _fit(monkeypatch, "1", [0, 1, 2, 3], n_batches=4, skip_nonfinite_steps=True, max_consecutive_skips=2)
    ops.health(DEV).zero_()


def test_fit_with_gradient_clip_val_logs_a_coefficient_below_one(monkeypatch, capsys):
    """6e.  On the parent the keyword is swallowed and nothing is logged."""
    tr, snaps = _fit(monkeypatch, "1", [], n_batches=4, gradient_clip_val=1e-3)
    m = tr.callback_metrics
    assert 0.0 < m["grad_clip_coef"] < 1.0 and m["grad_norm"] > 1e-3 and m["skipped_steps"] == 0
    assert abs(m["grad_clip_coef"] - 1e-3 / (m["grad_norm"] + 1e-6)) <= 1e-6 * m["grad_clip_coef"]
    out = capsys.readouterr().out
    assert "grad_norm" in out and "clip_coef" in out and "skipped 0" in out
    assert tr.optimizers[0].guard_stats()["clipped_steps"] == 4
    # "value" goes to the per-element limit instead
    tr, _ = _fit(monkeypatch, "0", [], n_batches=2, gradient_clip_val=1e-4, gradient_clip_algorithm="value")
    g = tr.optimizers[0].guard
    assert (g.max_norm, g.clip_value) == (None, 1e-4) and tr.callback_metrics["grad_clip_coef"] == 1.0


def test_grad_norm_monitor_writes_the_top_tensors(monkeypatch, tmp_path):
    import json
    import tinyedm_amd as T
    from test_graph_gpu import _build
    from tinyedm_amd.callbacks import GradNormMonitor
    monkeypatch.setenv("EDM_GRAPH", "1")
    model, _ = _build(seed=6)
    loader = [(b[0].cpu(), b[1].cpu()) for b in _batches(4, seed=3)]
    path = tmp_path / "norms.jsonl"
    mon = GradNormMonitor(every_n_steps=2, path=str(path), top=3)
    tr = T.Trainer(max_epochs=1, log_every_n_steps=1, callbacks=[mon])
    tr.fit(model, train_dataloaders=loader)
    lines = [json.loads(l) for l in path.read_text().splitlines()]
    assert [l["step"] for l in lines] == [2, 4]
    names = {n for n, _ in model.named_parameters()}
    for l in lines:
        assert len(l["top"]) == 3 and all(t["name"] in names and t["numel"] > 0 for t in l["top"])
        norms = [t["grad_norm"] for t in l["top"]]
        assert norms == sorted(norms, reverse=True) and norms[0] <= l["grad_norm"] * (1 + 1e-6) and l["grad_norm"] > 0
    g = tr.optimizers[0].guard                               # the monitor's own guard: every limit off
    assert (g.max_norm, g.clip_value, g.skip_nonfinite) == (None, None, False)
    assert tr.callback_metrics["grad_clip_coef"] == 1.0


def test_guarded_captured_step_behind_a_reducer_reads_the_scale_from_the_device_record(monkeypatch):
    """7, at the step level.  tests/test_rccl_gpu.py keeps its forced single-rank RCCL group inside spawned workers with a
    fixed script, so nothing of it can be imported; a stand-in reducer (world 1, finish() a no-op) puts the captured step
    on the data-parallel path instead -- reducer.finish(), then the guard, with 1/world = 0.5 riding in the device record --
    and an eager run with grad_scale = 0.5 is the yardstick.  Real multi-rank runs stay unexercised, as on every box here."""
    import types
    from test_graph_gpu import rel
    from tinyedm_amd.graph import CapturedTrainStep
    batches = _batches(4, seed=21)
    model_e, opt_e, base_e, sched_e = _setup(monkeypatch)
    base_e.fuse_zero_grad = True
    base_e.set_guard(max_norm=1e-3)
    base_e.grad_scale = 0.5
    opt_e.zero_grad()
    norms_e = []
    for b in batches:
        model_e.training_step(b, 0).backward()
        opt_e.step()
        opt_e.zero_grad()
        sched_e.step()
        norms_e.append(base_e.guard_stats()["grad_norm"])
    model_g, opt_g, base_g, sched_g = _setup(monkeypatch)
    base_g.fuse_zero_grad = True
    base_g.set_guard(max_norm=1e-3)
    opt_g.zero_grad()
    calls = []
    reducer = types.SimpleNamespace(active=True, world=1, capturable=lambda: True, finish=lambda: calls.append(1) or 1.0,
                                    reset=lambda: None)
    step = CapturedTrainStep(model_g, opt_g, grad_scale=0.5, reducer=reducer)
    norms_g = []
    for b in batches:
        step(b)
        sched_g.step()
        assert step.last_path == "unfused"
        norms_g.append(base_g.guard_stats()["grad_norm"])
    torch.cuda.synchronize()
    assert len(step._graphs) == 1 and len(calls) == 3       # two warm-up steps and the capture; the replay calls nothing
    assert abs(norms_g[0] / norms_e[0] - 1.0) < 1e-3        # (the first step starts from identical weights)
    for name, a, b, lim in (("theta", base_g.arena.theta, base_e.arena.theta, 2e-3), ("adam_m", base_g.m, base_e.m, 2e-2),
                            ("adam_v", base_g.v, base_e.v, 2e-2), ("ema", opt_g.ema_arena, opt_e.ema_arena, 2e-3)):
        e = rel(a, b)
        record(f"grad_guard/reducer_step/{name}_vs_eager", e, lim)
        assert e <= lim, f"{name}: rel {e:.3e}"
    # half the scale: the norm of the same gradient is half that of an unscaled run's first step
    model_1, opt_1, base_1, _ = _setup(monkeypatch)
    base_1.set_guard(max_norm=1e-3)
    opt_1.zero_grad()
    model_1.training_step(batches[0], 0).backward()
    opt_1.step()
    assert abs(norms_e[0] / (0.5 * base_1.guard_stats()["grad_norm"]) - 1.0) < 1e-3


def test_state_dict_carries_the_limits_and_counters(ops):
    from tinyedm_amd.ema import FusedAdam
    g = torch.Generator().manual_seed(4)
    init = [torch.randn(5, generator=g), torch.randn(70, 3, generator=g)]
    opt = FusedAdam([torch.nn.Parameter(t.clone().to(DEV)) for t in init], lr=1e-3)
    assert "guard" not in opt.state_dict()
    opt.set_guard(max_norm=0.5, skip_nonfinite=True)
    opt.arena.grad.copy_(torch.randn(opt.arena.grad.numel(), generator=g))
    opt.step()                                              # norm ~ sqrt(215) > 0.5: clipped
    opt.arena.grad[3] = float("nan")
    opt.step()                                              # skipped
    sd = opt.state_dict()
    assert sd["guard"] == {"max_norm": 0.5, "clip_value": None, "skip_nonfinite": True, "steps": 2, "skipped": 1,
                           "clipped": 1, "consecutive_skips": 1}
    ops.check_health(DEV, "a clipped and a skipped step")
    opt2 = FusedAdam([torch.nn.Parameter(t.clone().to(DEV)) for t in init], lr=1e-3)
    opt2.set_guard(max_norm=0.5, skip_nonfinite=True)
    opt2.load_state_dict(sd)
    st = opt2.guard_stats()
    assert (st["steps"], st["skipped_steps"], st["clipped_steps"], st["consecutive_skips"]) == (2, 1, 1, 1)
    assert torch.equal(opt2.m, opt.m) and opt2.step_count == 2
    FusedAdam([torch.nn.Parameter(t.clone().to(DEV)) for t in init], lr=1e-3).load_state_dict(sd)   # no guard here: ignored
