"""Adam + EMA applied inside the 3x3 weight-gradient finish of a captured step (csrc/conv_wgrad3.hip k_wgrad3_finish<true>,
csrc/optim.hip k_adam_ema_ranges, graph.CapturedTrainStep): the apply form against the parent's two-kernel path
(ops.wgrad3_group into a zero arena, then ops.adam_ema) and against an fp64 evaluation of the same formulas; the ranges
form of the optimizer kernel against k_adam_ema; the captured step with the fused path on and off.

Limits.  The two paths evaluate the same fp32 expressions on the same operands (the raw gradient comes from the same
k_wgrad3 launch, whose partial tiles are summed in a fixed order), so they can differ only where the compiler contracts
a*x + b*y into an FMA in one kernel and not in the other, i.e. by one rounding of a product more or less: 2 ulp OF THE
LARGER TERM.  That is 2 ulp of the result only where the sum does not cancel, so the state compared in ulps is random
but well conditioned (random_state(conditioned=True): m has the gradient's sign, the EMA its weight's sign, |theta| >= 0.25, far
above the 3e-3 an update moves it).  Measured on a state WITHOUT that care (signs of m, ema and theta independent of the
gradient), where a few of the 1.2 M sums cancel: v 1 ulp (its terms are positive), m 14 930 ulp, theta 512, ema 502 --
while the largest ABSOLUTE errors of both paths against fp64 agreed to four digits (m 6.776e-08, theta 2.380e-07, both
paths).  On the conditioned states every quantity came out within 1 ulp.  The any-sign state is
still checked, against fp64: the yardstick there is the parent's path A, and the fused path's largest error may be at
most twice A's, for both states."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import weights_ref as R
from parity_log import record

DEV = "cuda"
LR, B1, B2, EPS, STEP, EMA_BETA, GRAD_SCALE = 2e-3, 0.9, 0.999, 1e-8, 3, 0.9, 0.5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def q(x):
    return x.to(torch.bfloat16).to(torch.float32)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)


def ulps(a, b):
    """largest distance of two fp32 tensors in units in the last place"""
    def key(t):
        i = t.detach().cpu().contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a) - key(b)).abs().max()) if a.numel() else 0


def step_record(dev=DEV):
    """the device edm_step_params record of step STEP, its bias corrections rounded as edm_adam_ema rounds them"""
    b1, b2 = float(np.float32(B1)), float(np.float32(B2))
    rec = np.zeros(12, dtype=np.float32)
    rec[4:9] = [LR, EMA_BETA, GRAD_SCALE, 1.0 - b1 ** STEP, math.sqrt(1.0 - b2 ** STEP)]
    return torch.from_numpy(rec.view(np.int32)).to(dev)


def _sign(t):
    return torch.where(t >= 0, 1.0, -1.0)


def random_theta(g, n, conditioned):
    t = torch.randn(n, generator=g)
    return _sign(t) * (0.25 + t.abs()) if conditioned else t


def random_state(g, theta, grad, conditioned):
    """random non-zero m, v and ema beside theta.  conditioned: every sum of the update has terms of one sign (m has the
    gradient's sign, ema its weight's); otherwise all signs are independent"""
    n = theta.numel()
    m = 0.01 + 0.1 * torch.randn(n, generator=g).abs()
    m = m * (_sign(grad.float()) if conditioned else _sign(torch.randn(n, generator=g)))
    v = 0.01 * torch.rand(n, generator=g) + 1e-4
    ema = theta * (0.9 + 0.2 * torch.rand(n, generator=g)) if conditioned else theta + 0.05 * torch.randn(n, generator=g)
    return dict(theta=theta, m=m, v=v, ema=ema)


def adam64(theta, g, m, v, ema):
    """the update of k_adam_ema in fp64 on fp32-valued scalars"""
    rec = step_record("cpu").numpy().view(np.float32).astype(np.float64)
    lr, beta, gs, bc1, bc2s = rec[4:9]
    b1, b2, eps = (float(np.float32(x)) for x in (B1, B2, EPS))
    g = g * gs
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    theta = theta - (lr / bc1) * m / (v.sqrt() / bc2s + eps)
    return theta, m, v, beta * ema + (1 - beta) * theta


# the smallest shapes of tests/test_wgrad3_gpu.py at B = 2 and 8x8 maps: a permuted layer, a layer with I < Cin, and a
# conv_in-like layer of 2 x 1 tiles.  Its K range is too short to split at this size (a share must be 16 stages long), so the
# K-split form of the finish has a group of its own below: the smallest layer of GROUP_KSPLIT that splits.
GROUP_ROWS = [
    dict(B=2, H=8, W=8, Cin=512, Cout=256, perm=True),
    dict(B=2, H=8, W=8, Cin=32, Cout=64, I=4, scale=0.7),
    dict(B=2, H=8, W=8, Cin=32, Cout=256, I=3),
]
GROUP_SPLIT = [
    dict(B=11, H=28, W=28, Cin=32, Cout=128, I=1),
    dict(B=2, H=8, W=8, Cin=64, Cout=64, perm=True),
]


def _arena(g, group):
    """a flat arena with the group's master weights at odd offsets between stretches that belong to no layer"""
    sizes = [kw["Cout"] * kw.get("I", kw["Cin"]) * 9 for kw in group]
    offs, pos = [], 37
    for s in sizes:
        offs.append(pos)
        pos += s + 5
    return offs, pos + 11


def _case(g, group, conditioned=True):
    offs, total = _arena(g, group)
    theta = random_theta(g, total, conditioned)
    layers = []
    for kw, off in zip(group, offs):
        B, H, W, Cin, Cout = kw["B"], kw["H"], kw["W"], kw["Cin"], kw["Cout"]
        I, scale = kw.get("I", Cin), kw.get("scale", 1.0)
        x = q(torch.randn(B, Cin, H, W, generator=g))
        x[:, I:] = 0.0
        gy = q(torch.randn(B, Cout, H, W, generator=g))
        p = torch.randperm(Cout, generator=g) if kw.get("perm") else None
        gy_master = gy
        if p is not None:
            gy_master = torch.empty_like(gy)
            gy_master[:, p] = gy
        w = theta[off:off + Cout * I * 9].view(Cout, I, 3, 3)
        w64 = w.double().clone().requires_grad_(True)
        F.conv2d(x[:, :I].double(), w64, padding=1).backward(gy_master.double())
        ref = R.project(scale * w64.grad, w.double())               # fp64 projected gradient of the master weight
        layers.append(types.SimpleNamespace(off=off, n=w.numel(), shape=w.shape, x=nhwc(x), dy=nhwc(gy), scale=scale,
                                            perm=None if p is None else p.to(torch.int32).to(DEV), ref=ref.reshape(-1)))
    g64 = torch.zeros(total, dtype=torch.float64)
    for L in layers:
        g64[L.off:L.off + L.n] = L.ref
    return layers, random_state(g, theta, g64, conditioned), g64


def _items(layers, theta, grad):
    return [(L.x, L.dy, theta[L.off:L.off + L.n].view(L.shape), grad[L.off:L.off + L.n].view(L.shape), L.perm, L.scale,
             True) for L in layers]


@pytest.mark.parametrize("name,group,conditioned", [("rows", GROUP_ROWS, True), ("rows-any-sign", GROUP_ROWS, False),
                                                    ("ksplit", GROUP_SPLIT, True)])
def test_apply_form_matches_finish_then_adam(ops, name, group, conditioned):
    g = torch.Generator().manual_seed(len(group) * 17 + 3)
    layers, state, g64 = _case(g, group, conditioned)
    if name == "ksplit":
        assert ops.wgrad3_plan_ksplit([(kw["B"], kw["H"], kw["W"], kw["Cin"], kw["Cout"]) for kw in group])[0] > 1
    dyn = step_record()
    A = {k: t.clone().to(DEV) for k, t in state.items()}
    Bq = {k: t.clone().to(DEV) for k, t in state.items()}
    grad_a, grad_b = torch.zeros_like(A["theta"]), torch.zeros_like(Bq["theta"])
    # path A, the parent's: finish into the zero arena, then the whole-arena optimizer pass
    ops.wgrad3_group(_items(layers, A["theta"], grad_a))
    ops.adam_ema(A["theta"], grad_a, A["m"], A["v"], A["ema"], LR, B1, B2, EPS, STEP, EMA_BETA, GRAD_SCALE, dyn=dyn,
                 zero_grad=True)
    # path B: the apply form alone
    done = ops.wgrad3_group_apply(_items(layers, Bq["theta"], grad_b), Bq["theta"], Bq["m"], Bq["v"], Bq["ema"], dyn,
                                  B1, B2, EPS)
    torch.cuda.synchronize()
    ops.check_health(DEV, "apply form on finite operands")
    assert done == [True] * len(layers)
    assert float(grad_b.abs().max()) == 0.0                         # the fused rows never write the gradient arena
    inside = torch.zeros(state["theta"].numel(), dtype=torch.bool)
    for L in layers:
        inside[L.off:L.off + L.n] = True
    worst_ulp, worst_ratio = 0, 0.0
    for k in ("theta", "m", "v", "ema"):
        a, b, s0 = A[k].cpu(), Bq[k].cpu(), state[k]
        assert torch.equal(b[~inside], s0[~inside]), f"{k}: the apply form touched elements outside its rows"
        assert torch.isfinite(b).all()
        u = ulps(a[inside], b[inside])
        print(f"[{name}] {k}: A vs B {u} ulp")
        worst_ulp = max(worst_ulp, u)
    if conditioned:
        record(f"fused_opt/apply_vs_two_kernels_ulp[{name}]", worst_ulp, 2)
    ref = dict(zip(("theta", "m", "v", "ema"), adam64(state["theta"].double(), g64, state["m"].double(),
                                                      state["v"].double(), state["ema"].double())))
    errs = {}
    for k in ("theta", "m", "v", "ema"):
        ea = float((A[k].cpu().double() - ref[k])[inside].abs().max())
        eb = float((Bq[k].cpu().double() - ref[k])[inside].abs().max())
        print(f"[{name}] {k}: max abs error vs fp64  A {ea:.3e}  B {eb:.3e}")
        errs[k] = (ea, eb)
        worst_ratio = max(worst_ratio, eb / max(ea, 1e-300))
    record(f"fused_opt/apply_err_over_parent_err[{name}]", worst_ratio, 2.0)
    assert not conditioned or worst_ulp <= 2, f"apply form vs finish + adam_ema: {worst_ulp} ulp"
    for k, (ea, eb) in errs.items():
        assert eb <= 2.0 * ea, f"{k}: fused error {eb:.3e} > 2 x parent's {ea:.3e}"


def test_apply_form_trips_the_health_word_on_a_nonfinite_gradient(ops):
    g = torch.Generator().manual_seed(5)
    layers, state, _ = _case(g, GROUP_ROWS[1:2])
    S = {k: t.clone().to(DEV) for k, t in state.items()}
    layers[0].dy[1, 3, 3, 7] = float("nan")
    ops.check_health(DEV, "before")
    ops.wgrad3_group_apply(_items(layers, S["theta"], torch.zeros_like(S["theta"])), S["theta"], S["m"], S["v"], S["ema"],
                           step_record(), B1, B2, EPS)
    with pytest.raises(ops.GraphCorruptionError, match="non-finite gradient"):
        ops.check_health(DEV, "poisoned dY")


# ------------------------------------------------------------------------------------------------ ranges kernel
N_ARENA = 5003
RANGE_SETS = {
    # (offset, numel) slices that are EXCLUDED; the kernel runs over the rest
    "odd": [(0, 3), (1500, 7), (4000, 1)],                 # ranges (3, 1497), (1507, 2493), (4001, 1002): several chunks each
    "random": None,                                        # drawn below
    "one-element": [(0, 2501), (2502, N_ARENA - 2502)],    # the only range is element 2501
    "empty-complement": [(0, N_ARENA)],
    "whole-arena": [],
}


@pytest.mark.parametrize("name", list(RANGE_SETS))
@pytest.mark.parametrize("with_ema", [True, False])
def test_ranges_form_matches_adam_ema(ops, name, with_ema):
    g = torch.Generator().manual_seed(41 + len(name))
    excl = RANGE_SETS[name]
    if excl is None:
        cuts = sorted(set(torch.randint(1, N_ARENA, (12,), generator=g).tolist()))
        excl = [(a, b - a) for a, b in zip(cuts[0::2], cuts[1::2])]
    grad = torch.randn(N_ARENA, generator=g)
    st = random_state(g, random_theta(g, N_ARENA, True), grad, True)        # (2 ulp: see the module docstring)
    st["grad"] = grad
    A = {k: t.clone().to(DEV) for k, t in st.items()}
    Bq = {k: t.clone().to(DEV) for k, t in st.items()}
    args = (LR, B1, B2, EPS, STEP, EMA_BETA, GRAD_SCALE)
    ops.adam_ema(A["theta"], A["grad"], A["m"], A["v"], A["ema"] if with_ema else None, *args, zero_grad=True)
    ranges, chunks = ops.adam_ranges_table(excl, N_ARENA, DEV)
    ops.adam_ema_ranges(Bq["theta"], Bq["grad"], Bq["m"], Bq["v"], Bq["ema"] if with_ema else None, ranges, chunks, *args,
                        zero_grad=True)
    torch.cuda.synchronize()
    inside = torch.ones(N_ARENA, dtype=torch.bool)
    for o, c in excl:
        inside[o:o + c] = False
    assert int(inside.sum()) == int(ranges[:, 1].sum()) if ranges.numel() else not inside.any()
    worst = 0
    for k in ("theta", "m", "v", "ema", "grad"):
        a, b = A[k].cpu(), Bq[k].cpu()
        assert torch.equal(b[~inside], st[k][~inside]), f"{k}: elements outside the ranges changed"
        if k == "grad":
            assert float(b[inside].abs().max()) == 0.0 if inside.any() else True
        elif k == "ema" and not with_ema:
            assert torch.equal(b, st[k])
        else:
            worst = max(worst, ulps(a[inside], b[inside]))
    print(f"[{name}, ema={with_ema}] ranges form vs k_adam_ema: {worst} ulp")
    record(f"fused_opt/ranges_vs_adam_ema_ulp[{name}]", worst, 2)
    assert worst <= 2


def test_ranges_table_rejects_overlapping_or_outlying_slices(ops):
    with pytest.raises(ValueError):
        ops.adam_ranges_table([(0, 10), (5, 10)], 100, DEV)
    with pytest.raises(ValueError):
        ops.adam_ranges_table([(95, 10)], 100, DEV)


# ------------------------------------------------------------------------------------------------ step level
def _batches(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [((0.5 * torch.randn(8, 3, 16, 16, generator=g)).to(DEV), torch.randint(0, 10, (8,), generator=g).to(DEV))
            for _ in range(n)]


def _run(monkeypatch, fused, batches):
    from test_graph_gpu import _build, _opt
    from tinyedm_amd.graph import CapturedTrainStep
    monkeypatch.setenv("EDM_FUSED_OPT", "1" if fused else "0")
    model, _ = _build()
    opt, base, sched = _opt(model)
    base.fuse_zero_grad = True              # as Trainer.fit and bench.py
    opt.zero_grad()
    step = CapturedTrainStep(model, opt)
    paths = []
    for b in batches:
        step(b)
        sched.step()
        paths.append(step.last_path)
    torch.cuda.synchronize()
    return step, opt, base, paths


def test_captured_step_fused_matches_unfused(monkeypatch):
    from test_graph_gpu import rel
    batches = _batches(6)
    step_u, opt_u, base_u, paths_u = _run(monkeypatch, False, batches)
    step_f, opt_f, base_f, paths_f = _run(monkeypatch, True, batches)
    assert paths_u == ["unfused"] * 6 and paths_f == ["fused"] * 6
    assert len(step_f._graphs) == 1 and len(step_u._graphs) == 1
    assert len(step_f.fused_slices) > 0
    at = dict(zip(base_f.arena.offsets, base_f.arena.params))
    assert all(at[o].numel() == n and at[o].dim() == 4 and tuple(at[o].shape[2:]) == (3, 3) for o, n in step_f.fused_slices)
    assert (base_f.step_count, opt_f.current_step) == (base_u.step_count, opt_u.current_step)
    for name, a, b, lim in (("theta", base_f.arena.theta, base_u.arena.theta, 2e-3), ("adam_m", base_f.m, base_u.m, 2e-2),
                            ("adam_v", base_f.v, base_u.v, 2e-2), ("ema", opt_f.ema_arena, opt_u.ema_arena, 2e-3)):
        e = rel(a, b)
        print(f"fused vs unfused captured step, {name}: rel {e:.3e}")
        record(f"fused_opt/captured_step/{name}_vs_unfused", e, lim)
        assert e <= lim, f"{name}: rel {e:.3e}"
    assert float(base_f.arena.grad.abs().max()) == 0.0
    assert float(base_u.arena.grad.abs().max()) == 0.0


def test_fused_step_trips_the_health_word_on_a_poisoned_dy(monkeypatch):
    from test_graph_gpu import _build, _opt
    from tinyedm_amd import networks as N
    from tinyedm_amd import ops
    from tinyedm_amd.graph import CapturedTrainStep
    monkeypatch.setenv("EDM_FUSED_OPT", "1")
    model, _ = _build(seed=4)
    opt, base, _ = _opt(model)
    base.fuse_zero_grad = True
    opt.zero_grad()
    step = CapturedTrainStep(model, opt)
    b = _batches(1, seed=2)[0]
    step(b)
    assert step.last_path == "fused"
    ops.check_health(DEV, "clean fused step")
    apply, hit = N._w3_apply, []

    def poisoned(fo, args):
        if not hit:
            args[0][1].view(-1)[5] = float("nan")           # one queued dY of a layer the finish is about to update
            hit.append(1)
        return apply(fo, args)

    monkeypatch.setattr(N, "_w3_apply", poisoned)
    step(b)
    assert hit and step.last_path == "fused"
    with pytest.raises(ops.GraphCorruptionError, match="non-finite gradient"):
        ops.check_health(DEV, "poisoned fused step")


def test_path_is_unfused_with_a_reducer_with_profiles_and_after_an_eval_mode_backward(monkeypatch):
    from test_graph_gpu import _build, _opt
    from tinyedm_amd.graph import CapturedTrainStep
    monkeypatch.setenv("EDM_FUSED_OPT", "1")
    model, _ = _build(pdrop=0.0)
    opt, base, _ = _opt(model)
    base.fuse_zero_grad = True
    opt.zero_grad()
    assert CapturedTrainStep(model, opt).path() == "fused"
    # a reducer (any world size): the all-reduce sits between the finish and the optimizer
    reducer = types.SimpleNamespace(active=True, world=1, capturable=lambda: True)
    assert CapturedTrainStep(model, opt, reducer=reducer).path() == "unfused"
    # the switch
    monkeypatch.setenv("EDM_FUSED_OPT", "0")
    assert CapturedTrainStep(model, opt).path() == "unfused"
    monkeypatch.setenv("EDM_FUSED_OPT", "1")
    # without the fused clear nobody vouches for a zero arena
    base.fuse_zero_grad = False
    assert CapturedTrainStep(model, opt).path() == "unfused"
    base.fuse_zero_grad = True
    # an eval-mode backward leaves gradients in the arena: that step takes the whole-arena pass (which consumes and
    # clears them, as before), the next one is fused again
    step = CapturedTrainStep(model, opt)
    b = _batches(1, seed=6)[0]
    step(b)
    assert step.last_path == "fused" and step.path() == "fused"
    model.eval()
    with torch.enable_grad():
        model.training_step(b, 1).backward()
    model.train()
    torch.cuda.synchronize()
    assert float(base.arena.grad.abs().max()) > 0.0
    assert step.path() == "unfused"
    step(b)
    torch.cuda.synchronize()
    assert step.last_path == "unfused" and float(base.arena.grad.abs().max()) == 0.0
    assert step.path() == "fused"
    step(b)
    assert step.last_path == "fused"
    # post-hoc EMA profiles: k_adam_ema_phema owns the pass
    base.attach_profiles([6.94])
    try:
        assert step.path() == "unfused"
    finally:
        base.phema = None
