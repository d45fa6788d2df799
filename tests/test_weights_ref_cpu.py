"""tests/weights_ref.py checked without a GPU: the references against fp64 autograd and against the documented index
formulas, an fp32 emulation of every operation that must stay inside the bounds on every case tests/test_weights_gpu.py
runs (three summation orders), and a list of plausible faults that must each fall outside them on those same inputs --
if one passed, the inputs would be too tame for the GPU test to mean anything."""
import math

import pytest
import torch

import weights_ref as R

f32, f64 = torch.float32, torch.float64
ORDERS = ["sequential", "reversed", "pairwise64"]


# ------------------------------------------------------------------------------------------------ the references
def test_project_is_the_gradient_of_effective():
    g = R.gen(1)
    for O, n in [(5, 10), (7, 36), (4, 2304)]:
        w = R.master_rows(g, O, n).double()
        live = w.norm(dim=1) > 0
        a = torch.randn(O, n, generator=g, dtype=f64) + R.BETA * w
        w_ = w.clone().requires_grad_(True)
        (R.effective(w_) * a).sum().backward()
        got, ref = R.project(a, w)[live], w_.grad[live]
        assert ((got - ref).abs() <= 1e-12 * ref.abs().max(dim=1, keepdim=True).values).all()


def test_project_of_a_zero_row_is_the_one_sided_limit():
    g = R.gen(2)
    n = 36
    a = torch.randn(1, n, generator=g, dtype=f64)
    z = R.project(a, torch.zeros(1, n, dtype=f64))
    assert torch.allclose(z, a / (R.EPS * math.sqrt(n)), rtol=1e-15, atol=0.0)
    tiny = torch.randn(1, n, generator=g, dtype=f64)
    tiny = tiny / tiny.pow(2).mean().sqrt() * 1e-12
    assert ((R.project(a, tiny) - z).abs() <= 1e-7 * z.abs().max()).all()      # rms / eps = 1e-8 away
    assert torch.equal(R.normalize_master(torch.zeros(2, n, dtype=f64)), torch.zeros(2, n, dtype=f64))


def test_finish_places_rows_by_perm_and_skips_the_padding():
    S, taps, O, I, Ipad = 3, 9, 4, 2, 5
    slabs = torch.full((S, taps, O, Ipad), float("nan"), dtype=f64)
    slabs[..., :I] = torch.arange(S * taps * O * I, dtype=f64).view(S, taps, O, I)
    perm = torch.tensor([2, 0, 3, 1], dtype=torch.int32)
    a = R.slab_sum(slabs, I, taps, perm, 0.5)
    for r in range(O):
        for i in range(I):
            for t in range(taps):
                assert a[perm[r], i, t] == 0.5 * slabs[:, t, r, i].sum()
    w = R.master_rows(R.gen(3), O, I * taps).double().view(O, I, taps)
    g0 = torch.ones(O, I, taps, dtype=f64)
    assert torch.equal(R.finish(slabs, w, I, taps, perm, 0.5, g0), g0 + R.project(a, w))


def test_plain_packs_follow_their_formulas():
    O, I, taps, Ipad = 5, 3, 9, 8
    hat = torch.arange(O * I * taps, dtype=f64).view(O, I, taps) + 1
    perm = torch.tensor([3, 0, 4, 1, 2], dtype=torch.int32)
    for p in (None, perm):
        wf, wd = R.pack_fwd(hat, taps, Ipad, p), R.pack_dgrad(hat, taps, p)
        assert tuple(wf.shape) == (taps, O, Ipad) and tuple(wd.shape) == (taps, I, O)
        for r in range(O):
            mo = r if p is None else int(p[r])
            for i in range(I):
                for t in range(taps):
                    assert wf[t, r, i] == hat[mo, i, t] and wd[taps - 1 - t, i, r] == hat[mo, i, t]
        assert bool((wf[:, :, I:] == 0).all())


@pytest.mark.parametrize("O,I", [(32, 64), (64, 32), (64, 256)])
def test_fragment_packs_follow_the_documented_layout(O, I):
    taps = 9
    hat = torch.arange(O * I * taps, dtype=f64).view(O, I, taps)
    co, ci, t = torch.meshgrid(torch.arange(O), torch.arange(I), torch.arange(taps), indexing="ij")

    def offset(t, c, cb, ks, lane, e, NC, NCB):
        return ((((t * NC + c) * NCB + cb) * 2 + ks) * 64 + lane) * 8 + e

    off_f = offset(t, ci >> 5, co >> 5, (ci >> 4) & 1, 32 * ((ci >> 3) & 1) + (co & 31), ci & 7, I >> 5, O >> 5)
    off_d = offset(taps - 1 - t, co >> 5, ci >> 5, (co >> 4) & 1, 32 * ((co >> 3) & 1) + (ci & 31), co & 7, O >> 5, I >> 5)
    for pack, off in ((R.pack_fwd_frag(hat), off_f), (R.pack_dgrad_frag(hat), off_d)):
        assert pack.numel() == hat.numel() and off.unique().numel() == hat.numel()
        assert torch.equal(pack.flatten()[off], hat)


def test_case_tables_reach_the_paths_they_name():
    """the host-side choices (rows per workgroup, s-groups) that the comments of the case tables rely on"""
    by = {m.name: m for m in R.PREP_MODULES}
    n_of = lambda name: by[name].I * by[name].k ** 2
    rb = lambda name: R.expected_rb(by[name].O, n_of(name))
    assert [rb(k) for k in ("rb2_ragged_group", "groups_32_4", "long_n5184", "long_n13824", "frag_64x256")] == [2, 32, 4, 2, 16]
    assert by["rb2_ragged_group"].O % 2 == 1 and by["groups_32_4"].O - 32 == 4
    # the three normalisation paths: registers (n % 4 == 0, n <= 5120), the three-pass loop, the scalar loop
    assert n_of("scalar_n27_padded") % 4 and n_of("long_scalar_n4095") % 4 and n_of("lin10") % 4
    assert n_of("regs_ragged_n36") % 4 == 0 and n_of("regs_ragged_n36") % 256
    assert n_of("regs_last_n5120") == 20 * 256 and n_of("long_first_n5124") == 20 * 256 + 4
    assert n_of("long_n5184") // 4 > 2 * 512 and (n_of("long_n5184") // 4) % 512                  # three trips, ragged last
    assert by["ipad10_scalar_fwd"].I % 8 and by["scalar_n27_padded"].ipad % 8 == 0
    for m in R.PREP_RB_MODULES:
        n = m.I * 9
        assert [R.expected_rb(m.O, n, rb * n * 2) for rb in R.PREP_RBS] == R.PREP_RBS
    G = {c: R.finish_G(c[0], c[1], c[3], c[4]) for c in R.FINISH_CASES}
    assert G[(1, 1, 16, 64, 64)] == 1 and G[(2, 1, 16, 64, 64)] == 2 and G[(3, 9, 8, 32, 32)] == 2
    # S <= 3 takes G = 2 up to rows of 2048 floats (E4 * 2 G <= 1024 holds with equality there); only longer rows get G = 1,
    # and a row of at most 16384 floats never needs a second trip of 4 x 1024 vectors
    assert G[(3, 1, 8, 2048, 2048)] == 2 and G[(3, 1, 4, 4096, 4096)] == 1 and G[(2, 9, 3, 1536, 1536)] == 1
    assert 4096 // 4 * 1 <= 4 * 1024 and 2 * 1024 < 13824 // 4 < 4 * 1024       # a full trip, and one whose last vectors are idle
    assert G[(4, 1, 16, 256, 256)] == 4 and G[(8, 1, 16, 64, 64)] == 8
    # the unrolled trip (s + 7 G < S) followed by a tail: S = 20, G = 2 -> s = 0 .. 14 unrolled, 16 and 18 in the tail; rows
    # of 512 floats get G = 8 (128 vectors x 8 = 1024) and never enter the unrolled trip, rows of 2048 floats get G = 2
    assert G[(20, 1, 16, 512, 512)] == 8 and not 0 + 7 * 8 < 20
    assert G[(20, 1, 8, 2048, 2048)] == 2 and 0 + 7 * 2 < 20 and not 16 + 7 * 2 < 20
    assert G[(37, 9, 8, 64, 64)] == 4 and not 0 + 7 * 4 < 37 - 8 * 4 and 0 + 7 * 4 < 37
    assert 48 * 1024 < 13824 * 4 <= 64 * 1024                                 # the longest rows of the ImageNet nets
    assert len(R.MULTI_41) == 41 and [c[2] for c in R.MULTI_CASES[8:13]] == [1] * 5
    assert [c[3] * c[1] <= 2 * 512 for c in R.MULTI_CASES[-2:]] == [True, False]   # prefetched / late-load form
    assert R.W3_LATE_LAYER["Cin"] * 9 > 28 * 256


# ------------------------------------------------------------------------------------------------ fp32 emulation
def fsum(x, order):
    """fp32 sum over the last axis with every partial sum rounded to fp32, in the given order"""
    assert x.dtype == f32
    if order == "reversed":
        return fsum(x.flip(-1), "sequential")
    if order == "sequential":
        acc = torch.zeros(x.shape[:-1], dtype=f32)
        for j in range(x.shape[-1]):
            acc = acc + x[..., j]
        return acc
    m = x.shape[-1]
    pad = (-m) % 64
    if pad:
        x = torch.cat([x, torch.zeros(x.shape[:-1] + (pad,), dtype=f32)], dim=-1)
    lanes = fsum(x.reshape(x.shape[:-1] + (-1, 64)).transpose(-1, -2).contiguous(), "sequential")   # lane l: x[l::64]
    while lanes.shape[-1] > 1:
        h = lanes.shape[-1] // 2
        lanes = lanes[..., :h] + lanes[..., h:]
    return lanes[..., 0]


EPS32 = torch.tensor(1e-4, dtype=f32)


def emu_normalize(w, order, training):
    """(stored master, hat) in fp32: the master is renormalised first when training, hat comes from the stored master"""
    w = w.reshape(w.shape[0], -1)
    n = w.shape[1]
    rsn = torch.rsqrt(torch.tensor(float(n), dtype=f32))
    m = w
    if training:
        d = EPS32 + torch.sqrt(fsum(w * w, order)) * rsn
        m = w * (1.0 / d)[:, None]
    d = EPS32 + torch.sqrt(fsum(m * m, order)) * rsn
    return m, m * (rsn / d)[:, None]


def emu_project(a, w, order):
    n = w.shape[1]
    dot, ss = fsum(a * w, order), fsum(w * w, order)
    rn, sqn = torch.sqrt(ss), torch.sqrt(torch.tensor(float(n), dtype=f32))
    d = EPS32 + rn / sqn
    c0 = 1.0 / (d * sqn)
    c1 = torch.where(rn > 0, dot / (d * rn * sqn), torch.zeros_like(dot))
    return c0[:, None] * (a - w * c1[:, None])


def emu_finish(c, order):
    S, taps, O, Ipad = c.slabs.shape
    a_packed = fsum(c.slabs[..., :c.I].permute(1, 2, 3, 0).contiguous(), order) * torch.tensor(c.scale, dtype=f32)
    a = torch.empty(O, c.I, taps, dtype=f32)
    a[R._perm_index(c.perm, O)] = a_packed.permute(1, 2, 0)
    v = emu_project(a.reshape(O, -1), c.w.reshape(O, -1), order).reshape(O, c.I, taps)
    return c.g0 + v if c.accumulate else v


def _inside(what, got, ref, bound):
    r = R.check(got, ref, bound)
    assert r.ok, f"{what}: error / bound = {r.worst:.3g}, rel L2 {r.l2:.3e}"
    return r.worst


@pytest.mark.parametrize("order", ORDERS)
def test_emulated_normalisation_is_inside_the_bounds(order):
    worst = 0.0
    for m in R.PREP_MODULES + R.PREP_RB_MODULES:
        w0, _ = R.prep_master(m.name)
        for training in (True, False):
            master, hat = emu_normalize(w0, order, training)
            shape = w0.shape
            if training:
                worst = max(worst, _inside(f"{m.name} master", master.view(shape), R.normalize_master(w0.double()),
                                           R.normalize_bound(w0.double())))
                assert bool((master[m.O // 2] == 0).all())
            else:
                assert torch.equal(master.view(shape), w0)
            worst = max(worst, _inside(f"{m.name} hat", hat.view(shape), R.effective(master.view(shape).double()),
                                       R.effective_bound(master.view(shape).double())))
    assert 0.0 < worst < 0.5            # the bound has the margin of 2 it was given, and is not orders of magnitude loose


def _all_finish_cases():
    for c in R.FINISH_CASES:
        for v in R.FINISH_VARIANTS:
            yield ("finish", c + v), R.finish_case(*c, *v)
    for k, c in enumerate(R.MULTI_CASES):
        yield ("multi", k, c), R.multi_case(k, c)
    for k, c in enumerate(R.MULTI_41):
        yield ("multi41", k, c), R.multi_case(k, c, salt=2)


@pytest.mark.parametrize("order", ORDERS)
def test_emulated_finish_is_inside_the_bounds(order):
    worst = 0.0
    for what, c in _all_finish_cases():
        O = c.w.shape[0]
        assert bool(torch.isnan(c.slabs[..., c.I:]).all())                                  # NaN padding
        assert O == 1 or int((c.w.reshape(O, -1) == 0).all(dim=1).sum()) == 1                # one all-zero master row
        worst = max(worst, _inside(str(what), emu_finish(c, order), c.ref, c.bound))
    assert 0.0 < worst < 0.5


@pytest.mark.parametrize("name", R.W3_REAL_GROUPS)
def test_emulated_wgrad3_projection_is_inside_the_bounds(name):
    group, layers = R.w3_real_group(name)
    for kw, L in zip(group, layers):
        Cout = L.wm.shape[0]
        assert torch.equal(L.G, L.G.round()) and bool((L.wm[Cout // 2] == 0).all())
        a = (L.G.float() * torch.tensor(L.scale, dtype=f32)).reshape(Cout, -1)
        for order in ORDERS[1:]:
            v = emu_project(a, L.wm.reshape(Cout, -1), order).reshape(L.wm.shape)
            _inside(f"{name} {kw} {order}", L.g0 + v if L.accumulate else v, L.ref, R.w3_bound(L))


# ------------------------------------------------------------------------------------------------ sharpness
def _wrong_d(w, fault, eps=R.EPS):
    """(d, sqrt(n) as used for w_hat) of a faulty normalisation"""
    n = w.shape[1]
    rn, sqn = w.norm(dim=1, keepdim=True), math.sqrt(n)
    if fault == "eps_dropped":
        return (rn / sqn).clamp_min(1e-300), sqn
    if fault == "eps_under_sqrt":
        return torch.sqrt(eps + rn * rn / n), sqn
    if fault == "sqrt_n_once":
        return eps + rn / sqn, 1.0
    raise KeyError(fault)


NORM_FAULTS = ["eps_dropped", "eps_under_sqrt", "sqrt_n_once"]


def _outside(got, ref, bound):
    return not R.check(got, ref, bound).ok


@pytest.mark.parametrize("fault", NORM_FAULTS)
def test_a_wrong_normalisation_is_outside_the_bounds(fault):
    """on every module of the prep tables: the stored master (eps faults) and hat (all three)"""
    for m in R.PREP_MODULES + R.PREP_RB_MODULES:
        w0 = R.prep_master(m.name)[0].double()
        w = w0.reshape(m.O, -1)
        d, sqn = _wrong_d(w, fault)
        if fault != "sqrt_n_once":
            assert _outside((w / d).view(w0.shape), R.normalize_master(w0), R.normalize_bound(w0)), (fault, m.name, "master")
        assert _outside((w / d / sqn).view(w0.shape), R.effective(w0), R.effective_bound(w0)), (fault, m.name, "hat")


def _wrong_finish(c, fault):
    """fp64 result of a finish with one fault, or None where the fault cannot show on this case"""
    S, taps, O, Ipad = c.slabs.shape
    I, perm, scale = c.I, c.perm, c.scale
    slabs = c.slabs.double()
    base = (c.g0 if c.accumulate else torch.zeros_like(c.g0)).double()
    w = c.w.double()
    rows = lambda t: t.reshape(O, -1)
    a = R.slab_sum(slabs, I, taps, perm, scale)
    n = I * taps
    rn, sqn = rows(w).norm(dim=1, keepdim=True), math.sqrt(n)
    d = R.EPS + rn / sqn
    dot = (rows(a) * rows(w)).sum(dim=1, keepdim=True)
    live = rn > 0
    rms = rn / sqn
    if fault in NORM_FAULTS + ["c1_without_rn", "w_hat_for_w"] and not bool(((rms > 0) & (rms <= 1e-2)).any()):
        return None                                # (tensors of one or two rows: eps may not matter to any of them)

    def proj(a_, d_=d, sq0=sqn, c1=None):
        c1 = torch.where(live, dot / (d_ * rn.clamp_min(1e-300) * sqn), torch.zeros_like(dot)) if c1 is None else c1
        return (1.0 / (d_ * sq0) * (rows(a_) - rows(w) * c1)).view(w.shape)

    if fault in NORM_FAULTS:
        d_, sq0 = _wrong_d(rows(w), fault)
        if fault == "eps_dropped":                 # (a zero row would divide by zero: the kernel's guard stays)
            d_ = torch.where(live, d_, torch.full_like(d_, R.EPS))
        return base + proj(a, d_, sq0)
    if fault == "c1_without_rn":
        return base + proj(a, c1=torch.where(live, dot / (d * sqn), torch.zeros_like(dot)))
    if fault == "w_hat_for_w":
        return base + R.project(a, R.effective(w))
    if fault == "scale_not_on_a":
        return None if scale == 1.0 else base + proj(a / scale)
    if fault == "perm_inverted":
        inv = None if perm is None else torch.argsort(perm.long())
        return None if perm is None or torch.equal(inv, perm.long()) else R.finish(slabs, w, I, taps, inv, scale, base)
    if fault == "last_slab_left_out":
        return None if S == 1 else R.finish(slabs[:S - 1], w, I, taps, perm, scale, base)
    if fault == "padding_read":                    # rows taken I apart instead of Ipad apart
        if Ipad == I or O == 1:
            return None
        dense = slabs.reshape(S, taps, O * Ipad)[..., :O * I].reshape(S, taps, O, I)
        return R.finish(dense, w, I, taps, perm, scale, base)
    if fault == "accumulate_ignored":
        return c.ref - base if c.accumulate else None
    raise KeyError(fault)


FINISH_FAULTS = NORM_FAULTS + ["c1_without_rn", "w_hat_for_w", "scale_not_on_a", "perm_inverted", "last_slab_left_out",
                               "padding_read", "accumulate_ignored"]


@pytest.mark.parametrize("fault", FINISH_FAULTS)
def test_a_wrong_finish_is_outside_the_bounds(fault):
    """on EVERY case of the finish tables on which the fault can show at all"""
    hit = 0
    for what, c in _all_finish_cases():
        got = _wrong_finish(c, fault)
        if got is None:
            continue
        hit += 1
        assert _outside(got, c.ref, c.bound), (fault, what)
    assert hit >= 8


@pytest.mark.parametrize("fault", NORM_FAULTS + ["c1_without_rn", "w_hat_for_w"])
def test_a_wrong_wgrad3_projection_is_outside_the_bounds(fault):
    for name in ("single", "late"):
        for L in R.w3_real_group(name)[1]:
            Cout, I = L.wm.shape[:2]
            slabs = (L.G.reshape(Cout, I, 9).permute(2, 0, 1))[None].float()         # one exact slab, packed order
            c = R.FinishCase(slabs, L.wm.reshape(Cout, I, 9), L.g0.reshape(Cout, I, 9), None, I, 9, L.scale, L.accumulate,
                             L.ref.reshape(Cout, I, 9), R.w3_bound(L).reshape(Cout, I, 9))
            assert torch.equal(R.finish(slabs.double(), c.w.double(), I, 9, None, L.scale, c.g0 if L.accumulate else 0 * c.g0), c.ref)
            assert _outside(_wrong_finish(c, fault), c.ref, c.bound), (fault, name)


def test_wrong_packs_differ_from_the_right_ones():
    """packs are compared bit for bit, so a fault shows as soon as it moves one element: a perm inverted, dgrad taps not
    flipped, padding columns that hold data, the last row of a ragged group left as it was"""
    for m in R.PREP_MODULES + R.PREP_RB_MODULES:
        w0, perm = R.prep_master(m.name)
        taps, Ipad = m.k * m.k, m.ipad or m.I
        hat = R.effective(w0.double()).to(torch.bfloat16)
        wf, wd = R.pack_fwd(hat, taps, Ipad, perm), R.pack_dgrad(hat, taps, perm)
        if perm is not None:
            inv = torch.argsort(perm.long())
            assert not torch.equal(R.pack_fwd(hat, taps, Ipad, inv), wf) and not torch.equal(R.pack_dgrad(hat, taps, inv), wd)
        if taps > 1:
            assert not torch.equal(R.pack_dgrad(hat.flip(2), taps, perm), wd)
            if m.O % 32 == 0 and m.I % 32 == 0:
                assert not torch.equal(R.pack_dgrad_frag(hat.flip(2)), R.pack_dgrad_frag(hat))
                assert not torch.equal(R.pack_fwd_frag(hat).reshape(taps, m.O, m.I), wf)      # the two layouts differ
        if Ipad > m.I:
            wrong = hat.reshape(m.O, -1)[R._perm_index(perm, m.O)].reshape(m.O, m.I, taps)
            wrong = torch.cat([wrong, wrong[:, :Ipad - m.I]], dim=1).permute(2, 0, 1)         # padding filled with data
            assert not torch.equal(wrong, wf) and bool((wf[:, :, m.I:] == 0).all())
        rb = R.expected_rb(m.O, m.I * taps)
        if m.O % rb:                                                                          # ragged last group
            stale = hat.clone()
            stale[m.O - 1] = w0[m.O - 1].to(torch.bfloat16)                                   # last row never rewritten
            assert not torch.equal(R.pack_fwd(stale, taps, Ipad, perm), wf)
            left = w0.double().clone()
            norm = R.normalize_master(w0.double())
            left[:m.O - 1] = norm[:m.O - 1]
            assert _outside(left, norm, R.normalize_bound(w0.double())), m.name
