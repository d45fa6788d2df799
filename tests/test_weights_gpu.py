"""The weight side against fp64 (tests/weights_ref.py): the multi-tensor weight preparation that every training step and
sampler evaluation starts with (k_weight_prep_multi through networks._PrepPlan: three normalisation paths, four pack
writers, ragged last workgroups), the per-tensor fallback, and the three kernels that reduce split-K partial sums and
project the gradient through the weight normalisation (k_wgrad_finish, k_wgrad_finish_multi, k_wgrad3_finish).

Values are held to elementwise, order-independent fp32 bounds (derived in weights_ref.py, factor-2 margin) and to a
relative L2 of 1e-5; packs are pure data movement of the kernel's own hat and are compared bit for bit.  The case tables,
and which code path each case is there for, are in weights_ref.py; tests/test_weights_ref_cpu.py checks on the CPU that an
fp32 emulation stays inside these bounds and that a list of plausible faults does not.  The worst ratio of error to bound
of every check goes to parity_log under weights/."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import weights_ref as R
from parity_log import record

DEV = "cuda"
bf16, f32 = torch.bfloat16, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def N(ops):
    from tinyedm_amd import networks
    return networks


def chk(name, what, got, ref, bound):
    r = R.check(got, ref, bound)
    print(f"weights/{name}: {what}: error / bound {r.worst:.3g}, rel L2 {r.l2:.3e}")
    record("weights/" + name, r.worst, 1.0)
    record("weights/" + name + " (rel L2)", r.l2, R.L2_LIMIT)
    assert r.finite, f"{name} {what}: non-finite result"
    assert r.worst <= 1.0, f"{name} {what}: error / bound = {r.worst:.3g}"
    assert r.l2 <= R.L2_LIMIT, f"{name} {what}: rel L2 {r.l2:.3e}"


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.numel() == b.numel() and torch.equal(a.flatten().view(torch.int16), b.flatten().view(torch.int16))


# ------------------------------------------------------------------------------------------------ a. multi-tensor prep
WANT_ALL = ("fwd", "dgrad", "hat")


def build_mod(N, m):
    w0, perm = R.prep_master(m.name)
    mod = N.Linear(m.I, m.O) if m.kind == "linear" else N.Conv2d(m.I, m.O, m.k)
    assert mod.weight.numel() == w0.numel()
    mod.weight = torch.nn.Parameter(w0.reshape(mod.weight.shape).clone().to(DEV))
    mod._ipad = m.ipad
    mod._perm = None if perm is None else perm.to(DEV)
    return mod


def make_plan(N, specs, want=WANT_ALL, frag=True):
    mods = [build_mod(N, m) for m in specs]
    plan = N._PrepPlan(mods, frag={mod: (True, True) for mod, m in zip(mods, specs) if m.frag and frag},
                       wants=[want] * len(mods), cat=[mod for mod, m in zip(mods, specs) if m.cat] or None)
    for c in plan.caches:                 # whatever the kernel leaves unwritten stays NaN
        for t in c:
            if t is not None:
                t.fill_(NAN)
    return mods, plan


def plan_rows(plan):
    """per module, the first packed rows of its workgroups"""
    out = {}
    for k, r in plan.groups.cpu().tolist():
        out.setdefault(k, []).append(r)
    return out


def is_frag(t):
    return bool(getattr(t, "_edm_frag", False))


def check_packs(m, name, hat, wf, wd, perm):
    """every pack is bf16(the kernel's own hat) pushed through the index map of its layout, bit for bit"""
    taps, Ipad = m.k * m.k, m.ipad or m.I
    hb = hat.detach().cpu().reshape(m.O, m.I, taps).to(bf16)
    assert tuple(wf.shape) == (taps, m.O, Ipad) and tuple(wd.shape) == (taps, m.I, m.O)
    assert same_bits(wf, R.pack_fwd_frag(hb) if is_frag(wf) else R.pack_fwd(hb, taps, Ipad, perm)), f"{name}: forward pack"
    assert same_bits(wd, R.pack_dgrad_frag(hb) if is_frag(wd) else R.pack_dgrad(hb, taps, perm)), f"{name}: dgrad pack"
    if not is_frag(wf):
        assert bool((wf[:, :, m.I:] == 0).all()), f"{name}: padding columns"


def check_module(m, mod, cache, training, name, rb):
    """one module of a plan after plan.run(training)"""
    w0, perm = R.prep_master(m.name)
    taps = m.k * m.k
    wf, wd, wh = cache
    master = mod.weight.detach().cpu().reshape(m.O, m.I, taps)
    hat = wh.detach().cpu().reshape(m.O, m.I, taps)
    z = m.O // 2
    assert bool((w0[z] == 0).all())
    if training:
        chk(f"prep_multi/{name} master", f"training rb={rb}", master, R.normalize_master(w0.double()), R.normalize_bound(w0.double()))
    else:
        assert torch.equal(master, w0), f"{name}: an evaluation changed the master weight"
    # hat against the master the kernel just stored: the two steps are bounded separately
    chk(f"prep_multi/{name} hat", f"training={training} rb={rb}", hat, R.effective(master.double()), R.effective_bound(master.double()))
    assert bool((master[z] == 0).all()) and bool((hat[z] == 0).all()), f"{name}: the zero row"
    check_packs(m, name, hat, wf, wd, perm)
    want_frag = m.frag and rb % 8 == 0 and m.O % 32 == 0 and m.I % 32 == 0
    assert is_frag(wf) == is_frag(wd) == want_frag, f"{name}: fragment flag with rb = {rb}"


@pytest.mark.parametrize("training", [True, False], ids=["training", "eval"])
def test_prep_multi_plan(N, training):
    specs = R.PREP_MODULES
    mods, plan = make_plan(N, specs)
    rows = plan_rows(plan)
    for k, m in enumerate(specs):
        rb = R.expected_rb(m.O, m.I * m.k * m.k)
        assert rows[k] == list(range(0, m.O, rb)), (m.name, rows[k])
    cat = [k for k, m in enumerate(specs) if m.cat]
    assert plan.wcat is not None and tuple(plan.wcat.shape) == (sum(specs[k].O for k in cat), specs[cat[0]].I)
    plan.wcat.fill_(NAN)
    plan.run(training)
    torch.cuda.synchronize()
    for k, (m, mod) in enumerate(zip(specs, mods)):
        check_module(m, mod, plan.caches[k], training, m.name, R.expected_rb(m.O, m.I * m.k * m.k))
    # wcat: the hats of the `cat` Linears back to back, in the order given
    assert torch.equal(plan.wcat, torch.cat([plan.caches[k][2] for k in cat])) and bool(torch.isfinite(plan.wcat).all())
    assert all(plan.caches[k][2].data_ptr() == plan.wcat.data_ptr() + 4 * specs[cat[0]].I * sum(specs[j].O for j in cat if j < k)
               for k in cat)
    # a second plan over the same weights without hat, run as an evaluation so that the master stays as plan 1 left it:
    # the same rows summed in the same order give the same hat, so the packs must agree bit for bit
    plan2 = N._PrepPlan(mods, frag={mod: (True, True) for mod, m in zip(mods, specs) if m.frag}, wants=[("fwd", "dgrad")] * len(mods))
    for c in plan2.caches:
        assert c[2] is None
        c[0].fill_(NAN), c[1].fill_(NAN)
    before = [mod.weight.detach().clone() for mod in mods]
    plan2.run(False)
    torch.cuda.synchronize()
    for m, mod, w_, c, c2 in zip(specs, mods, before, plan.caches, plan2.caches):
        assert torch.equal(mod.weight.detach(), w_)
        assert is_frag(c2[0]) == is_frag(c[0]) and is_frag(c2[1]) == is_frag(c[1])
        assert same_bits(c2[0], c[0]) and same_bits(c2[1], c[1]), f"{m.name}: packs without hat differ"


@pytest.mark.parametrize("m", R.PREP_RB_MODULES, ids=[m.name for m in R.PREP_RB_MODULES])
def test_prep_multi_rows_per_workgroup(N, monkeypatch, m):
    """the same tensor with 8, 4, 2 and 1 rows per workgroup (the tile size shrunk): rb = 8 runs the fragment writers with
    rl0 in {0, 8, 16, 24} and both ks / g halves of the dgrad writer; below 8 the plan must drop the fragment flag"""
    n = m.I * m.k * m.k
    for rb in R.PREP_RBS:
        monkeypatch.setattr(N, "PREP_TILE_BYTES", rb * n * 2)
        for training in (True, False):
            mods, plan = make_plan(N, [m])
            assert plan_rows(plan)[0] == list(range(0, m.O, rb)) and plan.lds_bytes == rb * n * 2
            plan.run(training)
            torch.cuda.synchronize()
            check_module(m, mods[0], plan.caches[0], training, f"{m.name} rb={rb}", rb)


def test_weight_prep_per_tensor(ops):
    """the per-tensor fallback (k_weight_prep) on the same masters: hat and the renormalised master inside the same bounds,
    plain packs that are bf16(its own hat) bit for bit"""
    for m in R.PREP_MODULES:
        w0, perm = R.prep_master(m.name)
        taps = m.k * m.k
        p = None if perm is None else perm.to(DEV)
        for training in (True, False):
            w = w0.clone().to(DEV)
            wf, wd, wh = ops.weight_prep(w, taps, Ipad=m.ipad, want_hat=True, perm=p, normalize_inplace=training)
            torch.cuda.synchronize()
            master = w.cpu()
            if training:
                chk(f"prep_single/{m.name} master", "training", master, R.normalize_master(w0.double()), R.normalize_bound(w0.double()))
            else:
                assert torch.equal(master, w0)
            hat = wh.cpu().reshape(m.O, m.I, taps)
            chk(f"prep_single/{m.name} hat", f"training={training}", hat, R.effective(master.double()), R.effective_bound(master.double()))
            assert bool((hat[m.O // 2] == 0).all()) and bool((master[m.O // 2] == 0).all())
            check_packs(m, m.name + " (per tensor)", hat, wf, wd, perm)


@pytest.mark.parametrize("O,I", [(64, 256), (256, 256)])
def test_fragment_pack_is_what_conv3x3_s_reads(ops, N, O, I):
    """k_conv3x3_s with the fragment-major pack and with the plain pack of the same values gives the same output, bit for
    bit: the index map of weights_ref is the one the consumer reads.  Forward pack on an 8x8 map; the dgrad pack (a forward
    pack of the transposed conv) where that conv is one the kernel covers (O % 256 == 0)."""
    g = R.gen(14, O, I)
    w0 = R.master_rows(g, O, I * 9).reshape(O, I, 3, 3)
    packs = {}
    for frag in (True, False):
        mod = N.Conv2d(I, O, 3)
        mod.weight = torch.nn.Parameter(w0.clone().to(DEV))
        plan = N._PrepPlan([mod], frag={mod: (frag, frag)}, wants=[WANT_ALL])
        plan.run(False)
        packs[frag] = plan.caches[0]
    torch.cuda.synchronize()
    assert is_frag(packs[True][0]) and is_frag(packs[True][1]) and not is_frag(packs[False][0])
    assert torch.equal(packs[True][2], packs[False][2])
    hb = packs[True][2].cpu().reshape(O, I, 9).to(bf16)
    assert same_bits(packs[False][0], R.pack_fwd(hb, 9, I, None)) and same_bits(packs[True][0], R.pack_fwd_frag(hb))
    assert same_bits(packs[False][1], R.pack_dgrad(hb, 9, None)) and same_bits(packs[True][1], R.pack_dgrad_frag(hb))
    B, H, W = 2, 8, 8
    old = ops.IGEMM_VERSION
    ops.IGEMM_VERSION = 5
    try:
        ran = 0
        for which, Cin, Cout in ((0, I, O), (1, O, I)):
            if ops._conv_plan(B, H, W, Cin, Cout, 9, 5) & 0xff != 5:
                continue
            x = torch.randn(B, H, W, Cin, generator=g).to(bf16).to(DEV)
            y_frag = ops.conv_igemm(x, packs[True][which], 9)
            y_plain = ops.conv_igemm(x, packs[False][which], 9)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(y_plain.float()).all()) and bool((y_plain != 0).any())
            assert same_bits(y_frag, y_plain), f"{'dgrad' if which else 'forward'} pack {O}x{I}"
            ran += 1
    finally:
        ops.IGEMM_VERSION = old
    if not ran:
        pytest.skip("k_conv3x3_s does not cover this shape")


# ------------------------------------------------------------------------------------------------ b. per-tensor finish
def dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("case", R.FINISH_CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_finish_against_fp64(ops, case):
    for (perm, acc, scale) in R.FINISH_VARIANTS:
        c = R.finish_case(*case, perm, acc, scale)
        out = c.g0.clone().to(DEV) if acc else None
        got = ops.wgrad_finish(dev(c.slabs), dev(c.w), c.taps, c.I, perm=dev(c.perm), scale=scale, out=out)
        torch.cuda.synchronize()
        assert out is None or got.data_ptr() == out.data_ptr()
        chk("finish/" + "x".join(map(str, case)), f"perm={perm} accumulate={acc} scale={scale}", got, c.ref, c.bound)


# ------------------------------------------------------------------------------------------------ c. multi-tensor finish
def run_multi(ops, cases, tag):
    items = []
    for c in cases:
        # without accumulate the old contents must be overwritten, not added to
        grad = c.g0.clone() if c.accumulate else torch.full_like(c.g0, NAN)
        items.append((dev(c.slabs), dev(c.w), grad.to(DEV), dev(c.perm), c.taps, c.I, c.scale, c.accumulate))
    ops.wgrad_finish_multi(items)
    torch.cuda.synchronize()
    for k, (c, it) in enumerate(zip(cases, items)):
        S, taps, O, Ipad = c.slabs.shape
        chk(f"finish_multi/{tag}", f"item {k} (S={S} taps={taps} O={O} I={c.I} Ipad={Ipad} perm={c.perm is not None} "
            f"accumulate={c.accumulate} scale={c.scale})", it[2], c.ref, c.bound)


def test_wgrad_finish_multi_against_fp64(ops):
    cases = [R.multi_case(k, c) for k, c in enumerate(R.MULTI_CASES)]
    assert bool((cases[R.MULTI_ZERO_O1].w == 0).all())
    run_multi(ops, cases, "fifteen")


def test_wgrad_finish_multi_second_launch(ops):
    run_multi(ops, [R.multi_case(k, c, salt=2) for k, c in enumerate(R.MULTI_41)], "forty-one")


# ------------------------------------------------------------------------------------------------ d. k_wgrad3_finish
@pytest.mark.parametrize("name", R.W3_REAL_GROUPS)
def test_wgrad3_finish_with_a_real_master(ops, name):
    """the raw gradient of these integer operands is exact (tests/test_conv_exact_gpu.py), so the whole error is the
    projection's: master rows of every scale, one zero row, correlated with the gradient"""
    group, layers = R.w3_real_group(name)
    if name == "late":
        L = layers[0]
        if not ops.wgrad3_supported(L.x, L.dy, L.wm.shape[1]):
            pytest.skip("the grouped 3x3 weight gradient does not cover the late-load layer")
        assert L.wm.shape[1] * 9 > 7168
    grads = [L.g0.clone().to(DEV) for L in layers]
    ops.wgrad3_group([(L.x.to(DEV), L.dy.to(DEV), L.wm.to(DEV), gr, dev(L.perm), L.scale, L.accumulate)
                      for L, gr in zip(layers, grads)])
    torch.cuda.synchronize()
    for k, (kw, L, gr) in enumerate(zip(group, layers, grads)):
        chk(f"wgrad3_finish/{name}", f"layer {k} {kw}", gr, L.ref, R.w3_bound(L))
