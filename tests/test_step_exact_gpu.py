"""The training step's own fp32 kernels against exact restatements (tests/step_ref.py): the Diffuser's two Philox streams
and its arithmetic (csrc/optim.hip k_diffuse, k_diffuse_given), the dropout mask every saved-activation test takes as its
truth (csrc/common.h dropout_keep8 behind edm_dropout_mask) and every form of the fused Adam + EMA pass (plain, `dyn`,
ranges, post-hoc EMA profiles, guarded) against fp64, elementwise, in bounds counted from the roundings of each
expression.  Shapes are the smallest that reach each path: one element, quads that straddle samples, partial last quads,
and 4 * 4096 * 256 + 5 elements (8 * 4096 * 256 + 8 for the mask), where the grid-stride loop makes its second trip.

Measured figures are recorded under step_exact/... (tests/parity_log.py) and printed before they are asserted."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import step_ref as S
from parity_log import record

DEV = "cuda"
U = 2.0 ** -24
SEEDS = [0x0BADC0FFEE123457, 1]          # high word set / high word zero
STEPS = [0, 3, 2 ** 32 - 1]
PS = [(-1.2, 1.2), (0.4, 2.0)]           # (P_mean, P_std)
STRIDE2 = 4 * 4096 * 256                 # elements one trip of a 4096-workgroup grid of quads covers


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def _edges(total, edge):
    """every index of a small array, the first and the last `edge` of a large one"""
    if total <= 2 * edge:
        return np.arange(total)
    return np.concatenate([np.arange(edge), np.arange(total - edge, total)])


def _take(t, idx):
    """fp64 numpy copy of the flat elements idx of a device tensor"""
    return t.reshape(-1)[torch.from_numpy(idx).to(t.device)].double().cpu().numpy()


def _ratio(err, bound):
    return float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def _step_record(seed, step):
    """a device edm_step_params record holding only (step, seed)"""
    rec = torch.zeros(12, dtype=torch.int32)
    u = rec.numpy().view(np.uint32)
    u[0], u[1], u[2] = step & 0xFFFFFFFF, seed & 0xFFFFFFFF, seed >> 32
    return rec.to(DEV)


# ================================================================================================ Diffuser
DIFFUSE_CASES = [(1, 1), (3, 5), (2, 1024), (3, 1028), (5, 969), (7, 3072), (3, 1398103)]
assert 3 * 1398103 == STRIDE2 + 5
EDGE = 8192


@functools.lru_cache(maxsize=2)
def _clean(B, CHW):
    return torch.from_numpy(np.random.default_rng(B * CHW).standard_normal((B, CHW)).astype(np.float32))


def _check_noisy(name, noisy, clean, sg64, unit, idx, CHW):
    """noisy = fma(sigma, noise, clean) to 2 u (|clean| + |sigma noise|): one rounding of the product more or less (the
    compiler may contract), one of the sum"""
    c, sn = _take(clean, idx), sg64[idx // CHW] * unit
    r = _ratio(np.abs(_take(noisy, idx) - (c + sn)), 2 * U * (np.abs(c) + np.abs(sn)))
    record("step_exact/" + name, r, 1.0)
    print(f"{name}: err / bound {r:.3f}")
    assert torch.isfinite(noisy).all()
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("B,CHW", DIFFUSE_CASES)
def test_diffuse_against_restatement(ops, B, CHW, seed, step):
    idx = _edges(B * CHW, EDGE)
    b_of = idx // CHW
    unit_ref = S.diffuse_unit_noise(idx, seed, step)
    zero, clean = torch.zeros(B, CHW, device=DEV), _clean(B, CHW).to(DEV)
    for P_mean, P_std in PS:
        tag = f"B{B} CHW{CHW} P_mean {P_mean}"
        nz, sg = ops.diffuse(zero, P_mean, P_std, seed, step)
        assert torch.isfinite(nz).all() and torch.isfinite(sg).all() and (sg > 0).all()
        sg64 = sg.double().cpu().numpy()
        # unit noise: the kernel's zero-clean output over its own sigma
        unit = _take(nz, idx) / sg64[b_of]
        err = float(np.abs(unit - unit_ref).max())
        record("step_exact/diffuse_unit_noise_maxabs", err, 1e-5)
        print(f"diffuse {tag} seed {seed:#x} step {step}: unit noise max abs {err:.3e}")
        assert err <= 1e-5, err                      # the Box-Muller limit; a wrong counter is O(1)
        # sigma: Box-Muller's limit on n0 through P_std, the argument's rounding and the hardware exp
        sig_ref, n0 = S.diffuse_sigma(B, P_mean, P_std, seed, step)
        bound = S.f32(P_std) * 1e-5 + (np.abs(S.f32(P_mean) + S.f32(P_std) * n0) + 4) * 2.0 ** -23
        r = _ratio(np.abs(sg64 - sig_ref) / sig_ref, bound)
        record("step_exact/diffuse_sigma", r, 1.0)
        print(f"diffuse {tag} seed {seed:#x} step {step}: sigma rel err / bound {r:.3f}")
        assert r <= 1.0, (r, sg64, sig_ref)
        # non-zero clean: the same sigma bit for bit, the same noise added
        nz2, sg2 = ops.diffuse(clean, P_mean, P_std, seed, step)
        assert torch.equal(sg2, sg)
        _check_noisy("diffuse_noisy", nz2, clean, sg64, unit, idx, CHW)


@pytest.mark.parametrize("CHW", [5, 969, 1028])
def test_diffuse_samples_are_independent(ops, CHW):
    """a sample's noise and sigma depend on its index, the seed and the step, not on the batch around it"""
    seed, step = SEEDS[0], 3
    clean = _clean(7, CHW).to(DEV)
    nz7, sg7 = ops.diffuse(clean, -1.2, 1.2, seed, step)
    nz3, sg3 = ops.diffuse(clean[:3].contiguous(), -1.2, 1.2, seed, step)
    nz1, sg1 = ops.diffuse(clean[:1].contiguous(), -1.2, 1.2, seed, step)
    assert torch.equal(nz3[0], nz1[0]) and torch.equal(sg3[:1], sg1)
    assert torch.equal(nz7[:3], nz3) and torch.equal(sg7[:3], sg3)
    assert len(set(sg7.tolist())) == 7
    for other_seed, other_step in ((seed, step + 1), (seed ^ 1, step), (seed ^ (1 << 32), step), (seed, 2 ** 32 - 1)):
        nzo, sgo = ops.diffuse(clean, -1.2, 1.2, other_seed, other_step)
        assert (sgo != sg7).all(), (other_seed, other_step)
        assert (nzo != nz7).float().mean().item() > 0.99


@pytest.mark.parametrize("step", [3, 2 ** 32 - 1])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("B,CHW", [(3, 5), (5, 969)])
def test_diffuse_dyn_record_overrides_seed_and_step(ops, B, CHW, seed, step):
    """a device edm_step_params record replaces the by-value step and seed; the Diffuser's stream is the record's seed with
    its LOW word XORed by 0xD1FF05E5, what tinyedm_amd.Diffuser passes by value otherwise"""
    clean = _clean(B, CHW).to(DEV)
    garbage_seed, garbage_step = 0x5EED5EED0DDBA11, 99
    nz_dyn, sg_dyn = ops.diffuse(clean, -1.2, 1.2, garbage_seed, garbage_step, dyn=_step_record(seed, step))
    nz_val, sg_val = ops.diffuse(clean, -1.2, 1.2, seed ^ 0xD1FF05E5, step)
    assert torch.equal(nz_dyn, nz_val) and torch.equal(sg_dyn, sg_val)
    nz_g, sg_g = ops.diffuse(clean, -1.2, 1.2, garbage_seed, garbage_step)
    assert (sg_g != sg_dyn).all() and not torch.equal(nz_g, nz_dyn)
    # and that by-value call is the restatement's stream of the XORed seed
    sig_ref, _ = S.diffuse_sigma(B, -1.2, 1.2, seed ^ 0xD1FF05E5, step)
    assert np.abs(sg_dyn.double().cpu().numpy() / sig_ref - 1).max() <= 1e-4


@pytest.mark.parametrize("B,CHW", DIFFUSE_CASES)
def test_diffuse_given_against_fp64(ops, B, CHW):
    """The form with both normal draws supplied.  sigma = exp(P_mean + P_std eps) to 4 u of fp64: the kernel evaluates it
    in double and rounds once.  (An fp32 evaluation cannot keep that: half an ulp of the argument is 2 u of sigma by itself
    at |argument| in [2, 4).  With expf on the fp32 argument this test measured 4.38 u at (B, CHW) = (3, 5), P = (0.4, 2.0),
    of which the argument's rounding was 1.5 u; the other cases 0.5 u .. 3.4 u.)"""
    g = np.random.default_rng(B + CHW)
    eps = torch.from_numpy(g.standard_normal(B).astype(np.float32))
    noise = torch.from_numpy(g.standard_normal((B, CHW)).astype(np.float32)).to(DEV)
    clean = _clean(B, CHW).to(DEV)
    idx = _edges(B * CHW, EDGE)
    for P_mean, P_std in PS:
        noisy, sg = ops.diffuse_given(clean, eps.to(DEV), noise, P_mean, P_std)
        sg64 = sg.double().cpu().numpy()
        sig_ref = np.exp(S.f32(P_mean) + S.f32(P_std) * eps.double().numpy())
        rel = float((np.abs(sg64 - sig_ref) / sig_ref).max())
        record("step_exact/diffuse_given_sigma_rel", rel, 4 * U)
        print(f"diffuse_given B{B} CHW{CHW} P_mean {P_mean}: sigma rel err {rel:.3e} = {rel / U:.2f} u (limit 4 u)")
        assert rel <= 4 * U, (rel, sg64, sig_ref)
        _check_noisy("diffuse_given_noisy", noisy, clean, sg64, _take(noise, idx), idx, CHW)


# ================================================================================================ dropout mask
MASK_NS = [8, 16, 2056, 65536, 8 * 4096 * 256 + 8]
MASK_PS = [0.0, 5e-6, 0.1, 0.13, 0.5, 0.999]
MASK_EDGE = 4096


@pytest.mark.parametrize("p", MASK_PS)
@pytest.mark.parametrize("n", MASK_NS)
def test_dropout_mask_is_the_restatement(ops, n, p):
    idx = _edges(n, MASK_EDGE)
    thr = S.dropout_threshold(p) if p > 0 else 0
    q = 1.0 - thr / 65536.0
    for seed, sub, step in itertools.product(SEEDS, [0, 5, 2 ** 32 - 1], [0, 6]):
        mask = ops.dropout_mask(n, p, seed, sub, step, DEV)
        assert mask.dtype == torch.uint8 and mask.shape == (n,) and int(mask.max()) <= 1
        keep_ref, _ = S.dropout_keep_ref(n, p, seed, sub, step, elems=idx)
        got = mask[torch.from_numpy(idx).to(DEV)].cpu()
        assert torch.equal(got, torch.from_numpy(keep_ref)), (seed, sub, step, int((got.numpy() != keep_ref).sum()))
        if thr == 0:
            assert bool(mask.all())
        elif n == 65536:
            rate = mask.float().mean().item()
            dev = abs(rate - q) / np.sqrt(q * (1 - q) / n)
            record("step_exact/dropout_keep_rate_sigmas", dev, 5.0)
            assert dev <= 5.0, (rate, q, dev)


def test_mod_silu_drop_drops_where_the_restatement_does(ops):
    """the end-to-end tie: the kernel that applies the mask against the restatement, not against ops.dropout_mask"""
    B, H, W, C, p = 2, 5, 7, 64, 0.13
    seed, sub, step = SEEDS[0], 5, 6
    g = torch.Generator().manual_seed(9)
    r = torch.randn(B, H, W, C, generator=g)
    r = torch.where(r.abs() < 0.1, torch.full_like(r, 0.5), r).to(torch.bfloat16).to(DEV)       # no zeros
    lin = (0.3 * torch.randn(B, C, generator=g)).clamp(-0.5, 0.5).to(DEV)                        # lin * gain + 1 >= 0.55
    a = ops.mod_silu_drop_fwd(r, lin, torch.tensor(0.9, device=DEV), p, seed, sub, step)
    keep_ref, scale = S.dropout_keep_ref(r.numel(), p, seed, sub, step)
    dropped = torch.from_numpy(keep_ref == 0).view(B, H, W, C)
    assert 0 < int(dropped.sum()) < r.numel()
    assert torch.equal(a.cpu() == 0, dropped)
    # and the kernel that owns the mask agrees
    assert torch.equal(ops.dropout_mask(r.numel(), p, seed, sub, step, DEV).cpu(), torch.from_numpy(keep_ref))
    # unmasked, the kept values are the masked ones without the rescale
    a0 = ops.mod_silu_drop_fwd(r, lin, torch.tensor(0.9, device=DEV), 0.0, seed, sub, step)
    kept = ~dropped
    err = (a.float().cpu()[kept] - scale * a0.float().cpu()[kept]).abs()
    assert (err <= 2.0 ** -7 * (scale * a0.float().cpu()[kept]).abs()).all()          # two bf16 roundings


# ================================================================================================ Adam + EMA
HP = dict(lr=2e-3, b1=0.9, b2=0.999, eps=1e-8, ema_beta=0.9)
PBETAS = [0.5, 0.9, 0.99, 0.37]
ADAM_NS = [1, 3, 4, 5, 1023, 1024, 1028, 65540, STRIDE2 + 5]
ADAM_STEPS = [1, 7, 100000]
COMBOS = list(itertools.product(ADAM_STEPS, [1.0, 0.5], [True, False], [False, True]))     # step, grad_scale, ema, zero_grad
BIG_COMBOS = [(1, 1.0, True, False), (7, 0.5, False, True), (100000, 0.5, True, True)]    # every value once at the large size
FORM_K = {"plain": 0, "dyn": 0, "phema1": 1, "phema4": 4, "guarded": 0, "phema_guarded": 2, "skip": 2}


FULL = 1 << 17                           # arenas up to this size are compared whole, larger ones at both ends and the middle


@functools.lru_cache(maxsize=1)
def _state(n):
    return S.adam_state(n, n % 997, 4)


def _upload(st, K=2):
    D = {k: torch.from_numpy(st[k]).to(DEV) for k in ("theta", "grad", "m", "v", "ema")}
    D["profiles"] = [torch.from_numpy(p).to(DEV) for p in st["profiles"][:K]]
    return D


def _adam_record(lr, ema_beta, grad_scale, bc1, bc2sqrt):
    """a device edm_step_params record holding only the optimizer's five scalars"""
    rec = np.zeros(12, dtype=np.float32)
    rec[4:9] = [lr, ema_beta, grad_scale, bc1, bc2sqrt]
    return torch.from_numpy(rec.view(np.int32)).to(DEV)


def _guard_record(ops, coef=1.0, skip=0):
    rec = np.zeros(1, dtype=ops.GUARD_RECORD)
    rec["coef"], rec["skip"], rec["clip_value"] = coef, skip, np.inf
    return torch.from_numpy(rec.view(np.int64).copy()).to(DEV)


def _bits_equal(t, a):
    """device fp32 tensor t holds exactly the bits of the numpy float32 array a"""
    return torch.equal(t.view(torch.int32).cpu(), torch.from_numpy(a.view(np.int32)))


def _check_adam(form, D, st, sel, hp, with_ema, betas, where=""):
    """the arenas D after one update of the elements `sel` of state `st`, against adam_ema_ref in the issue's bounds"""
    K = len(betas)
    cut = {k: st[k][sel] for k in ("theta", "grad", "m", "v", "ema")}
    ref = S.adam_ema_ref(cut["theta"], cut["grad"], cut["m"], cut["v"], cut["ema"] if with_ema else None,
                         [p[sel] for p in st["profiles"][:K]], betas, **hp)
    bound = S.adam_ema_bounds(ref, cut["theta"], hp["ema_beta"], betas)
    items = [("m", D["m"], ref["m"], bound["m"]), ("v", D["v"], ref["v"], bound["v"]),
             ("theta", D["theta"], ref["theta"], bound["theta"])]
    if with_ema:
        items.append(("ema", D["ema"], ref["ema"], bound["ema"]))
    items += [("profile", D["profiles"][k], ref["profiles"][k], bound["profiles"][k]) for k in range(K)]
    idx = np.arange(st["theta"].size)[sel]
    for key, t, r64, b in items:
        got = _take(t, idx)
        assert np.isfinite(got).all(), (form, key)
        ratio = _ratio(np.abs(got - r64), b)
        record(f"step_exact/adam_{form}_{key}", ratio, 1.0)
        assert ratio <= 1.0, f"{form} {where}: {key} err / bound = {ratio:.3f}"
    return ref


def _run_form(ops, form, n, step, gs, with_ema, zero_grad):
    K = FORM_K[form]
    st = _state(n)
    D = _upload(st, K)
    ema = D["ema"] if with_ema else None
    bc1, bc2s = S.bias_corrections(HP["b1"], HP["b2"], step)
    hp = dict({k: S.f32(x) for k, x in HP.items()}, bc1=bc1, bc2sqrt=bc2s, grad_scale=gs)
    args = (HP["lr"], HP["b1"], HP["b2"], HP["eps"], step, HP["ema_beta"], gs)
    betas = PBETAS[:K]
    betas_d = torch.tensor(betas, dtype=torch.float32, device=DEV) if K else None
    state = (D["theta"], D["grad"], D["m"], D["v"], ema)
    unchanged = False
    if form == "plain":
        ops.adam_ema(*state, *args, zero_grad=zero_grad)
    elif form == "dyn":                     # garbage by value for everything the record holds
        rec = _adam_record(HP["lr"], HP["ema_beta"], gs, bc1, bc2s)
        ops.adam_ema(*state, 123.0, HP["b1"], HP["b2"], HP["eps"], 3 if step != 3 else 4, 0.125, 77.0, dyn=rec,
                     zero_grad=zero_grad)
    elif form in ("phema1", "phema4"):
        ops.adam_ema_phema(*state, D["profiles"], betas_d, *args, zero_grad=zero_grad)
    elif form in ("guarded", "phema_guarded"):
        # a max_norm of half the scaled gradient's norm clips: the update runs on grad_scale * coef
        norm = gs * float(np.linalg.norm(st["grad"].astype(np.float64)))
        table = ops.grad_guard_table([0], [n], n, DEV)
        rec = ops.guard_record(DEV)
        ops.grad_guard(D["grad"], table, torch.zeros(1, dtype=torch.float64, device=DEV), rec, grad_scale=gs,
                       max_norm=0.5 * norm)
        got = ops.read_guard_record(rec)
        assert got["skip"] == 0 and abs(got["norm"] / norm - 1) <= 1e-5, (got, norm)
        assert 0.4 < got["coef"] <= 0.5 and abs(got["coef"] * (norm + 1e-6) / (0.5 * norm) - 1) <= 1e-5, (got, norm)
        hp["grad_scale"] = gs * got["coef"]
        if form == "guarded":
            ops.adam_ema_guarded(*state, rec, *args, zero_grad=zero_grad)
        else:
            ops.adam_ema_phema_guarded(*state, D["profiles"], betas_d, rec, *args, zero_grad=zero_grad)
    else:                                   # a record that says skip: nothing but the clearing of the gradient
        ops.adam_ema_phema_guarded(*state, D["profiles"], betas_d, _guard_record(ops, skip=1), *args, zero_grad=zero_grad)
        unchanged = True
    ops.check_health(DEV, f"{form} n={n}")                # 0 after every clean case
    where = f"n={n} step={step} grad_scale={gs} ema={with_ema} zero_grad={zero_grad}"
    # the gradient arena: cleared to the last tail element, or not touched
    if zero_grad:
        assert not D["grad"].view(torch.int32).any(), where
    else:
        assert _bits_equal(D["grad"], st["grad"]), where
    if not with_ema:
        assert _bits_equal(D["ema"], st["ema"]), where
    if unchanged:
        for key in ("theta", "m", "v", "ema"):
            assert _bits_equal(D[key], st[key]), (key, where)
        for k in range(K):
            assert _bits_equal(D["profiles"][k], st["profiles"][k]), (k, where)
        return
    sel = slice(None) if n <= FULL else np.r_[0:EDGE, n // 2 - 8:n // 2 + 8, n - EDGE:n]
    _check_adam(form, D, st, sel, hp, with_ema, betas, where)
    if n > FULL:
        for key in ("theta", "m", "v"):
            assert torch.isfinite(D[key]).all() and not _bits_equal(D[key], st[key])
    if n >= 3:                              # g = m = v = 0: an update of exactly 0
        z = n // 2
        assert D["theta"][z].item() == st["theta"][z] and D["m"][z].item() == 0 and D["v"][z].item() == 0, where


@pytest.mark.parametrize("form", list(FORM_K))
@pytest.mark.parametrize("n", ADAM_NS)
def test_adam_ema_forms_against_fp64(ops, n, form):
    for step, gs, with_ema, zero_grad in (COMBOS if n <= FULL else BIG_COMBOS):
        _run_form(ops, form, n, step, gs, with_ema, zero_grad)


# ---- the ranges form: kept ranges of every short length and of one, two and two-and-a-bit chunks, starting at offsets
# 1, 2, 3 (mod 4) in turn, with at least one excluded element between neighbours
RANGE_LENGTHS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 2049]


def _kept_ranges():
    kept, pos = [], 0
    for k, length in enumerate(RANGE_LENGTHS):
        start = pos + 1
        while start % 4 != 1 + k % 3:
            start += 1
        kept.append((start, length))
        pos = start + length
    return kept, pos + 7


def test_adam_ema_ranges_against_fp64(ops):
    kept, n = _kept_ranges()
    assert [s % 4 for s, _ in kept] == [1, 2, 3] * 3
    inside = np.zeros(n, dtype=bool)
    for s, length in kept:
        assert not inside[s - 1] and not inside[s:s + length].any()
        inside[s:s + length] = True
    edges = np.flatnonzero(np.diff(np.concatenate([[True], inside, [True]]).astype(np.int8)))
    excluded = [(int(a), int(b - a)) for a, b in zip(edges[0::2], edges[1::2])]      # the runs of ~inside
    assert ops.complement_ranges(excluded, n) == kept
    ranges, chunks = ops.adam_ranges_table(excluded, n, DEV)
    st = S.adam_state(n, 77, 0)
    st["grad"][kept[5][0] + 1000] = st["m"][kept[5][0] + 1000] = st["v"][kept[5][0] + 1000] = 0     # forced, inside a range
    z = kept[5][0] + 1000
    for step, gs, with_ema, zero_grad in COMBOS:
        D = _upload(st, 0)
        bc1, bc2s = S.bias_corrections(HP["b1"], HP["b2"], step)
        hp = dict({k: S.f32(x) for k, x in HP.items()}, bc1=bc1, bc2sqrt=bc2s, grad_scale=gs)
        ops.adam_ema_ranges(D["theta"], D["grad"], D["m"], D["v"], D["ema"] if with_ema else None, ranges, chunks, HP["lr"],
                            HP["b1"], HP["b2"], HP["eps"], step, HP["ema_beta"], gs, zero_grad=zero_grad)
        ops.check_health(DEV, "ranges")
        where = f"ranges step={step} grad_scale={gs} ema={with_ema} zero_grad={zero_grad}"
        _check_adam("ranges", D, st, inside, hp, with_ema, [], where)
        out = torch.from_numpy(~inside)
        for key in ("theta", "grad", "m", "v", "ema"):                    # outside: the bits that were put there
            got, put = D[key].view(torch.int32).cpu(), torch.from_numpy(st[key].view(np.int32))
            assert torch.equal(got[out], put[out]), (key, where)
        g_in = D["grad"].view(torch.int32).cpu()[torch.from_numpy(inside)]
        if zero_grad:
            assert not g_in.any(), where
        else:
            assert torch.equal(g_in, torch.from_numpy(st["grad"].view(np.int32)[inside])), where
        if not with_ema:
            assert _bits_equal(D["ema"], st["ema"]), where
        assert D["theta"][z].item() == st["theta"][z] and D["m"][z].item() == 0 and D["v"][z].item() == 0, where


# ---- the health word
def _launch_for_health(ops, form, D, n):
    args = (HP["lr"], HP["b1"], HP["b2"], HP["eps"], 7, HP["ema_beta"], 1.0)
    state = (D["theta"], D["grad"], D["m"], D["v"], D["ema"])
    betas_d = torch.tensor(PBETAS[:2], dtype=torch.float32, device=DEV)
    if form == "plain":
        ops.adam_ema(*state, *args)
    elif form == "phema":
        ops.adam_ema_phema(*state, D["profiles"], betas_d, *args)
    elif form == "guarded":
        ops.adam_ema_guarded(*state, _guard_record(ops), *args)
    elif form == "phema_guarded":
        ops.adam_ema_phema_guarded(*state, D["profiles"], betas_d, _guard_record(ops), *args)
    else:
        ops.adam_ema_ranges(*state, *ops.adam_ranges_table([], n, DEV), *args)


@pytest.mark.parametrize("form", ["plain", "phema", "guarded", "phema_guarded", "ranges"])
@pytest.mark.parametrize("n,bad", [(1023, 1022), (1023, 513)])
def test_health_word_reports_a_nan_gradient(ops, n, bad, form):
    """one NaN gradient, in the last partial quad (element 1022 of 1023) or in a full one, sets bit 0 (1u) and nothing else;
    the same launch on clean gradients leaves the word at 0"""
    st = S.adam_state(n, 5, 2)
    ops.check_health(DEV, "before")
    _launch_for_health(ops, form, _upload(st), n)
    assert int(ops.health(DEV).item()) == 0
    st = dict(st, grad=st["grad"].copy())
    st["grad"][bad] = np.nan
    D = _upload(st)
    _launch_for_health(ops, form, D, n)
    assert int(ops.health(DEV).item()) == 1
    with pytest.raises(ops.GraphCorruptionError, match="non-finite gradient"):
        ops.check_health(DEV, "poisoned gradient")
    assert int(ops.health(DEV).item()) == 0
    # the NaN stays in its element
    ok = np.arange(n) != bad
    for key in ("theta", "m", "v", "ema"):
        got = D[key].cpu().numpy()
        assert np.isfinite(got[ok]).all() and np.isnan(got[bad]), key
