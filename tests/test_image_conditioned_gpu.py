"""Image-conditioned sampling on the GPU: SDEdit (solve(..., start_step=k, image=...)), inpainting by replacement
(mask=...) and ODE inversion (invert):

 * the kernels: ops.inpaint_blend's noise against a numpy restatement of Philox4x32-10 + Box-Muller under the blend's
   tag, on the dwordx4 path, the scalar path (HW % 4 != 0) and a misaligned tensor; its exact properties (mask == 0 is
   x, t == 0 is image, mask broadcast, batch independence); independence from the churn stream; the health bit;
   ops.state_init against ops.scale_f32 (bit for bit) and fp64 (1 ulp);
 * SDEdit and inpainting trajectories of tiny nets against the CPU oracle composing the same updates with the exact GPU
   noise (drawn by ops.inpaint_blend on zeros under an all-ones mask), Heun bf16 / "f32", stochastic Heun with a churn
   window, multistep orders 2 and 3, start_step 0 and 5, one inpainting case with CFG guidance; invert against Heun run
   up the table on the CPU.  Limits: the project's trajectory limits (bf16 1e-2, tests/test_network_gpu.py; f32 2e-4,
   tests/test_evalf32_gpu.py; 3x guided, tests/test_guided_solver_gpu.py);
 * bit-exact identities, eager and hipGraph, and the graph cache key;
 * the analytic Gaussian denoiser: inversion is second order, the round trip closes; the mixture: inpainting holds;
 * the generate CLI end to end."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs
from parity_log import record

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLEND_TAG, CHURN_TAG = 0x49500000, 0x43480000


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------ the noise stream, restated
M32 = np.uint64(0xFFFFFFFF)


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = c[0] * np.uint64(0xD2511F53)
        p1 = c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def _box_muller(a, b):
    u1 = ((a >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    u2 = ((b >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)


def _noise_ref(shape, seed, solve_index, step, tag=BLEND_TAG):
    """element j of sample b: normal j % 4 of philox((j / 4, b, tag ^ step, solve_index), (seed_lo, seed_hi))"""
    B, CHW = shape[0], int(np.prod(shape[1:]))
    j = np.arange(CHW, dtype=np.uint64)
    b = np.arange(B, dtype=np.uint64)[:, None]
    r = _philox4x32_10(j[None, :] // np.uint64(4) + 0 * b, b + 0 * j[None, :], tag ^ step, solve_index,
                       seed & 0xFFFFFFFF, seed >> 32)
    n0, n1 = _box_muller(r[0], r[1])
    n2, n3 = _box_muller(r[2], r[3])
    n = np.stack([n0, n1, n2, n3])                   # [4, B, CHW]
    k = (j % np.uint64(4)).astype(np.int64)
    return np.take_along_axis(n.transpose(1, 2, 0), k[None, :, None], axis=2)[..., 0].reshape(shape)


def _zeros(shape, offset=0):
    n = int(np.prod(shape))
    return torch.zeros(n + offset, device=DEV)[offset:].view(shape)


def _ones_mask(shape, rows=1):
    return torch.ones(rows, int(np.prod(shape[2:])), dtype=torch.uint8, device=DEV)


def _blend_noise(ops, shape, seed, solve_index, step, offset=0):
    """the N(0, 1) field the blend draws: image = 0, every pixel known, t = 1"""
    rec = ops.churn_record(seed, solve_index, DEV)
    return ops.inpaint_blend(_zeros(shape, offset), _zeros(shape, offset), _ones_mask(shape), 1.0, rec, step)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("shape,offset", [((7, 3, 32, 32), 0), ((5, 3, 7, 9), 0), ((7, 3, 32, 32), 1)],
                         ids=["cifar-vec", "odd-scalar", "misaligned-scalar"])
def test_blend_noise_vs_restatement(ops, shape, offset):
    seed, solve_index, step = 0x9E3779B97F4A7C15, 3, 5
    n = _blend_noise(ops, shape, seed, solve_index, step, offset)
    assert (_zeros(shape, offset).data_ptr() % 16 == 0) == (offset == 0)
    ops.check_health(DEV, "inpaint_blend")
    ref = _noise_ref(shape, seed, solve_index, step)
    err = float(np.abs(n.double().cpu().numpy() - ref).max())
    print(f"blend noise {shape} offset {offset}: max abs {err:.3e}")
    record(f"image_conditioned/blend_noise_{'x'.join(map(str, shape))}_off{offset}_maxabs", err, 1e-5)
    assert err <= 1e-5, err      # the churn's Box-Muller (__logf, __sincosf: 2.1e-6 there); a wrong counter is O(1)
    churn = _noise_ref(shape, seed, solve_index, step, CHURN_TAG)
    assert np.abs(ref - churn).max() > 1.0           # the restated streams differ: the tag matters
    if offset:          # the scalar path of a misaligned tensor draws what the dwordx4 path draws, bit for bit
        assert torch.equal(n, _blend_noise(ops, shape, seed, solve_index, step))


def _operands(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g).to(DEV)
    image = torch.randn(shape, generator=g).to(DEV)
    mask = (torch.rand(shape[0], int(np.prod(shape[2:])), generator=g) < 0.4).to(torch.uint8).to(DEV)
    return x, image, mask


@pytest.mark.parametrize("shape", [(6, 3, 16, 16), (5, 3, 7, 9), (3, 2, 6, 6)], ids=["vec", "odd", "hw36-chw72"])
def test_blend_exact_properties(ops, shape):
    x, image, mask = _operands(shape, 1)
    rec = ops.churn_record(42, 7, DEV)
    B, C = shape[:2]
    sel = mask.view(B, 1, *shape[2:]).expand(shape).bool()
    assert 0 < int(sel.sum()) < sel.numel()
    t, step = 2.75, 4
    out = ops.inpaint_blend(x, image, mask, t, rec, step)
    assert torch.equal(out[~sel], x[~sel])                                   # mask == 0: x, bit for bit
    n = _blend_noise(ops, shape, 42, 7, step)
    ref = image.double() + t * n.double()                                    # mask != 0: image + t*n, one fma
    assert ((out.double() - ref)[sel].abs() <= 1.2e-7 * ref[sel].abs() + 1e-37).all()
    # the noise does not depend on the mask: the masked blend is the all-ones blend where the mask is set
    full = ops.inpaint_blend(x, image, torch.ones_like(mask), t, rec, step)
    assert torch.equal(out[sel], full[sel])
    # t == 0: image itself on the mask
    out0 = ops.inpaint_blend(x, image, mask, 0.0, rec, step)
    assert torch.equal(out0, torch.where(sel, image, x))
    neg = -torch.zeros_like(image)                                           # ... its sign bit included
    assert torch.equal(torch.signbit(ops.inpaint_blend(x, neg, torch.ones_like(mask), 0.0, rec, 0)),
                       torch.ones_like(sel))
    # mask_B == 1 is the same mask repeated B times
    one = mask[:1].contiguous()
    assert torch.equal(ops.inpaint_blend(x, image, one, t, rec, step),
                       ops.inpaint_blend(x, image, one.expand(B, -1).contiguous(), t, rec, step))
    # a sample's noise is independent of B
    assert torch.equal(ops.inpaint_blend(x[:2].contiguous(), image[:2].contiguous(), mask[:2].contiguous(), t, rec, step),
                       out[:2])
    ops.check_health(DEV, "inpaint_blend properties")


def test_state_init(ops):
    g = torch.Generator().manual_seed(2)
    for n, offset in ((3 * 32 * 32 * 5, 0), (4099, 0), (4099, 1)):
        x0 = torch.randn(n + offset, generator=g).to(DEV)[offset:]
        image = torch.randn(n + offset, generator=g).to(DEV)[offset:]
        x0[::7] *= -0.0
        for t in (80.0, 0.002, 1.7320508, 0.0):
            assert torch.equal(ops.state_init(x0, t), ops.scale_f32(x0, t))
            assert torch.equal(torch.signbit(ops.state_init(x0, t)), torch.signbit(ops.scale_f32(x0, t)))
            out = ops.state_init(x0, t, image)
            t32 = float(np.float32(t))
            ref = (image.double() + t32 * x0.double())
            ulp = torch.maximum(ref.abs(), torch.tensor(1.2e-38, dtype=torch.float64, device=DEV))
            ulp = 2.0 ** (torch.floor(torch.log2(ulp)) - 23)
            assert ((out.double() - ref).abs() <= ulp).all()                 # a single fma: within 1 ulp (in fact 1/2)
    ops.check_health(DEV, "state_init")


def test_blend_stream_independent_of_churn(ops):
    shape = (8, 3, 64, 64)
    m = int(np.prod(shape))
    for seed, index, step in ((5, 0, 0), (5, 3, 7), (1 << 40, 0, 2)):
        rec = ops.churn_record(seed, index, DEV)
        a = _blend_noise(ops, shape, seed, index, step).double().flatten()
        b = ops.heun_churn(_zeros(shape), 1.0, rec, step).double().flatten()
        corr = torch.corrcoef(torch.stack([a, b]))[0, 1].item()
        print(f"blend / churn correlation at {(seed, index, step)}: {corr:.2e} (limit {5 / math.sqrt(m):.2e})")
        assert abs(corr) <= 5 / math.sqrt(m), corr
        assert abs(a.mean().item()) < 5 / math.sqrt(m) and abs(a.std().item() - 1.0) < 5 / math.sqrt(2 * m)


def test_blend_and_state_init_nonfinite_set_health(ops):
    rec = ops.churn_record(1, 0, DEV)
    ops.check_health(DEV, "before")
    for shape, idx in (((7, 3, 32, 32), (3, 1, 5, 17)), ((5, 3, 7, 9), (4, 2, 6, 8))):      # dwordx4 body; last partial quad
        for which in ("x", "image"):
            x, image = torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV)
            (x if which == "x" else image)[idx] = float("nan")
            mask = _ones_mask(shape) * (which == "image")
            ops.inpaint_blend(x, image, mask.contiguous(), 1.0, rec, 0)
            with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
                ops.check_health(DEV, f"inpaint_blend {which}")
    x0 = torch.zeros(4099, device=DEV)
    x0[4097] = float("inf")
    ops.state_init(x0, 2.0, torch.zeros_like(x0))
    with pytest.raises(ops.GraphCorruptionError, match="non-finite sampler state"):
        ops.check_health(DEV, "state_init")
    ops.check_health(DEV, "after")


def test_new_ops_reject_bad_operands(ops):
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    mask = torch.ones(1, 64, dtype=torch.uint8, device=DEV)
    rec = ops.churn_record(0, 0, DEV)
    bad = [
        (TypeError, lambda: ops.inpaint_blend(x.double(), x, mask, 1.0, rec, 0)),
        (TypeError, lambda: ops.inpaint_blend(x, x, mask.bool(), 1.0, rec, 0)),
        (ValueError, lambda: ops.inpaint_blend(x, x[:1], mask, 1.0, rec, 0)),
        (ValueError, lambda: ops.inpaint_blend(x.transpose(2, 3), x, mask, 1.0, rec, 0)),
        (ValueError, lambda: ops.inpaint_blend(x, x, torch.ones(3, 64, dtype=torch.uint8, device=DEV), 1.0, rec, 0)),
        (ValueError, lambda: ops.inpaint_blend(x, x, torch.ones(1, 63, dtype=torch.uint8, device=DEV), 1.0, rec, 0)),
        (ValueError, lambda: ops.inpaint_blend(x, x, torch.ones(64, dtype=torch.uint8, device=DEV), 1.0, rec, 0)),
        (RuntimeError, lambda: ops.inpaint_blend(x, x, mask.cpu(), 1.0, rec, 0)),
        (ValueError, lambda: ops.inpaint_blend(x, x, mask, -1.0, rec, 0)),
        (ValueError, lambda: ops.inpaint_blend(x, x, mask, math.inf, rec, 0)),
        (ValueError, lambda: ops.inpaint_blend(x, x, mask, math.nan, rec, 0)),
        (ValueError, lambda: ops.inpaint_blend(x, x, mask, 1.0, rec, -1)),
        (ValueError, lambda: ops.inpaint_blend(x, x, mask, 1.0, rec, 1 << 16)),
        (ValueError, lambda: ops.inpaint_blend(x, x, mask, 1.0, torch.zeros(3, dtype=torch.int32, device=DEV), 0)),
        (ValueError, lambda: ops.inpaint_blend(torch.zeros(4, 8, device=DEV), torch.zeros(4, 8, device=DEV), mask, 1.0, rec, 0)),
        (TypeError, lambda: ops.state_init(x.half(), 1.0)),
        (ValueError, lambda: ops.state_init(x, 1.0, x[:1])),
        (ValueError, lambda: ops.state_init(x, -0.5)),
        (ValueError, lambda: ops.state_init(x, math.nan, x)),
        (RuntimeError, lambda: ops.state_init(x, 1.0, x.cpu())),
        (ValueError, lambda: ops.state_init(x.transpose(2, 3), 1.0)),
    ]
    from tinyedm_amd import _lib
    calls = _lib.N_CALLS
    for exc, fn in bad:
        with pytest.raises(exc):
            fn()
    assert _lib.N_CALLS == calls                    # nothing was launched


# ------------------------------------------------------------------ trajectories vs the CPU oracle
def _edm(P, ecfg, dcfg, dtype):
    """an eval-mode EDM on the GPU with the oracle's parameters (the _cifar pattern of tests/test_evalf32_gpu.py)"""
    import tinyedm_amd as T
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), dcfg.dropout_rate,
                     dcfg.sigma_data, dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    emb.load_state_dict({k[len("embedding."):]: v for k, v in P.items() if k.startswith("embedding.")}, strict=True)
    den.load_state_dict({k[len("denoiser."):]: v for k, v in P.items() if k.startswith("denoiser.")}, strict=True)
    den.set_eval_dtype(dtype)
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                  steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01)
    return model.to(DEV).eval()


def _oracle_D(Pm, em, dm, bf16, guide=None):
    def D(x, s, labels):
        sig = s.reshape(-1).expand(x.shape[0])
        Dm = O.edm_forward(Pm, em, dm, x, sig, labels, bf16=bf16).float()
        if guide is None:
            return Dm
        Pg, eg, dg, w, (lo, hi) = guide
        if not lo < float(s) <= hi:
            return Dm
        gl = labels if eg.num_classes is not None else None
        Dg = O.edm_forward(Pg, eg, dg, x, sig, gl, bf16=bf16).float()
        return Dg + w * (Dm - Dg)
    return D


def _oracle_conditioned(ops, sol, D, x0, labels, k, image, mask, solve_index):
    """the conditioned solve on the CPU: the solver's update formulas, the state entered at t_k, the known pixels
    replaced before every evaluation (and by the image at the end), with the noise the GPU kernels draw"""
    import tinyedm_amd as T
    t, N = sol.t_steps, sol.num_steps
    sel = None if mask is None else mask.bool().expand(x0.shape)
    img = torch.zeros_like(x0) if image is None else image.float()

    def blend(x, i):
        if sel is None:
            return x
        n = _blend_noise(ops, tuple(x0.shape), sol.seed, solve_index, i).cpu()
        return torch.where(sel, img + t[i] * n, x)
    x1 = img + t[k] * x0.float()
    if isinstance(sol, T.MultistepSolver):
        hist = []
        for i, (a, c0, c1, c2) in enumerate(sol.multistep_coefficients(start_step=k).tolist()):
            if i < k:
                continue
            x = blend(x1, i)
            m = D(x, t[i], labels)
            x1 = a * x + c0 * m
            if c1 != 0.0:
                x1 = x1 + c1 * hist[-1]
            if c2 != 0.0:
                x1 = x1 + c2 * hist[-2]
            hist.append(m)
    else:
        s = sol.churn_schedule() if isinstance(sol, T.StochasticSolver) else None
        rec = ops.churn_record(sol.seed, solve_index, DEV)
        for i in range(k, N):
            x = blend(x1, i)
            t0, t1 = t[i], t[i + 1]
            if s is not None and s.gamma[i] > 0:       # the churn lifts the blended state
                x = x + s.c[i] * ops.heun_churn(torch.zeros(x0.shape, device=DEV), 1.0, rec, i).cpu()
                t0 = s.t_hat[i]
            dx = (x - D(x, t0, labels)) / t0
            x1 = x + (t1 - t0) * dx
            if i < N - 1:
                dxp = (x1 - D(x1, t1, labels)) / t1
                x1 = x + (t1 - t0) * (0.5 * dx + 0.5 * dxp)
    return x1 if sel is None else torch.where(sel, img, x1)


SCHED = dict(num_steps=8, sigma_min=0.01, sigma_max=20.0, rho=5.0)
CASES = ["heun_bf16", "heun_f32", "stochastic_bf16", "multistep2_bf16", "multistep3_f32", "multistep3_bf16",
         "multistep2_f32"]


def _case_solver(case, **kw):
    import tinyedm_amd as T
    if case.startswith("stochastic"):
        return T.StochasticSolver(**SCHED, S_churn=30.0, S_min=0.3, S_max=8.0, seed=1234, **kw)
    if case.startswith("multistep"):
        return T.MultistepSolver(**SCHED, order=int(case[9]), seed=1234, **kw)
    return T.DeterministicSolver(**SCHED, seed=1234, **kw)


def _inputs():
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(2, 3, 8, 8, generator=g)
    labels = torch.randint(0, 10, (2,), generator=g)
    image = 0.5 * torch.randn(2, 3, 8, 8, generator=g)
    mask = torch.zeros(2, 1, 8, 8, dtype=torch.bool)
    mask[0, 0, :, :4] = True                        # per-sample masks: the left half; a frame
    mask[1, 0, :2] = mask[1, 0, -2:] = True
    mask[1, 0, :, :1] = True
    return x0, labels, image, mask


@pytest.mark.parametrize("start", [0, 5])
@pytest.mark.parametrize("mode", ["sdedit", "inpaint"])
@pytest.mark.parametrize("case", CASES)
def test_conditioned_trajectory_vs_oracle(ops, case, mode, start):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    em, dm = tiny_cfgs(10)
    Pm = O.init_params(em, dm, torch.Generator().manual_seed(7))
    bf16 = case.endswith("bf16")
    main = _edm(Pm, em, dm, "bf16" if bf16 else "f32")
    sol = _case_solver(case)
    if case.startswith("stochastic"):
        churned = (sol.churn_schedule().gamma > 0).nonzero().flatten().tolist()
        assert 0 < len(churned) < 8 and any(i >= 5 for i in churned)       # a window, and it reaches the partial solve
    x0, labels, image, mask = _inputs()
    mask = mask if mode == "inpaint" else None
    sol.solve_index = 5
    x_hip = sol.solve(main, x0.to(DEV), labels.to(DEV), start_step=start, image=image.to(DEV),
                      mask=None if mask is None else mask.to(DEV)).cpu()
    assert sol.solve_index == 5 + (mode == "inpaint" or case.startswith("stochastic"))
    with torch.no_grad():
        x_or = _oracle_conditioned(ops, sol, _oracle_D(Pm, em, dm, bf16), x0, labels, start, image, mask, 5)
    e = rel(x_hip, x_or)
    lim = 1e-2 if bf16 else 2e-4
    print(f"{case} {mode} start {start}: rel {e:.3e} (limit {lim:.0e})")
    record(f"image_conditioned/{case}_{mode}_start{start}_vs_{'bf16' if bf16 else 'fp32'}_oracle", e, lim)
    assert e <= lim, e
    if mask is not None:
        sel = mask.expand(x0.shape)
        assert torch.equal(x_hip[sel], image[sel])
    # the conditioning must matter at this size: the plain solve from x0 is far from the conditioned oracle.  Not so for
    # SDEdit entered at t_0 = 20: the image (std 0.5) moves that state by 2.5 %, the order of the bf16 error itself
    plain = _case_solver(case)
    plain.solve_index = 5
    x_plain = plain.solve(main, x0.to(DEV), labels.to(DEV)).cpu()
    assert not torch.equal(x_plain, x_hip)
    if mask is not None or start > 0:
        assert rel(x_plain, x_or) > 5 * e


def test_guided_inpainting_vs_oracle(ops):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    em, dm = tiny_cfgs(10)
    eg, dg = tiny_cfgs(None)
    Pm = O.init_params(em, dm, torch.Generator().manual_seed(7))
    Pg = O.init_params(eg, dg, torch.Generator().manual_seed(11))
    interval = (0.2, 7.0)
    sol = _case_solver("heun_bf16", guide=_edm(Pg, eg, dg, "bf16"), guidance=2.0, guidance_interval=interval)
    flags = sol.guided_evaluations()
    assert any(flags[10:]) and not all(flags[10:])          # of the evaluations a start_step = 5 solve runs
    main = _edm(Pm, em, dm, "bf16")
    x0, labels, image, mask = _inputs()
    for start in (0, 5):
        sol.solve_index = 2
        x_hip = sol.solve(main, x0.to(DEV), labels.to(DEV), start_step=start, image=image.to(DEV),
                          mask=mask.to(DEV)).cpu()
        with torch.no_grad():
            x_or = _oracle_conditioned(ops, sol, _oracle_D(Pm, em, dm, True, (Pg, eg, dg, 2.0, interval)), x0, labels,
                                       start, image, mask, 2)
        e = rel(x_hip, x_or)
        print(f"guided inpainting start {start}: rel {e:.3e} (limit 3e-2)")
        record(f"image_conditioned/cfg_heun_bf16_inpaint_start{start}_vs_bf16_oracle", e, 3e-2)
        assert e <= 3e-2, e


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("end", [0, 5])
def test_invert_vs_oracle(ops, dtype, end):
    import tinyedm_amd as T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    em, dm = tiny_cfgs(10)
    Pm = O.init_params(em, dm, torch.Generator().manual_seed(7))
    main = _edm(Pm, em, dm, dtype)
    sol = T.DeterministicSolver(**SCHED)
    _, labels, image, _ = _inputs()
    lat = sol.invert(main, image.to(DEV), labels.to(DEV), end_step=end).cpu()
    D = _oracle_D(Pm, em, dm, dtype == "bf16")
    t, N = sol.t_steps, sol.num_steps
    with torch.no_grad():
        x = image.float()
        for i in range(N - 1, end, -1):                 # Heun up the table: t_i -> t_{i-1}
            t0, t1 = t[i], t[i - 1]
            dx = (x - D(x, t0, labels)) / t0
            x1 = x + (t1 - t0) * dx
            dxp = (x1 - D(x1, t1, labels)) / t1
            x = x + (t1 - t0) * (0.5 * dx + 0.5 * dxp)
        ref = x / t[end]
    e = rel(lat, ref)
    lim = 1e-2 if dtype == "bf16" else 2e-4
    print(f"invert {dtype} end {end}: rel {e:.3e} (limit {lim:.0e})")
    record(f"image_conditioned/invert_{dtype}_end{end}_vs_oracle", e, lim)
    assert e <= lim, e
    assert rel(lat, image / t[end]) > 5 * e             # the steps moved the state


# ------------------------------------------------------------------ identities and the hipGraph path
@pytest.fixture(scope="module")
def pair(ops):
    em, dm = tiny_cfgs(10)
    main = _edm(O.init_params(em, dm, torch.Generator().manual_seed(7)), em, dm, "bf16")
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(3, 3, 8, 8, generator=g).to(DEV)
    labels = torch.randint(0, 10, (3,), generator=g).to(DEV)
    image = (0.5 * torch.randn(3, 3, 8, 8, generator=g)).to(DEV)
    mask = (torch.rand(3, 1, 8, 8, generator=g) < 0.5).to(DEV)
    return main, x0, labels, image, mask


@pytest.mark.parametrize("case", ["heun_bf16", "stochastic_bf16", "multistep3_bf16"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_defaults_are_the_plain_solve(pair, case, graph):
    main, x0, labels, _, _ = pair
    a, b = _case_solver(case), _case_solver(case)
    plain = a.solve(main, x0, labels, graph)
    assert torch.equal(b.solve(main, x0, labels, graph, start_step=0, image=None, mask=None), plain)
    assert a.solve_index == b.solve_index == int(case.startswith("stochastic"))
    if graph:
        assert list(a._graphs[main]) == list(b._graphs[main]) and len(b._graphs[main]) == 1
        a.solve_index = 0
        # the explicit defaults replay the entry the plain call captured
        assert torch.equal(a.solve(main, x0, labels, True, start_step=0, image=None, mask=None), plain)
        assert len(a._graphs[main]) == 1
    # start_step = 0 with a zero image is the same state: x0 * t_0 + 0
    assert torch.equal(_case_solver(case).solve(main, x0, labels, start_step=0, image=torch.zeros_like(x0)), plain)


@pytest.mark.parametrize("case", ["heun_bf16", "multistep2_bf16"])
def test_mask_identities(pair, case):
    main, x0, labels, image, mask = pair
    plain = _case_solver(case).solve(main, x0, labels)
    zeros = _case_solver(case).solve(main, x0, labels, image=torch.zeros_like(x0), mask=torch.zeros_like(mask))
    assert torch.equal(zeros, plain)                                        # nothing known: the unconditioned solve
    ones = _case_solver(case).solve(main, x0, labels, image=image, mask=torch.ones(8, 8, device=DEV))
    assert torch.equal(ones, image)                                         # everything known: the image
    for m in (mask, mask[:1], mask[1, 0].float(), mask.to(torch.uint8)):
        out = _case_solver(case).solve(main, x0, labels, image=image, mask=m, start_step=2)
        sel = m.bool().expand(x0.shape) if m.dim() == 4 else m.bool().expand(x0.shape)
        assert torch.equal(out[sel], image[sel])
        assert not torch.equal(out[~sel], plain[~sel]) and torch.isfinite(out).all()


def test_zero_churn_inpainting_is_deterministic_inpainting(pair):
    import tinyedm_amd as T
    main, x0, labels, image, mask = pair
    det = T.DeterministicSolver(**SCHED, seed=77)
    sto = T.StochasticSolver(**SCHED, S_churn=0.0, S_noise=1.003, seed=77)
    det.solve_index = sto.solve_index = 3
    for graph in (False, True):
        det.solve_index = sto.solve_index = 3
        a = det.solve(main, x0, labels, graph, image=image, mask=mask, start_step=1)
        b = sto.solve(main, x0, labels, graph, image=image, mask=mask, start_step=1)
        assert torch.equal(a, b)
        assert det.solve_index == sto.solve_index == 4
    assert list(det._graphs[main]) == list(sto._graphs[main])


def test_seed_and_solve_index_reproduce_inpainting(pair):
    main, x0, labels, image, mask = pair
    sel = mask.expand(x0.shape)
    s1, s2 = _case_solver("heun_bf16"), _case_solver("heun_bf16")
    a = [s1.solve(main, x0, labels, image=image, mask=mask) for _ in range(3)]
    b = [s2.solve(main, x0, labels, image=image, mask=mask) for _ in range(3)]
    assert s1.solve_index == s2.solve_index == 3
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2])
    s1.solve_index = 1
    assert torch.equal(s1.solve(main, x0, labels, image=image, mask=mask), a[1])
    s1.solve(main, x0, labels, image=image, start_step=3)           # SDEdit and plain solves draw nothing:
    s1.solve(main, x0, labels)
    assert s1.solve_index == 2                                      # the index stays
    s2.seed, s2.solve_index = 1235, 0
    other = s2.solve(main, x0, labels, image=image, mask=mask)
    assert torch.equal(other[sel], a[0][sel]) and torch.equal(other[sel], image[sel])
    assert not torch.equal(other[~sel], a[0][~sel])


@pytest.mark.parametrize("case", ["heun_bf16", "stochastic_bf16", "multistep3_bf16"])
def test_conditioned_hipgraph_replay_and_cache_key(pair, case):
    main, x0, labels, image, mask = pair
    sol = _case_solver(case)
    g = torch.Generator().manual_seed(9)
    image2 = (0.5 * torch.randn(3, 3, 8, 8, generator=g)).to(DEV)
    mask2 = (torch.rand(3, 1, 8, 8, generator=g) < 0.3).to(DEV)

    def both(**kw):
        i = sol.solve_index
        e = sol.solve(main, x0, labels, **kw)
        sol.solve_index = i
        r = sol.solve(main, x0, labels, graph=True, **kw)
        assert torch.equal(r, e)
        return r
    n = lambda: len(sol._graphs[main])
    a = both(image=image, start_step=3)                             # SDEdit: capture
    assert n() == 1
    assert not torch.equal(both(image=image2, start_step=3), a) and n() == 1       # a new image replays
    both(start_step=3)                                              # no image: another graph
    assert n() == 2
    b = both(image=image, mask=mask, start_step=3)                  # inpainting
    assert n() == 3
    both(image=image2, mask=mask, start_step=3)
    c = both(image=image, mask=mask2, start_step=3)                 # new mask content
    assert not torch.equal(c, b)
    sol.seed, sol.solve_index = 99, 0                               # new seed and index: device values
    d = both(image=image, mask=mask, start_step=3)
    assert not torch.equal(d, b) and n() == 3
    both(image=image, mask=mask[:1], start_step=3)                  # a new mask shape captures
    assert n() == 4
    sol.MAX_GRAPHS = 4
    both(image=image, mask=mask, start_step=4)                      # a new start_step captures; the oldest entry goes
    assert n() == 4
    both(image=image, mask=mask, start_step=3)                      # still cached
    assert n() == 4


def test_invert_hipgraph_replay_and_eviction(ops, pair):
    import tinyedm_amd as T
    main, x0, labels, image, mask = pair
    sol = T.DeterministicSolver(**SCHED)
    e = sol.invert(main, image, labels, end_step=2)
    assert torch.equal(sol.invert(main, image, labels, graph=True, end_step=2), e)
    assert torch.equal(sol.invert(main, image, labels, graph=True, end_step=2), e)
    assert len(sol._graphs[main]) == 1
    img2 = image.flip(0).contiguous()
    assert torch.equal(sol.invert(main, img2, labels, graph=True, end_step=2), sol.invert(main, img2, labels, end_step=2))
    assert len(sol._graphs[main]) == 1
    assert torch.equal(sol.invert(main, image, labels, graph=True, end_step=0), sol.invert(main, image, labels))
    assert len(sol._graphs[main]) == 2
    # a solve of the same shapes has its own entry, and the round trip runs through two graphs
    lat = sol.invert(main, image, labels, graph=True, end_step=2)
    back = sol.solve(main, lat, labels, graph=True, start_step=2)
    assert torch.equal(back, sol.solve(main, lat, labels, start_step=2)) and len(sol._graphs[main]) == 3
    # eviction: MAX_GRAPHS = 1 releases the launch-table slots and plan pins of the entry that goes
    sol2 = T.DeterministicSolver(**SCHED)
    sol2.MAX_GRAPHS = 1
    st = ops._tables._state(torch.cuda.current_device())
    den = main.denoiser
    out_a = sol2.solve(main, x0, labels, graph=True, image=image, mask=mask, start_step=3)
    pins = sum(p.pins for p in den._plans.values())
    sol2.solve(main, x0, labels, graph=True, image=image, start_step=4)             # evicts the first
    assert len(sol2._graphs[main]) == 1 and sum(p.pins for p in den._plans.values()) == pins
    pool = st["pool_i"]
    sol2.solve_index = 0
    assert torch.equal(sol2.solve(main, x0, labels, graph=True, image=image, mask=mask, start_step=3), out_a)
    sol2.invert(main, image, labels, graph=True, end_step=5)
    assert len(sol2._graphs[main]) == 1 and sum(p.pins for p in den._plans.values()) <= pins
    assert st["pool_i"] == pool                     # the re-captures drew their slots from the released ones


# ------------------------------------------------------------------ analytic denoisers
MU, SD = 0.3, 0.5


def _gaussian(x, s, labels=None):
    s = s.double()
    return (MU + SD ** 2 / (SD ** 2 + s * s) * (x.double() - MU)).float()


def _gaussian64(x, s):
    return MU + SD ** 2 / (SD ** 2 + s * s) * (x - MU)


def _invert64(img, t, k):
    """Heun up the fp64 table from t_{N-1} to t_k; the unit-scale latent"""
    x = img.double()
    for i in range(len(t) - 2, k, -1):
        t0, t1 = t[i], t[i - 1]
        dx = (x - _gaussian64(x, t0)) / t0
        x1 = x + (t1 - t0) * dx
        x = x + (t1 - t0) * (0.5 * dx + 0.5 * (x1 - _gaussian64(x1, t1)) / t1)
    return x / t[k]


def _solve64(lat, t, k):
    N = len(t) - 1
    x1 = lat.double() * t[k]
    for i in range(k, N):
        x, t0, t1 = x1, t[i], t[i + 1]
        dx = (x - _gaussian64(x, t0)) / t0
        x1 = x + (t1 - t0) * dx
        if i < N - 1:
            x1 = x + (t1 - t0) * (0.5 * dx + 0.5 * (x1 - _gaussian64(x1, t1)) / t1)
    return x1


def _analytic_image():
    g = torch.Generator().manual_seed(0)
    return (MU + SD * torch.randn(64, 192, generator=g, dtype=torch.float64)).float().reshape(64, 3, 8, 8)


@pytest.mark.parametrize("end", [0, 6])
def test_inversion_is_second_order(ops, end):
    import tinyedm_amd as T
    img = _analytic_image()
    err, err64 = {}, {}
    for N in (32, 64, 128):
        sol = T.DeterministicSolver(num_steps=N)
        t = sol.t_steps.double()
        exact = (MU + math.sqrt(SD ** 2 + t[end].item() ** 2) / math.sqrt(SD ** 2 + t[N - 1].item() ** 2)
                 * (img.double() - MU)) / t[end]
        err[N] = rel(sol.invert(_gaussian, img.to(DEV), end_step=end), exact)
        err64[N] = rel(_invert64(img, t, end), exact)
        print(f"inversion end {end} N {N}: GPU {err[N]:.4e}, fp64 restatement {err64[N]:.4e}")
    for N in (32, 64, 128):
        assert abs(err[N] - err64[N]) <= 0.10 * err64[N] + 1e-5, (N, err[N], err64[N])
    assert err[32] / err[64] >= 3 and err[64] / err[128] >= 3, err


@pytest.mark.parametrize("end", [0, 6])
def test_round_trip_closes(ops, end):
    import tinyedm_amd as T
    img = _analytic_image()
    err, err64 = {}, {}
    for N in (32, 64, 128):
        sol = T.DeterministicSolver(num_steps=N)
        t = sol.t_steps.double()
        lat = sol.invert(_gaussian, img.to(DEV), end_step=end)
        err[N] = rel(sol.solve(_gaussian, lat, start_step=end), img)
        err64[N] = rel(_solve64(_invert64(img, t, end), t, end), img)
        print(f"round trip end {end} N {N}: GPU {err[N]:.4e}, fp64 restatement {err64[N]:.4e}")
    for N in (32, 64, 128):
        assert abs(err[N] - err64[N]) <= 0.10 * err64[N] + 1e-5, (N, err[N], err64[N])
    assert err[32] > err[64] > err[128], err


def _mixture(means):
    means = means.to(DEV)
    stds = torch.tensor([0.1, 0.2, 0.3, 0.15], dtype=torch.float64, device=DEV)
    logw = torch.tensor([0.1, 0.2, 0.3, 0.4], dtype=torch.float64, device=DEV).log()

    def D(x, s, labels=None):
        """the posterior mean E[y | y + s n = x] of the mixture, in fp64"""
        xs = x.double().reshape(x.shape[0], 1, -1)
        v = stds ** 2 + s.double() ** 2
        logp = logw - 0.5 * ((xs - means) ** 2).sum(-1) / v - 0.5 * means.shape[1] * v.log()
        p = torch.softmax(logp, dim=1)
        post = means + (stds ** 2 / v)[:, None] * (xs - means)
        return (p[:, :, None] * post).sum(1).reshape(x.shape).to(x.dtype)
    return D


@pytest.mark.parametrize("case", ["heun", "stochastic", "multistep"])
def test_inpainting_on_the_mixture(ops, case):
    import tinyedm_amd as T
    g = torch.Generator().manual_seed(0)
    means = 0.5 * torch.randn(4, 192, generator=g, dtype=torch.float64)
    x0 = torch.randn(16, 192, generator=g, dtype=torch.float64).float().reshape(16, 3, 8, 8).to(DEV)
    image = (means[1] + 0.2 * torch.randn(16, 192, generator=g, dtype=torch.float64)).float().reshape(16, 3, 8, 8).to(DEV)
    D = _mixture(means)
    mask = torch.zeros(8, 8, dtype=torch.bool, device=DEV)
    mask[:, :4] = True                              # the left half is known
    sol = {"heun": T.DeterministicSolver(num_steps=18, seed=5), "multistep": T.MultistepSolver(num_steps=18, seed=5),
           "stochastic": T.StochasticSolver(num_steps=18, S_churn=10.0, seed=5)}[case]
    plain = sol.solve(D, x0)
    out = sol.solve(D, x0, image=image, mask=mask)
    sel = mask.expand(x0.shape)
    assert torch.isfinite(out).all()
    assert torch.equal(out[sel], image[sel])
    assert not torch.equal(out[~sel], plain[~sel])
    ops.check_health(DEV, "inpainting on the mixture")


# ------------------------------------------------------------------ generate CLI
CLI = ["--config_name", "cifar10_cond", "--num_samples", "4", "--batch_size", "4", "--num_steps", "4", "--num_classes",
       "10", "--image_size", "32", "--num_workers", "0"]


def _generate(out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "generate.py"), "--output_dir", str(out), *CLI, *extra]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def _load(d):
    from PIL import Image
    return np.stack([np.asarray(Image.open(os.path.join(d, f"{i}.png"))).astype(np.int64) for i in range(4)])


def test_generate_cli_image_conditioned(ops, tmp_path):
    _generate(tmp_path / "plain")
    plain = _load(tmp_path / "plain")
    assert plain.shape == (4, 32, 32, 3)
    # inpainting: the box is regenerated, everything outside is the input within the uint8 round trip
    _generate(tmp_path / "box", "--init_dir", str(tmp_path / "plain"), "--mask_box", "8", "4", "24", "20")
    box = _load(tmp_path / "box")
    inside = np.zeros((32, 32), bool)
    inside[4:20, 8:24] = True                       # X0 Y0 X1 Y1 = 8 4 24 20: rows 4..19, columns 8..23
    assert np.abs(box - plain)[:, ~inside].max() <= 1
    assert all((box[i][inside] != plain[i][inside]).any() for i in range(4))
    # SDEdit: differs from the inputs and from a plain run
    _generate(tmp_path / "sdedit", "--init_dir", str(tmp_path / "plain"), "--start_step", "2")
    sdedit = _load(tmp_path / "sdedit")
    assert all((sdedit[i] != plain[i]).any() for i in range(4))
    _generate(tmp_path / "plain2")
    assert np.array_equal(_load(tmp_path / "plain2"), plain)
    # an argument error leaves before anything is loaded
    cmd = [sys.executable, os.path.join(ROOT, "experiments", "generate.py"), "--output_dir", str(tmp_path / "x"), *CLI,
           "--start_step", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--init_dir" in r.stderr


def test_generate_cli_invert_round_trip(ops, tmp_path):
    import tinyedm_amd as T
    from tinyedm_amd import generate as G, networks
    from tinyedm_amd.config import compose, instantiate
    from tinyedm_amd.datamodules import RandomNoiseDataModule
    _generate(tmp_path / "plain")
    plain = _load(tmp_path / "plain")
    lat_path = tmp_path / "lat.pt"
    _generate(tmp_path / "unused", "--init_dir", str(tmp_path / "plain"), "--invert_to", str(lat_path), "--start_step", "1")
    saved = torch.load(lat_path)
    assert saved["latents"].shape == (4, 3, 32, 32) and saved["end_step"] == 1 and saved["num_steps"] == 4
    assert not os.path.exists(tmp_path / "unused" / "0.png")
    # the same model in this process (the CLI's random init of the config), the same round trip
    cfg = compose("cifar10_cond", os.path.join(ROOT, "experiments", "conf"))
    networks.manual_seed(cfg.seed)
    torch.manual_seed(cfg.seed)
    model = instantiate(cfg.model).to(DEV).eval()
    model.denoiser.set_eval_dtype("f32x3")
    sol = T.DeterministicSolver(num_steps=4)
    imgs = G.load_images(str(tmp_path / "plain"), G.CIFAR_MEAN, G.CIFAR_STD, 32, 3).to(DEV)
    _, labels = next(iter(RandomNoiseDataModule(4, 0, 32, 4, 10, seed=0).predict_dataloader()))
    assert torch.equal(saved["class_labels"], labels.cpu())
    mean = torch.tensor(G.CIFAR_MEAN, device=DEV)
    std = torch.tensor(G.CIFAR_STD, device=DEV)

    def levels(x):
        return ops.prediction_to_u8_nhwc(x.float().contiguous(), mean, std).cpu().numpy().astype(np.int64)
    with torch.no_grad():
        lat = sol.invert(model, imgs, labels, end_step=1)
        bound = int(np.abs(levels(sol.solve(model, lat, labels, start_step=1)) - plain).max())
        back = levels(sol.solve(model, saved["latents"].to(DEV), labels, start_step=1))
    got = int(np.abs(back - plain).max())
    print(f"CLI invert round trip: {got} levels, in-process round trip {bound} levels")
    assert got <= bound, (got, bound)
    assert rel(saved["latents"], lat) <= 1e-6
