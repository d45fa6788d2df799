"""The input gradient of the denoiser on the GPU: the conv_in dgrad kernel against fp64 of the same bf16 operands and its
exact properties; the whole-network VJP against autograd through the CPU oracle, judged by the oracle's own bf16 / fp32
distance; that input_vjp computes data gradients only (no weight-side launch, no parameter state touched, the next training
step bit-identical); that eval-mode autograd delivers the same bits; and the error paths."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import dps_ref as P
from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs
from parity_log import record

DEV = "cuda"
U = 2.0 ** -24
TINY_C0 = tiny_cfgs()[1].encoder_out_channels[0]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _dev(t, offset_bytes=0):
    """t on the device, `offset_bytes` behind a 16-byte boundary"""
    n = offset_bytes // t.element_size()
    buf = torch.empty(t.numel() + n, device=DEV, dtype=t.dtype)
    out = buf[n:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == offset_bytes and out.is_contiguous()
    return out


# ------------------------------------------------------------------ 1. the kernel
KERNEL_CASES = [(3, 3, 32, 32, 128), (2, 1, 28, 28, 128), (1, 4, 32, 32, 192), (5, 3, 6, 10, 32), (2, 3, 8, 8, TINY_C0)]
SD = 0.5


def _operands(case):
    B, Cimg, H, W, C0 = case
    g = torch.Generator().manual_seed(sum(case))
    gy = (0.5 * torch.randn(B, H, W, C0, generator=g)).bfloat16()
    w = (torch.randn(C0, Cimg, 3, 3, generator=g) / math.sqrt(9 * (Cimg + 1))).bfloat16()
    gD = torch.randn(B, Cimg, H, W, generator=g)
    sigma = torch.logspace(math.log10(0.002), math.log10(80.0), B) if B > 1 else torch.tensor([0.7])
    return gy, w, gD, sigma.float()


def _pack(ops, w):
    """fp32 [C0][NT]: pack[co][(ky * 3 + kx) * Cimg + c] = w[co, c, ky, kx]"""
    C0, Cimg = w.shape[:2]
    pack = torch.zeros(C0, ops.conv_in_dgrad_pack_cols(Cimg))
    pack[:, :9 * Cimg] = w.float().permute(0, 2, 3, 1).reshape(C0, 9 * Cimg)
    return pack.to(DEV)


@pytest.fixture(scope="module")
def kernel_refs():
    """the fp64 result and its magnitude per case, with and without gD: computed once"""
    out = {}
    for case in KERNEL_CASES:
        gy, w, gD, sigma = _operands(case)
        for with_gd in (False, True):
            out[case, with_gd] = P.conv_in_dgrad(gy.double(), w.double(), gD.double() if with_gd else None, sigma.double(), SD)
    return out


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "misaligned4"])
@pytest.mark.parametrize("with_gd", [False, True], ids=["nogD", "gD"])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=["x".join(map(str, c)) for c in KERNEL_CASES])
def test_conv_in_dgrad_vs_fp64(ops, kernel_refs, case, with_gd, offset):
    B, Cimg, H, W, C0 = case
    gy, w, gD, sigma = _operands(case)
    ref, mag = kernel_refs[case, with_gd]
    got = ops.conv_in_dgrad(_dev(gy, offset), _pack(ops, w), _dev(gD, offset) if with_gd else None, sigma.to(DEV), SD).cpu()
    assert got.shape == (B, Cimg, H, W) and got.dtype == torch.float32
    lim = (9 * C0 + 4) * U * mag            # per output element
    err = (got.double() - ref).abs()
    worst = (err / lim.clamp_min(1e-300)).max().item()
    print(f"conv_in_dgrad {case} gD={with_gd} offset {offset}: max err / limit {worst:.3e}, rel {rel(got, ref):.3e}")
    record(f"input_vjp/conv_in_dgrad_{'x'.join(map(str, case))}_{'gD' if with_gd else 'nogD'}_o{offset}_vs_fp64", worst, 1.0)
    assert bool((err <= lim).all()), worst
    assert rel(got, ref) > 0 or not with_gd        # (an fp32 result is not the fp64 one)


@pytest.mark.parametrize("case", KERNEL_CASES, ids=["x".join(map(str, c)) for c in KERNEL_CASES])
def test_conv_in_dgrad_exact_properties(ops, case):
    B, Cimg, H, W, C0 = case
    gy, w, gD, sigma = _operands(case)
    pack = _pack(ops, w)
    full = ops.conv_in_dgrad(_dev(gy), pack, _dev(gD), sigma.to(DEV), SD)
    # both memory paths give the same bits
    assert torch.equal(ops.conv_in_dgrad(_dev(gy, 4), pack, _dev(gD, 4), sigma.to(DEV), SD), full)
    # a sample's result does not depend on B
    for b in sorted({0, B // 2, B - 1}):
        one = ops.conv_in_dgrad(_dev(gy[b:b + 1]), pack, _dev(gD[b:b + 1]), sigma[b:b + 1].to(DEV), SD)
        assert torch.equal(one, full[b:b + 1]), b
    # gy = 0 gives exactly c_skip * gD: c_skip as the kernel forms it (gD = 1), one rounded product per element
    zero = torch.zeros_like(gy)
    c_skip = ops.conv_in_dgrad(_dev(zero), pack, torch.ones_like(gD).to(DEV), sigma.to(DEV), SD)
    assert torch.equal(c_skip, c_skip[:, :1, :1, :1].expand_as(c_skip))
    exact = SD ** 2 / (sigma.double() ** 2 + SD ** 2)
    assert ((c_skip[:, 0, 0, 0].cpu().double() - exact).abs() <= 2 * U * exact).all()
    assert torch.equal(ops.conv_in_dgrad(_dev(zero), pack, _dev(gD), sigma.to(DEV), SD), c_skip * gD.to(DEV))
    # and without gD exactly zero
    assert not ops.conv_in_dgrad(_dev(zero), pack, None, sigma.to(DEV), SD).any()


def test_conv_in_dgrad_refuses_bad_arguments(ops):
    gy, w, gD, sigma = _operands(KERNEL_CASES[3])
    pack = _pack(ops, w)
    with pytest.raises(ValueError):
        ops.conv_in_dgrad(_dev(gy).float(), pack, None, sigma.to(DEV), SD)
    with pytest.raises(ValueError):
        ops.conv_in_dgrad(_dev(gy), pack[:-1], None, sigma.to(DEV), SD)
    with pytest.raises(ValueError):
        ops.conv_in_dgrad(_dev(gy), pack, _dev(gD[:, :2]), sigma.to(DEV), SD)
    with pytest.raises(ValueError):
        ops.conv_in_dgrad(_dev(gy), pack, _dev(gD[:1]), sigma.to(DEV), SD)


# ------------------------------------------------------------------ 2. the whole network against the oracle
def _edm(Pm, ecfg, dcfg, arena=False, dtype="bf16"):
    import tinyedm_amd as T
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), 0.0,
                     dcfg.sigma_data, dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    emb.load_state_dict({k[len("embedding."):]: v for k, v in Pm.items() if k.startswith("embedding.")}, strict=True)
    den.load_state_dict({k[len("denoiser."):]: v for k, v in Pm.items() if k.startswith("denoiser.")}, strict=True)
    den.set_eval_dtype(dtype)
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                  steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01).to(DEV).eval()
    opt = None
    if arena:
        opt = T.FusedAdam(list(model.parameters()), lr=1e-3)
        opt.zero_grad()
    return model, opt


def _net_case(name):
    if name == "tiny":
        e, d = tiny_cfgs(None)
        return e, d, (2, 3, 8, 8)
    if name == "tiny_cond":
        e, d = tiny_cfgs(10)
        return e, d, (2, 3, 8, 8)
    if name == "cifar10":
        e, d = O.cifar10_cfg(None)
        return e, d, (2, 3, 32, 32)
    from test_configs_gpu import mnist_cfg
    e, d = mnist_cfg()
    return e, d, (2, 1, 28, 28)


def _net_inputs(ecfg, shape, seed=13):
    g = torch.Generator().manual_seed(seed)
    x = 0.5 * torch.randn(shape, generator=g) + 0.1
    sigma = torch.tensor([0.4, 2.5])[:shape[0]]
    x = x + sigma.view(-1, 1, 1, 1) * torch.randn(shape, generator=g)
    labels = torch.randint(0, ecfg.num_classes, (shape[0],), generator=g) if ecfg.num_classes else None
    cot = torch.randn(shape, generator=g)
    return x, sigma, labels, cot


def _oracle_vjp(Pm, e, d, x, sigma, labels, cot, bf16):
    xr = x.clone().requires_grad_()
    D = O.edm_forward(Pm, e, d, xr, sigma, labels, bf16=bf16)
    (g,) = torch.autograd.grad(D, xr, cot)
    return D.detach(), g


@pytest.mark.parametrize("name", ["tiny", "tiny_cond", "cifar10", "mnist"])
def test_whole_network_input_gradient_vs_oracle(name):
    """The bf16 path's rounding error through the full depth cannot be derived: the yardstick is the oracle's own distance
    e_ref between its bf16-rounding and fp32 input gradients; the HIP gradient (same rounding points as the bf16 oracle, other
    accumulation orders) may be at most 2 e_ref from either."""
    import tinyedm_amd as T
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    e, d, shape = _net_case(name)
    d.dropout_rate = 0.0
    Pm = O.init_params(e, d, torch.Generator().manual_seed(21), gains_nonzero=True)
    x, sigma, labels, cot = _net_inputs(e, shape)
    model, _ = _edm(Pm, e, d)
    lab = None if labels is None else labels.to(DEV)
    with torch.no_grad():
        D_plain = model(x.to(DEV), sigma.to(DEV), lab)
    D, gx = T.input_vjp(model, x.to(DEV), sigma.to(DEV), lab, cot.to(DEV))
    assert D.dtype == gx.dtype == torch.float32 and gx.shape == x.shape and not gx.requires_grad
    assert torch.equal(D, D_plain)                  # the forward of the VJP is the no_grad bf16 forward, bit for bit
    _, g32 = _oracle_vjp(Pm, e, d, x, sigma, labels, cot, False)
    _, g16 = _oracle_vjp(Pm, e, d, x, sigma, labels, cot, True)
    e_ref = rel(g16, g32)
    d32, d16 = rel(gx, g32), rel(gx, g16)
    print(f"input gradient {name} {shape}: e_ref (oracle bf16 vs fp32) {e_ref:.3e}; HIP vs fp32 {d32:.3e}, vs bf16 {d16:.3e} "
          f"(limit {2 * e_ref:.3e})")
    record(f"input_vjp/{name}_e_ref_oracle_bf16_vs_fp32", e_ref, 2 * e_ref)
    record(f"input_vjp/{name}_hip_vs_fp32_oracle", d32, 2 * e_ref)
    record(f"input_vjp/{name}_hip_vs_bf16_oracle", d16, 2 * e_ref)
    assert e_ref > 0
    assert d32 <= 2 * e_ref and d16 <= 2 * e_ref, (d32, d16, e_ref)
    # the J^T v is not the trivial c_skip * v
    c_skip = (d.sigma_data ** 2 / (sigma ** 2 + d.sigma_data ** 2)).view(-1, 1, 1, 1)
    assert rel(c_skip * cot, g32) > 10 * e_ref


# ------------------------------------------------------------------ 3. dgrad-only really is; eval-mode autograd agrees
@pytest.fixture(scope="module")
def arena_model():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    e, d = tiny_cfgs(10)
    Pm = O.init_params(e, d, torch.Generator().manual_seed(7), gains_nonzero=True)
    model, opt = _edm(Pm, e, d, arena=True)
    x, sigma, labels, cot = _net_inputs(e, (2, 3, 8, 8))
    return model, opt, x.to(DEV), sigma.to(DEV), labels.to(DEV), cot.to(DEV)


def _train_step(model, opt, x, labels):
    import tinyedm_amd as T
    from tinyedm_amd import networks as N
    T.manual_seed(99)
    model.train()
    opt.zero_grad()
    loss = model.training_step((x, labels), 0)
    loss.backward()
    torch.cuda.synchronize()
    grads = opt.arena.grad.clone()
    model.eval()
    opt.zero_grad()
    N.reset_backward_state()
    return loss.detach().clone(), grads


def test_input_vjp_computes_data_gradients_only(arena_model):
    import tinyedm_amd as T
    from tinyedm_amd import _lib, networks as N
    model, opt, x, sigma, labels, cot = arena_model
    clean = 0.5 * torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1)).to(DEV)
    theta0 = opt.arena.theta.clone()

    def restore():      # (a training forward normalises the master weights in place: both steps start from the same ones)
        with torch.no_grad():
            opt.arena.theta.copy_(theta0)
        N.bump_weight_epoch()
    loss_a, grads_a = _train_step(model, opt, clean, labels)
    restore()
    theta1 = opt.arena.theta.clone()
    opt.arena.grad.fill_(0.25)
    before = opt.arena.grad.clone()
    step, epoch = N.rng.step, N.FORWARD_EPOCH
    flags = {n: getattr(p, "_edm_deferred", False) for n, p in model.named_parameters()}
    calls = []
    real = _lib.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    _lib.call = spy
    try:
        D, gx = T.input_vjp(model, x, sigma, labels, cot)
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    assert torch.isfinite(gx).all() and gx.abs().max() > 0
    bad = [n for n in calls if any(w in n for w in ("wgrad", "mod_finish", "linear_wgrad"))]
    assert not bad, bad
    assert "edm_conv_in_dgrad" in calls
    assert torch.equal(opt.arena.grad, before) and all(torch.equal(p.grad, torch.full_like(p.grad, 0.25))
                                                       for p in model.parameters())
    assert torch.equal(opt.arena.theta, theta1)
    assert (N.rng.step, N.FORWARD_EPOCH) == (step, epoch)
    assert flags == {n: getattr(p, "_edm_deferred", False) for n, p in model.named_parameters()}
    assert not N._tail_slot and not N._sg_pending and not N._bwd_end_queued and not N._fin_pending and not N._w3_pending
    assert not N._DGRAD_ONLY[0] and not model.training
    # a training step afterwards is the training step without the VJP call in between, bit for bit
    opt.zero_grad()
    loss_b, grads_b = _train_step(model, opt, clean, labels)
    restore()
    assert torch.equal(loss_a, loss_b) and torch.equal(grads_a, grads_b)
    assert grads_a.abs().max() > 0


def test_eval_mode_autograd_delivers_the_same_input_gradient(arena_model):
    import tinyedm_amd as T
    from tinyedm_amd import networks as N
    model, opt, x, sigma, labels, cot = arena_model
    model.eval()
    D_ref, gx_ref = T.input_vjp(model, x, sigma, labels, cot)

    def backward(requires):
        opt.zero_grad()
        opt.arena.grad.zero_()
        xr = x.clone().requires_grad_(requires)
        D = model(xr, sigma, labels)
        D.backward(cot)
        torch.cuda.synchronize()
        N.reset_backward_state()
        return D.detach(), xr.grad, opt.arena.grad.clone()
    D1, g1, pg1 = backward(True)
    D0, g0, pg0 = backward(False)
    assert g0 is None and g1 is not None and g1.dtype == torch.float32
    assert torch.equal(D1, D_ref) and torch.equal(D0, D_ref)
    assert torch.equal(g1, gx_ref)
    assert pg1.abs().max() > 0 and torch.equal(pg1, pg0)        # the parameter gradients do not notice
    opt.zero_grad()


def test_training_mode_autograd_delivers_an_input_gradient(arena_model):
    model, opt, x, sigma, labels, cot = arena_model
    import tinyedm_amd as T
    T.manual_seed(3)
    model.train()
    try:
        opt.zero_grad()
        xr = x.clone().requires_grad_()
        model(xr, sigma, labels).backward(cot)
        torch.cuda.synchronize()
    finally:
        model.eval()
        opt.zero_grad()
    _, gx = T.input_vjp(model, x, sigma, labels, cot)
    assert xr.grad is not None and torch.isfinite(xr.grad).all()
    assert rel(xr.grad, gx) <= 5e-2         # (the training forward re-normalises the weights: close, not equal)


# ------------------------------------------------------------------ 4. error paths
@pytest.mark.parametrize("dtype", ["f32", "f32x3"])
def test_fp32_evaluation_paths_have_no_backward(arena_model, dtype):
    import tinyedm_amd as T
    model, opt, x, sigma, labels, cot = arena_model
    model.denoiser.set_eval_dtype(dtype)
    try:
        with pytest.raises(ValueError, match=r"set_eval_dtype\(\"bf16\"\).*--network_dtype bf16"):
            T.input_vjp(model, x, sigma, labels, cot)
        with pytest.raises(RuntimeError, match="forward-only"):     # the existing error of autograd on that path stays
            model(x.clone().requires_grad_(), sigma, labels)
    finally:
        model.denoiser.set_eval_dtype("bf16")


def test_input_vjp_refuses_bad_tensors(arena_model):
    import tinyedm_amd as T
    model, opt, x, sigma, labels, cot = arena_model
    with pytest.raises(ValueError, match="GPU"):
        T.input_vjp(model, x.cpu(), sigma, labels, cot)
    with pytest.raises(ValueError, match="cotangent must have D's shape"):
        T.input_vjp(model, x, sigma, labels, cot[:1])
    with pytest.raises(ValueError, match="cotangent must have D's shape"):
        T.input_vjp(model, x, sigma, labels, cot[:, :1])
    # a refused call leaves nothing behind: the next one is the first one's result
    a = T.input_vjp(model, x, sigma, labels, cot)[1]
    assert torch.equal(a, T.input_vjp(model, x, sigma, labels, cot)[1])
