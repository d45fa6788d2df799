"""Paired image quality on the GPU: edm_pair_ssim and edm_f32_pair_feature_distance against the numpy fp64 reference
(tests/quality_ref.py), the exact integer squared error, the region rules, batch and load-path invariance bit for bit,
PairedQuality end to end on the tiny network, and the two command lines.

Tolerances.  SSIM: absolute 1e-9, derived: each filtered moment carries a relative error of at most about win^2 2^-53 =
2.5e-14 of L^2 at win 15; the variance terms are divided by at least C2 = 9e-4 L^2, which gives at most about 1e-10 per
implementation and under 4e-10 for two; the mean terms err relative to themselves.  Feature distance: relative 1e-9 (all
terms are non-negative; n 2^-53 at 8e5 terms is 9e-11)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import quality_ref as R
from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs

DEV = "cuda"
SSIM_TOL = 1e-9
FD_RTOL = 1e-9
SHAPES = [(3, 11, 11, 1), (2, 12, 13, 3), (5, 32, 32, 3), (2, 64, 64, 3), (1, 37, 70, 3)]      # (n, H, W, C)
WINDOWS = ["gauss11", "uniform7", "gauss3", "gauss15"]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def _window(name):
    from tinyedm_amd import compare
    return {"gauss11": lambda: compare.gaussian_window(11, 1.5), "uniform7": lambda: compare.uniform_window(7),
            "gauss3": lambda: compare.gaussian_window(3, 1.5), "gauss15": lambda: compare.gaussian_window(15, 1.5)}[name]()


@functools.lru_cache(maxsize=None)
def _pair_u8(shape):
    """a smooth random image and a noisy, partly flat copy: uint8 [n, H, W, C] (flat regions are where fp32 would fail)"""
    rng = np.random.default_rng(sum(shape))
    n, H, W, C = shape
    base = rng.integers(0, 256, (n, (H + 3) // 4, (W + 3) // 4, C)).repeat(4, axis=1).repeat(4, axis=2)[:, :H, :W]
    a = np.clip(base + rng.normal(0, 6, shape), 0, 255).round().astype(np.uint8)
    b = np.clip(a + rng.normal(0, 12, shape), 0, 255).round().astype(np.uint8)
    b[:, : H // 3] = 200
    a[:, : H // 4] = 200
    return a, b


@functools.lru_cache(maxsize=None)
def _ref(shape, wname, kind):
    a, b = _pair_u8(shape)
    if kind == "f32":
        a, b = _as_f32(a), _as_f32(b)
    return R.pair_ssim(a, b, _window(wname), 255.0 if kind == "u8" else 1.0)


def _as_f32(u8):
    """float32 [n, C, H, W] in [0, 1] with fractional detail below a grey level"""
    x = u8.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(x * np.float32(0.999) + np.float32(1e-4))


def _fits(shape, wname):
    return len(_window(wname)) <= min(shape[1], shape[2])


# ------------------------------------------------------------------------------------------------ SSE and SSIM
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_sse_u8_exact(ops, shape):
    a, b = _pair_u8(shape)
    wname = "gauss11"
    ssim, sse, counts = ops.pair_ssim(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), _window(wname), 255.0)
    want_ssim, want_sse, want_counts = _ref(shape, wname, "u8")
    assert sse.dtype == torch.float64 and tuple(sse.shape) == (shape[0], shape[3])
    assert torch.equal(sse.cpu(), torch.from_numpy(want_sse)), "the squared error of uint8 images is an exact integer"
    assert counts.dtype == torch.int32 and torch.equal(counts.cpu(), torch.from_numpy(want_counts))
    assert int(counts[0, 0]) == shape[1] * shape[2] and int(counts[0, 1]) == (shape[1] - 10) * (shape[2] - 10)


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("wname", WINDOWS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_ssim_against_reference(ops, shape, wname, kind):
    if not _fits(shape, wname):
        a, b = _pair_u8(shape)
        with pytest.raises(ValueError, match="does not fit"):
            ops.pair_ssim(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), _window(wname), 255.0)
        return
    a, b = _pair_u8(shape)
    L = 255.0
    if kind == "f32":
        a, b, L = _as_f32(a), _as_f32(b), 1.0
    ssim, sse, counts = ops.pair_ssim(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), _window(wname), L)
    want, want_sse, want_counts = _ref(shape, wname, kind)
    err = float(np.abs(ssim.cpu().numpy() - want).max())
    print(f"ssim {shape} {wname} {kind}: max abs err {err:.3e} (values {want.min():.4f} .. {want.max():.4f})")
    assert ssim.dtype == torch.float64 and err <= SSIM_TOL
    assert torch.equal(counts.cpu(), torch.from_numpy(want_counts))
    if kind == "f32":
        assert np.allclose(sse.cpu().numpy(), want_sse, rtol=1e-12, atol=0)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_ssim_identical_and_constant(ops, kind):
    shape = (2, 37, 70, 3)
    a, _ = _pair_u8(shape)
    L, p, q = 255.0, 37, 201
    cp, cq = np.full((1, 16, 40, 2), p, np.uint8), np.full((1, 16, 40, 2), q, np.uint8)
    if kind == "f32":
        a, cp, cq, L = _as_f32(a), _as_f32(cp), _as_f32(cq), 1.0
    dev = lambda x: torch.from_numpy(x).to(DEV)        # noqa: E731
    for wname in WINDOWS:
        w = _window(wname)
        s, sse, _ = ops.pair_ssim(dev(a), dev(a.copy()), w, L)
        assert float((s - 1.0).abs().max()) <= SSIM_TOL and not bool(sse.any()), wname
        s, _, _ = ops.pair_ssim(dev(cp), dev(cp.copy()), w, L)
        assert float((s - 1.0).abs().max()) <= SSIM_TOL, wname
        s, sse, counts = ops.pair_ssim(dev(cp), dev(cq), w, L)
        pv, qv = (float(cp.flat[0]), float(cq.flat[0]))
        c1 = (0.01 * L) ** 2
        assert float((s - (2 * pv * qv + c1) / (pv * pv + qv * qv + c1)).abs().max()) <= SSIM_TOL, wname
        if kind == "u8":
            assert torch.equal(sse.cpu(), torch.full((1, 2), float((q - p) ** 2 * 16 * 40), dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ regions
def _regions(n, H, W):
    rng = np.random.default_rng(H * W)
    box = np.zeros((n, H, W), np.uint8)
    box[:, H // 4: H // 4 + H // 2, W // 3: W // 3 + W // 2] = 1
    irregular = (rng.random((n, H, W)) < 0.4).astype(np.uint8) * 7       # (non-zero = counted, not only 1)
    shared = (rng.random((1, H, W)) < 0.6).astype(np.uint8)
    return {"box": box, "irregular": irregular, "broadcast": shared}


@pytest.mark.parametrize("kind", ["box", "irregular", "broadcast"])
@pytest.mark.parametrize("shape", [(2, 12, 13, 3), (3, 37, 70, 2)], ids=str)
def test_regions(ops, shape, kind):
    a, b = _pair_u8(shape)
    region = _regions(*shape[:3])[kind]
    for wname in ("gauss11", "gauss3"):
        w = _window(wname)
        ssim, sse, counts = ops.pair_ssim(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), w, 255.0,
                                          torch.from_numpy(region).to(DEV))
        want, want_sse, want_counts = R.pair_ssim(a, b, w, 255.0, region)
        assert torch.equal(counts.cpu(), torch.from_numpy(want_counts)), (kind, wname)
        assert torch.equal(sse.cpu(), torch.from_numpy(want_sse)), (kind, wname)
        assert 0 < int(counts[:, 1].min()) and int(counts[:, 0].max()) < shape[1] * shape[2]
        assert float(np.abs(ssim.cpu().numpy() - want).max()) <= SSIM_TOL, (kind, wname)


def test_region_empty_gives_nan(ops):
    shape = (2, 12, 13, 3)
    a, b = _pair_u8(shape)
    region = np.zeros((2, 12, 13), np.uint8)
    region[1, 0, :] = 1                                 # image 1: counted pixels on the border, no counted centre
    ssim, sse, counts = ops.pair_ssim(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), _window("gauss3"), 255.0,
                                      torch.from_numpy(region).to(DEV))
    assert bool(torch.isnan(ssim).all()) and counts.cpu().tolist() == [[0, 0], [13, 0]]
    d = a[1, 0].astype(np.int64) - b[1, 0].astype(np.int64)
    assert torch.equal(sse.cpu(), torch.tensor([[0.0] * 3, (d * d).sum(axis=0).astype(np.float64).tolist()], dtype=torch.float64))


def test_ssim_beyond_one_launch(ops):
    """more (image, channel, tile) workgroups than one launch holds (2^23): the rows behind the seam against the same
    pairs scored alone, bit for bit, the squared error of every row against integer arithmetic, and SSIM of every row
    against the single 3 x 3 window written out in torch fp64 on the device (the data is too large for the numpy path)"""
    n, seam = (1 << 23) + 3, 1 << 23
    g = torch.Generator(device=DEV).manual_seed(11)
    a = torch.randint(0, 256, (n, 3, 3, 1), dtype=torch.uint8, device=DEV, generator=g)
    b = (a.int() + torch.randint(-30, 31, a.shape, device=DEV, generator=g)).clamp(0, 255).to(torch.uint8)
    w = _window("gauss3")
    ssim, sse, counts = ops.pair_ssim(a, b, w, 255.0)
    assert tuple(ssim.shape) == (n, 1) and bool((counts == torch.tensor([9, 1], dtype=torch.int32, device=DEV)).all())
    d = a.view(n, 9).long() - b.view(n, 9).long()
    assert torch.equal(sse.view(n), (d * d).sum(dim=1).double())
    for lo in (0, seam - 2):
        part = ops.pair_ssim(a[lo:lo + 5], b[lo:lo + 5], w, 255.0)
        assert all(torch.equal(p, f[lo:lo + 5]) for p, f in zip(part, (ssim, sse, counts))), lo
        want = R.pair_ssim(a[lo:lo + 5].cpu().numpy(), b[lo:lo + 5].cpu().numpy(), w, 255.0)[0]
        assert float(np.abs(part[0].cpu().numpy() - want).max()) <= SSIM_TOL
    w2 = torch.from_numpy(np.outer(w, w).reshape(9)).to(DEV)
    x, y = a.view(n, 9).double(), b.view(n, 9).double()
    ma, mb = x @ w2, y @ w2
    va, vb, cov = (x * x) @ w2 - ma * ma, (y * y) @ w2 - mb * mb, (x * y) @ w2 - ma * mb
    c1, c2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    want = (2 * ma * mb + c1) * (2 * cov + c2) / ((ma * ma + mb * mb + c1) * (va + vb + c2))
    err = float((ssim.view(n) - want).abs().max())
    print(f"ssim over {n} planes in two launches: max abs err {err:.3e}")
    assert err <= SSIM_TOL


def test_pair_ssim_refusals(ops):
    a = torch.zeros(2, 12, 13, 3, dtype=torch.uint8, device=DEV)
    w = _window("gauss3")
    before = ops._lib.N_CALLS
    for args in ((a, a[:1], w, 255.0), (a, a.float(), w, 255.0), (a, a, w, 1.0), (a, a, w, 0.0), (a[0], a[0], w, 255.0),
                 (a, a, _window("gauss15"), 255.0), (a, a, torch.from_numpy(w).to(DEV), 255.0), (a.int(), a.int(), w, 255.0),
                 (a.float(), a.float(), w, float("nan"))):
        with pytest.raises(ValueError):
            ops.pair_ssim(*args)
    for region in (torch.zeros(3, 12, 13, dtype=torch.uint8, device=DEV), torch.zeros(2, 12, 13, device=DEV),
                   torch.zeros(2, 13, 12, dtype=torch.uint8, device=DEV), torch.zeros(2, 12, 13, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ops.pair_ssim(a, a, w, 255.0, region)
    assert ops._lib.N_CALLS == before, "a refused call reached the library"


# ------------------------------------------------------------------------------------------------ the feature distance
FD_SHAPES = [(1, 1, 1), (2, 4, 3), (3, 64, 128), (2, 256, 192), (1, 1024, 768)]      # (B, HW, C)


@functools.lru_cache(maxsize=None)
def _maps(shape):
    B, HW, C = shape
    rng = np.random.default_rng(HW + C)
    side = int(round(HW ** 0.5))
    H, W = (side, side) if side * side == HW else (HW, 1)
    a = rng.standard_normal((B, H, W, C)).astype(np.float32)
    b = (a + 0.3 * rng.standard_normal((B, H, W, C))).astype(np.float32)
    if C == 1:
        # one channel: a unit "vector" is its sign, so the distance is 4 (opposite signs) or the rounding residue of
        # 1/(1 + 1e-10/|a|) - 1/(1 + 1e-10/|b|), about 1e-20, which no relative tolerance describes: take the opposite signs
        b = -np.abs(b) * np.sign(a)
    return a, b


@pytest.mark.parametrize("shape", FD_SHAPES, ids=str)
def test_feature_distance_against_reference(ops, shape):
    a, b = _maps(shape)
    want = R.feature_distance(a, b)
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = ops.f32_pair_feature_distance(ad, bd)
    assert got.dtype == torch.float64 and tuple(got.shape) == (shape[0],)
    err = float((np.abs(got.cpu().numpy() - want) / want).max())
    print(f"feature distance {shape}: max rel err {err:.3e} (values {want.min():.4f} .. {want.max():.4f})")
    assert err <= FD_RTOL
    zero = ops.f32_pair_feature_distance(ad, ad.clone())
    assert torch.equal(zero.cpu(), torch.zeros(shape[0], dtype=torch.float64)), "identical inputs give exactly 0.0"


def test_feature_distance_zero_pixel_and_placement(ops):
    a, b = (torch.from_numpy(x.copy()).to(DEV) for x in _maps((3, 64, 128)))
    a[0, 2, 3] = 0.0
    b[1, 0, 0] = 0.0
    a[2, 5, 5] = 0.0
    b[2, 5, 5] = 0.0
    alone = ops.f32_pair_feature_distance(a, b)
    want = R.feature_distance(a.cpu().numpy(), b.cpu().numpy())
    assert bool(torch.isfinite(alone).all()) and float((np.abs(alone.cpu().numpy() - want) / want).max()) <= FD_RTOL
    canary = -777.25
    out = torch.full((3, 3), canary, dtype=torch.float64, device=DEV)
    assert ops.f32_pair_feature_distance(a, b, out, 1) is out
    assert torch.equal(out[:, 1], alone) and bool((out[:, 0] == canary).all()) and bool((out[:, 2] == canary).all())
    before = ops._lib.N_CALLS
    for kw in (dict(out=out, column=3), dict(out=out, column=-1), dict(out=out.float(), column=0), dict(out=out[:2], column=0),
               dict(out=None, column=1), dict(out=out.cpu(), column=0), dict(out=out.t().contiguous().t(), column=0)):
        with pytest.raises(ValueError):
            ops.f32_pair_feature_distance(a, b, **kw)
    wide = torch.zeros(1, 1, 1, 769, device=DEV)
    for x, y in ((a, b[:2]), (a.double(), b.double()), (a.cpu(), b.cpu()), (a[0], b[0]), (wide, wide), (a[:, :, :, ::2], b[:, :, :, ::2])):
        with pytest.raises(ValueError):
            ops.f32_pair_feature_distance(x, y)
    assert ops._lib.N_CALLS == before, "a refused call reached the library"


# ------------------------------------------------------------------------------------------------ invariance, bit for bit
def _offset_view(x):
    """the same values in a tensor whose storage starts one element later (4-byte aligned only)"""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    buf[1:] = x.flatten()
    v = buf[1:].view(x.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_ssim_rows_do_not_depend_on_the_batch(ops, kind):
    shape = (5, 32, 32, 3) if kind == "u8" else (1, 37, 70, 3)
    a, b = _pair_u8(shape)
    if kind == "u8":
        a, b, L = np.concatenate([a, a[:1]]), np.concatenate([b, b[:1]]), 255.0
    else:
        a, b, L = _as_f32(np.concatenate([a] * 3)), _as_f32(np.concatenate([b, a, b])), 1.0
    n = a.shape[0]
    H, W = (a.shape[1], a.shape[2]) if kind == "u8" else (a.shape[2], a.shape[3])
    region = torch.from_numpy(_regions(n, H, W)["irregular"]).to(DEV)
    ad, bd, w = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), _window("gauss11")
    for reg in (None, region):
        full = ops.pair_ssim(ad, bd, w, L, reg)
        for i in range(n):
            one = ops.pair_ssim(ad[i:i + 1], bd[i:i + 1], w, L, None if reg is None else reg[i:i + 1])
            assert all(torch.equal(o[0], f[i]) for o, f in zip(one, full)), (kind, i)
        rev = ops.pair_ssim(ad.flip(0).contiguous(), bd.flip(0).contiguous(), w, L, None if reg is None else reg.flip(0).contiguous())
        assert all(torch.equal(r.flip(0), f) for r, f in zip(rev, full)), "a row's place in the batch"
    if kind == "f32":
        full = ops.pair_ssim(ad, bd, w, L)
        moved = ops.pair_ssim(_offset_view(ad), _offset_view(bd), w, L)
        assert all(torch.equal(m, f) for m, f in zip(moved, full)), "an unaligned view"
        # the same pixels through other strides: NHWC storage viewed as NCHW
        strided = ops.pair_ssim(ad.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2),
                                bd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), w, L)
        assert all(torch.equal(s, f) for s, f in zip(strided, full)), "the strides"


@pytest.mark.parametrize("shape", [(3, 64, 128), (2, 256, 192), (2, 4, 3)], ids=str)
def test_feature_distance_rows_do_not_depend_on_the_batch(ops, shape):
    a, b = (torch.from_numpy(x).to(DEV) for x in _maps(shape))
    full = ops.f32_pair_feature_distance(a, b)
    for i in range(shape[0]):
        assert torch.equal(ops.f32_pair_feature_distance(a[i:i + 1], b[i:i + 1])[0], full[i]), i
    assert torch.equal(ops.f32_pair_feature_distance(a.flip(0).contiguous(), b.flip(0).contiguous()).flip(0), full)
    # 16-byte loads against element loads: an unaligned view of either operand, and of both
    for x, y in ((_offset_view(a), b), (a, _offset_view(b)), (_offset_view(a), _offset_view(b))):
        assert torch.equal(ops.f32_pair_feature_distance(x, y), full), "the load path"


# ------------------------------------------------------------------------------------------------ end to end
def _model(P, ecfg, dcfg):
    import tinyedm_amd as T
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), dcfg.dropout_rate,
                     dcfg.sigma_data, dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    emb.load_state_dict({k[len("embedding."):]: v for k, v in P.items() if k.startswith("embedding.")})
    den.load_state_dict({k[len("denoiser."):]: v for k, v in P.items() if k.startswith("denoiser.")})
    den.set_eval_dtype("f32x3")
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                  steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01)
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def small():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ecfg, dcfg = tiny_cfgs(num_classes=3)
    P = O.init_params(ecfg, dcfg, torch.Generator().manual_seed(5), gains_nonzero=True)
    return _model(P, ecfg, dcfg), int(dcfg.in_channels)


def _images(n, C, size, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, size, size, C), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
    return a, b


def _maps_by_hand(ops, model, u8_nhwc, ids, taps, sigma, seed):
    """the extractor's steps written out: normalise, noise with (seed, id), run to the taps"""
    from tinyedm_amd.callbacks import _eval_dtype
    u8 = torch.from_numpy(u8_nhwc).to(DEV).permute(0, 3, 1, 2).contiguous()
    n = u8.shape[0]
    clean = ops.u8_gather_normalize(u8, torch.arange(n, device=DEV), 0.5, 0.5)
    ids_dev = torch.from_numpy(np.asarray(ids, dtype=np.uint32)).to(DEV)
    with torch.no_grad(), _eval_dtype(model, "f32x3"):
        noisy, sig = ops.eval_diffuse(clean, ids_dev, torch.zeros(n, dtype=torch.int32, device=DEV),
                                      torch.tensor([sigma], dtype=torch.float32, device=DEV), ops.churn_record(seed, 0, DEV),
                                      check_levels=False)
        return model.forward_taps(noisy, sig, None, taps)


def test_paired_quality_end_to_end(ops, small):
    from tinyedm_amd import compare
    model, C = small
    n, size, taps, ids = 5, 16, ("enc1", "mid"), [7, 3, 11, 0, 5]
    a, b = _images(n, C, size, 1)
    region = _regions(n, size, size)["box"]
    pq = compare.PairedQuality(model, taps=taps, seed=9, sigma=0.2, batch_size=n)
    got = pq.score(a, b, region=region, ids=ids)
    w = compare.gaussian_window(11, 1.5)
    want_ssim, want_sse, want_counts = R.pair_ssim(a, b, w, 255.0, region)
    assert torch.equal(got["counts"].cpu(), torch.from_numpy(want_counts))
    npix = want_counts[:, 0].astype(np.float64) * C
    assert torch.equal(got["mse"].cpu(), torch.from_numpy(want_sse.sum(axis=1) / npix))
    assert np.allclose(got["psnr"].cpu().numpy(), R.psnr(want_sse.sum(axis=1), npix, 255.0), rtol=1e-14, atol=0)
    assert float(np.abs(got["ssim_channels"].cpu().numpy() - want_ssim).max()) <= SSIM_TOL
    assert float(np.abs(got["ssim"].cpu().numpy() - want_ssim.mean(axis=1)).max()) <= SSIM_TOL
    ma, mb = (_maps_by_hand(ops, model, x, ids, taps, 0.2, 9) for x in (a, b))
    want_fd = np.stack([R.feature_distance(ma[t].cpu().numpy(), mb[t].cpu().numpy()) for t in taps], axis=1)
    got_fd = got["perceptual_taps"].cpu().numpy()
    assert got_fd.shape == (n, 2) and float((np.abs(got_fd - want_fd) / want_fd).max()) <= FD_RTOL
    assert np.allclose(got["perceptual"].cpu().numpy(), want_fd.mean(axis=1), rtol=1e-9, atol=0)
    s = got["summary"]
    assert set(s) == {"mse", "psnr", "ssim", "perceptual"} and s["ssim"]["worst"] == int(got["ssim"].argmin())
    assert s["perceptual"]["worst"] == int(got["perceptual"].argmax()) and s["psnr"]["min"] == float(got["psnr"].min())
    # batch_size changes no bit
    for bs in (1, 3):
        other = compare.PairedQuality(model, taps=taps, seed=9, sigma=0.2, batch_size=bs).score(a, b, region=region, ids=ids)
        for k in ("mse", "psnr", "ssim", "ssim_channels", "perceptual", "perceptual_taps", "counts"):
            assert torch.equal(other[k], got[k]), (bs, k)
    # a set against itself
    same = pq.score(a, a.copy(), ids=ids)
    assert torch.equal(same["perceptual_taps"].cpu(), torch.zeros(n, 2, dtype=torch.float64))
    assert not bool(same["mse"].any()) and float((same["ssim"] - 1.0).abs().max()) <= SSIM_TOL
    assert torch.equal(same["psnr"].cpu(), torch.full((n,), 120.0, dtype=torch.float64))
    # float32 images in network range go through the writer's map: the same pixels, up to the rounding of x / 2 + 1 / 2
    fa, fb = (((torch.from_numpy(x).to(DEV).permute(0, 3, 1, 2).float() / 255.0) - 0.5) / 0.5 for x in (a, b))
    fl = compare.PairedQuality(None).score(fa, fb, region=region)
    assert "perceptual" not in fl and float((fl["ssim"] - got["ssim"]).abs().max()) < 1e-5
    assert np.allclose((fl["mse"] * 255.0 ** 2).cpu().numpy(), got["mse"].cpu().numpy(), rtol=1e-5)
    with pytest.raises(ValueError, match="mixed dtypes"):
        pq.score(a, fb)
    with pytest.raises(ValueError, match="counts no valid window centre"):
        pq.score(a, b, region=np.zeros((1, size, size), np.uint8))
    assert model.denoiser.eval_dtype == "f32x3" and not model.training


def test_extract_keeps_its_bits(ops, small):
    """FeatureExtractor.extract through tapped_maps against the pooled path written out on the same maps"""
    from tinyedm_amd.features import FeatureExtractor
    model, C = small
    n, taps, ids = 5, ("enc1", "mid"), [7, 3, 11, 0, 5]
    a, _ = _images(n, C, 16, 2)
    ex = FeatureExtractor(model, sigma=0.2, taps=taps, seed=9, batch_size=2)
    got = ex.extract(a, ids=ids)
    maps = _maps_by_hand(ops, model, a, ids, taps, 0.2, 9)
    want = torch.cat([ops.f32_pool_features(maps[t]) for t in taps], dim=1)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, ex.dim) and torch.equal(got, want)
    seen = [(lo, hi, tuple(m[0])) for lo, hi, m in ex.tapped_maps(a, ids=ids)]
    assert seen == [(0, 2, taps), (2, 4, taps), (4, 5, taps)]
    two = list(ex.tapped_maps(a, a.copy(), ids=ids))
    assert all(len(m) == 2 and all(torch.equal(m[0][t], m[1][t]) for t in taps) for _, _, m in two)
    # between two batches, and when the generator is abandoned, the model and the grad mode are the caller's
    gen = FeatureExtractor(model, sigma=0.2, taps=taps, seed=9, batch_size=2, network_dtype="f32").tapped_maps(a, ids=ids)
    model.train()
    try:
        lo, hi, (m,) = next(gen)
        assert (lo, hi) == (0, 2) and tuple(m["mid"].shape) == tuple(maps["mid"][:2].shape)
        assert float((m["mid"] - maps["mid"][:2]).norm() / maps["mid"][:2].norm()) < 1e-3      # (f32 against f32x3)
        assert torch.is_grad_enabled() and model.training and model.denoiser.eval_dtype == "f32x3"
        del gen
        assert torch.is_grad_enabled() and model.training and model.denoiser.eval_dtype == "f32x3"
    finally:
        model.eval()
    with pytest.raises(ValueError, match="image sets differ"):
        list(ex.tapped_maps(a[:3], a[:2]))
    assert model.denoiser.eval_dtype == "f32x3" and not model.training


# ------------------------------------------------------------------------------------------------ the command lines
def _write_pngs(path, images):
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    for i, a in enumerate(images):
        Image.fromarray(a if a.shape[2] == 3 else a[:, :, 0]).save(os.path.join(path, f"{i}.png"))


def test_compare_cli(ops, tmp_path):
    from tinyedm_amd import compare
    a, b = _images(4, 3, 16, 3)
    _write_pngs(str(tmp_path / "a"), a)
    _write_pngs(str(tmp_path / "b"), b)
    rep_path = str(tmp_path / "q.json")
    compare.main(["--image_dir", str(tmp_path / "a"), "--ref_image_dir", str(tmp_path / "b"), "--report", rep_path,
                  "--region_box", "2", "3", "14", "12", "--worst", "2"])
    rep = json.load(open(rep_path))
    assert set(rep) == {"settings", "summary", "images", "worst"} and set(rep["summary"]) == {"mse", "psnr", "ssim"}
    assert rep["settings"]["num_images"] == 4 and rep["settings"]["win_size"] == 11 and rep["settings"]["region_box"] == [2, 3, 14, 12]
    assert [r["index"] for r in rep["images"]] == [0, 1, 2, 3] and all(len(v) == 2 for v in rep["worst"].values())
    assert all(set(r) == {"index", "mse", "psnr", "ssim", "ssim_channels"} for r in rep["images"])
    region = compare.region_from_box((2, 3, 14, 12), 16, 16, 11)
    want_ssim, want_sse, want_counts = R.pair_ssim(a, b, compare.gaussian_window(11, 1.5), 255.0, region)
    assert np.abs(np.array([r["ssim"] for r in rep["images"]]) - want_ssim.mean(axis=1)).max() <= SSIM_TOL
    assert [r["mse"] for r in rep["images"]] == (want_sse.sum(axis=1) / (want_counts[:, 0] * 3.0)).tolist()
    assert rep["worst"]["ssim"][0] == int(want_ssim.mean(axis=1).argmin())
    with pytest.raises(ValueError, match="no valid centre"):
        compare.main(["--image_dir", str(tmp_path / "a"), "--ref_image_dir", str(tmp_path / "b"), "--report", rep_path,
                      "--region_box", "0", "0", "16", "4"])


def _generate(model, out, init, size, **kw):
    from tinyedm_amd import generate as G
    G.generate(None, False, str(out), 4, size, 3, 4, num_workers=0, num_steps=4, model=model, graph=False,
               init_dir=str(init), **kw)


def test_generate_quality_report(ops, small, tmp_path):
    model, C = small
    size = 16
    a, _ = _images(4, C, size, 4)
    _write_pngs(str(tmp_path / "init"), a)
    q = str(tmp_path / "q.json")
    _generate(model, tmp_path / "inp", tmp_path / "init", size, mask_box=(4, 4, 12, 12), quality_report=q,
              quality_perceptual=True)
    rep = json.load(open(q))
    assert set(rep) == {"settings", "restored"} and rep["settings"]["num_images"] == 4 and rep["settings"]["win_size"] == 11
    assert rep["settings"]["region_box"] == [4, 4, 12, 12] and rep["settings"]["perceptual"] is True
    assert set(rep["restored"]["summary"]) == {"mse", "psnr", "ssim", "perceptual"} and len(rep["restored"]["images"]) == 4
    assert all(np.isfinite([r["ssim"], r["psnr"], r["perceptual"]]).all() and r["perceptual"] > 0 for r in rep["restored"]["images"])
    # restoration: the outputs and A+ y; --restore_report is byte-identical to a run without the new flag
    r0, r1 = str(tmp_path / "r0.json"), str(tmp_path / "r1.json")
    _generate(model, tmp_path / "sr0", tmp_path / "init", size, restore_scale=2, restore_report=r0)
    _generate(model, tmp_path / "sr1", tmp_path / "init", size, restore_scale=2, restore_report=r1, quality_report=q)
    assert open(r0, "rb").read() == open(r1, "rb").read()
    rep = json.load(open(q))
    assert set(rep) == {"settings", "restored", "degraded"} and rep["settings"]["region_box"] is None
    for key in ("restored", "degraded"):
        assert set(rep[key]["summary"]) == {"mse", "psnr", "ssim"} and [r["index"] for r in rep[key]["images"]] == [0, 1, 2, 3]
    old = json.load(open(r0))
    assert abs(np.mean([r["psnr"] for r in rep["restored"]["images"]]) - old["psnr_restored"]) < 1e-3
    assert abs(np.mean([r["psnr"] for r in rep["degraded"]["images"]]) - old["psnr_degraded"]) < 1e-3
