"""Paired image quality without a GPU: the numpy reference against closed forms, the window tables, every refusal of
PairedQuality, `compare` and the new `generate` flags, the pairing of PNG indices, and the library surface."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import quality_ref as R
from tinyedm_amd import _lib, compare
from tinyedm_amd import generate as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------------ the window tables
@pytest.mark.parametrize("win,sigma", [(11, 1.5), (3, 0.5), (15, 2.0), (7, 1.0)])
def test_gaussian_window(win, sigma):
    w = compare.gaussian_window(win, sigma)
    assert w.dtype == np.float64 and w.shape == (win,)
    assert abs(w.sum() - 1.0) < 4e-16 and np.array_equal(w, w[::-1]) and w.argmax() == win // 2
    assert np.allclose(w, R.gaussian_taps(win, sigma), rtol=0, atol=1e-16)
    assert np.allclose(w[win // 2 + 1] / w[win // 2], np.exp(-1.0 / (2 * sigma * sigma)), rtol=1e-14)


@pytest.mark.parametrize("win", [3, 7, 15])
def test_uniform_window(win):
    w = compare.uniform_window(win)
    assert w.dtype == np.float64 and np.all(w == 1.0 / win) and abs(w.sum() - 1.0) < 4e-16


@pytest.mark.parametrize("bad", [2, 1, 17, 4, True, 11.0, None])
def test_window_refusals(bad):
    with pytest.raises(ValueError, match="win_size"):
        compare.gaussian_window(bad, 1.5)
    with pytest.raises(ValueError, match="win_size"):
        compare.uniform_window(bad)


def test_window_sigma_refusals():
    for s in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="sigma"):
            compare.gaussian_window(11, s)
    with pytest.raises(ValueError, match="window must be one of"):
        compare.make_window("box", 11, 1.5)
    assert [compare.default_win_size(s) for s in (3, 4, 8, 10, 11, 16, 32)] == [3, 3, 7, 9, 11, 11, 11]


# ------------------------------------------------------------------------------------------------ the reference: closed forms
@pytest.mark.parametrize("w", [compare.gaussian_window(11, 1.5), compare.uniform_window(7), compare.gaussian_window(3, 1.0)])
def test_reference_constant_images(w):
    p, q, L = 37.0, 201.0, 255.0
    a, b = np.full((1, 1, 16, 18), p), np.full((1, 1, 16, 18), q)
    c1 = (0.01 * L) ** 2
    S = R.ssim_map(a, b, w, L)
    assert S.shape == (1, 1, 16 - len(w) + 1, 18 - len(w) + 1)
    # (the variances of a constant are rounding residue of size 1e-16 L^2 against C2 = 9e-4 L^2)
    assert np.abs(S - (2 * p * q + c1) / (p * p + q * q + c1)).max() < 1e-12


def test_reference_identical_images():
    a = _rng(0).integers(0, 256, (2, 13, 17, 3), dtype=np.uint8)
    s, sse, counts = R.pair_ssim(a, a.copy(), compare.gaussian_window(11, 1.5), 255.0)
    assert np.abs(s - 1.0).max() < 1e-12 and not sse.any() and (counts == (13 * 17, 3 * 7)).all()
    assert R.psnr(0.0, 13 * 17 * 3, 255.0) == 120.0
    assert float(compare.psnr_from_sse(0.0, 13 * 17 * 3, 255.0)) == 120.0


def test_reference_single_window_by_hand():
    rng = _rng(1)
    win, L = 7, 255.0
    w = compare.gaussian_window(win, 1.5)
    a, b = rng.integers(0, 256, (win, win)).astype(np.float64), rng.integers(0, 256, (win, win)).astype(np.float64)
    w2 = np.outer(w, w)
    ma, mb = (w2 * a).sum(), (w2 * b).sum()
    va, vb, cov = (w2 * a * a).sum() - ma * ma, (w2 * b * b).sum() - mb * mb, (w2 * a * b).sum() - ma * mb
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    want = (2 * ma * mb + c1) * (2 * cov + c2) / ((ma * ma + mb * mb + c1) * (va + vb + c2))
    S = R.ssim_map(a[None, None], b[None, None], w, L)
    assert S.shape == (1, 1, 1, 1) and abs(S[0, 0, 0, 0] - want) < 1e-12


@pytest.mark.parametrize("win", [3, 11, 15])
def test_reference_separable_against_2d(win):
    rng = _rng(2)
    w = compare.gaussian_window(win, 1.5)
    a = rng.integers(0, 256, (2, 3, 19, 23)).astype(np.float64)
    b = np.clip(a + rng.normal(0, 20, a.shape), 0, 255).round()
    assert np.abs(R.ssim_map(a, b, w, 255.0) - R.ssim_map(a, b, w, 255.0, R.filter_valid_2d)).max() < 1e-12


def test_reference_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = _rng(3)
    win, L = 11, 1.0
    w = compare.gaussian_window(win, 1.5)
    a = rng.random((2, 20, 21))
    b = np.clip(a + rng.normal(0, 0.1, a.shape), 0, 1)
    half = win // 2

    def filt(x, _w):
        y = ndi.correlate1d(ndi.correlate1d(x, w, axis=-1, mode="constant"), w, axis=-2, mode="constant")
        return y[..., half:-half, half:-half]
    assert np.abs(R.ssim_map(a, b, w, L) - R.ssim_map(a, b, w, L, filt)).max() < 1e-12


def test_reference_region_rules():
    rng = _rng(4)
    a = rng.integers(0, 256, (2, 12, 13, 2), dtype=np.uint8)
    b = rng.integers(0, 256, (2, 12, 13, 2), dtype=np.uint8)
    w = compare.uniform_window(3)
    region = np.zeros((1, 12, 13), dtype=np.uint8)
    region[0, 0:5, 0:4] = 1                     # rows 0 and column 0 are not valid centres
    s, sse, counts = R.pair_ssim(a, b, w, 255.0, region)
    assert (counts == (20, 12)).all()
    d = a[:, 0:5, 0:4].astype(np.int64) - b[:, 0:5, 0:4].astype(np.int64)
    assert np.array_equal(sse, (d * d).sum(axis=(1, 2)).astype(np.float64))
    full = R.ssim_map(R.to_nchw(a), R.to_nchw(b), w, 255.0)
    assert np.abs(s - full[:, :, 0:4, 0:3].mean(axis=(2, 3))).max() < 1e-13
    region[:] = 0
    region[0, 0, :] = 1                         # counted pixels, no counted centre
    s, sse, counts = R.pair_ssim(a, b, w, 255.0, region)
    assert np.isnan(s).all() and (counts == (13, 0)).all()


def test_reference_feature_distance():
    rng = _rng(5)
    a = rng.normal(size=(2, 6, 5)).astype(np.float32)
    assert np.array_equal(R.feature_distance(a, a.copy()), np.zeros(2))
    b = (3.0 * a).astype(np.float32)            # the same directions: distance ~ 0, far below 2 - 2 cos's cancellation
    assert R.feature_distance(a, b).max() < 1e-13
    assert np.allclose(R.feature_distance(a, -a), 4.0, rtol=1e-9)         # opposite unit vectors: |2 u|^2 = 4 per pixel
    z = a.copy()
    z[0, 2] = 0.0
    d = R.feature_distance(a, z)
    assert np.isfinite(d).all() and abs(d[0] - 1.0 / 6.0) < 1e-9 and d[1] == 0.0


def test_psnr_floor_and_values():
    assert float(compare.psnr_from_sse(255.0 ** 2 * 10, 10, 255.0)) == 0.0
    sse = torch.tensor([0.0, 12.0, 3.0e5], dtype=torch.float64)
    assert np.allclose(compare.psnr_from_sse(sse, 3072, 255.0).numpy(), R.psnr(sse.numpy(), 3072, 255.0), rtol=1e-15)
    assert float(compare.psnr_from_sse(1e-9, 3072, 1.0)) == 120.0


def test_summary_and_worst():
    v = torch.tensor([3.0, 1.0, 2.0, 1.0], dtype=torch.float64)
    s = compare.summarize(v)
    assert s["mean"] == 1.75 and s["min"] == 1.0 and s["max"] == 3.0 and abs(s["std"] - np.std([3, 1, 2, 1])) < 1e-15
    assert compare.worst_indices(v, "ssim", 3) == [1, 3, 2] and compare.worst_indices(v, "psnr", 1) == [1]
    assert compare.worst_indices(v, "mse", 2) == [0, 2] and compare.worst_indices(v, "perceptual", 9) == [0, 2, 1, 3]


# ------------------------------------------------------------------------------------------------ refusals
def test_paired_quality_refusals():
    PQ = compare.PairedQuality
    for kw, match in (({"win_size": 4}, "win_size"), ({"win_size": 17}, "win_size"), ({"window": "box"}, "window"),
                      ({"win_sigma": 0.0}, "sigma"), ({"sigma": -1.0}, "sigma"), ({"network_dtype": "bf16"}, "network_dtype"),
                      ({"conditional": True}, "needs a model"), ({"std": (0.0,)}, "std"),
                      ({"mean": (float("nan"),)}, "mean")):
        with pytest.raises(ValueError, match=match):
            PQ(**kw)
    with pytest.raises(ValueError, match="EDM"):
        PQ(model=object())
    pq = PQ(win_size=3)
    u8 = np.zeros((2, 8, 8, 3), np.uint8)
    f32 = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="mixed dtypes"):
        pq._pair(u8, f32)
    with pytest.raises(ValueError, match="differ in shape"):
        pq._pair(u8, u8[:1])
    with pytest.raises(ValueError, match="must be non-empty"):
        pq._pair(u8.astype(np.int32), u8.astype(np.int32))
    with pytest.raises(ValueError, match="must be non-empty"):
        pq._pair(u8[0], u8[0])
    with pytest.raises(ValueError, match="on one GPU"):
        pq._pair(f32, f32)
    with pytest.raises(ValueError, match="region must be"):
        pq._region(np.zeros((3, 8, 8), np.uint8), 2, 8, 8, torch.device("cpu"))
    with pytest.raises(ValueError, match="region must be"):
        pq._region(np.zeros((2, 8, 8), np.float32), 2, 8, 8, torch.device("cpu"))
    edge = np.zeros((1, 8, 8), np.uint8)
    edge[0, 0, :] = 1
    with pytest.raises(ValueError, match="counts no valid window centre"):
        pq._region(edge, 2, 8, 8, torch.device("cpu"))
    assert pq._region(np.ones((1, 8, 8), np.uint8), 2, 8, 8, torch.device("cpu")).dtype == torch.uint8


def test_region_box():
    r = compare.region_from_box((2, 1, 6, 4), 8, 10, 3)
    assert r.shape == (1, 8, 10) and r.dtype == np.uint8 and r.sum() == 12 and r[0, 1:4, 2:6].all()
    for box in ((0, 0, 11, 4), (4, 4, 4, 6), (-1, 0, 3, 3), (0, 0, 3), (0.5, 0, 3, 3)):
        with pytest.raises(ValueError, match="X0 Y0 X1 Y1"):
            compare.region_from_box(box, 8, 10, 3)
    with pytest.raises(ValueError, match="no valid centre"):
        compare.region_from_box((0, 0, 5, 8), 8, 10, 11)       # 11 taps do not fit 8 rows at all
    with pytest.raises(ValueError, match="no valid centre"):
        compare.region_from_box((0, 0, 10, 1), 8, 10, 3)       # the top row only
    with pytest.raises(ValueError, match="no valid centre"):
        compare.region_from_box((9, 2, 10, 6), 8, 10, 3)       # the last column only


def _args(*extra):
    return compare.build_parser().parse_args(["--image_dir", "a", "--ref_image_dir", "b", "--report", "r.json", *extra])


def test_compare_check_args():
    compare.check_args(_args())
    compare.check_args(_args("--ckpt_path", "c.ckpt", "--load_ema", "--sigma", "0.2", "--taps", "mid", "enc1", "--seed", "3",
                             "--network_dtype", "f32", "--region_box", "1", "1", "5", "5", "--window", "uniform",
                             "--win_size", "7", "--worst", "3"))
    for extra, match in ((("--win_size", "4"), "win_size"), (("--win_size", "17"), "win_size"), (("--window", "box"), "window"),
                         (("--win_sigma", "0"), "sigma"), (("--sigma", "0.1"), "needs --ckpt_path"),
                         (("--taps", "mid"), "needs --ckpt_path"), (("--seed", "1"), "needs --ckpt_path"),
                         (("--network_dtype", "f32"), "needs --ckpt_path"), (("--load_ema",), "needs --ckpt_path"),
                         (("--ckpt_path", "c", "--network_dtype", "bf16"), "network_dtype"),
                         (("--ckpt_path", "c", "--sigma", "-1"), "sigma"), (("--ckpt_path", "c", "--seed", "-1"), "seed"),
                         (("--ckpt_path", "c", "--taps", "mid", "mid"), "twice"), (("--batch_size", "0"), "batch_size"),
                         (("--worst", "0"), "worst"), (("--region_box", "5", "1", "1", "5"), "region_box"),
                         (("--region_box", "-1", "1", "3", "5"), "region_box")):
        with pytest.raises(ValueError, match=match):
            compare.check_args(_args(*extra))
    same = compare.build_parser().parse_args(["--image_dir", "a", "--ref_image_dir", "./a", "--report", "r.json"])
    with pytest.raises(ValueError, match="same directory"):
        compare.check_args(same)
    with pytest.raises(SystemExit):
        compare.main(["--image_dir", "a", "--ref_image_dir", "b", "--report", "r.json", "--win_size", "4"])


def _generate_options(**kw):
    defaults = {k: p.default for k, p in inspect.signature(G.generate).parameters.items()}
    base = {k: defaults.get(k, False) for k in inspect.signature(G._validate).parameters}
    return {**base, "init_dir": "d", "image_size": 32, "num_steps": 8, **kw}


def test_generate_quality_flags():
    V = G._validate
    assert {"quality_report", "quality_perceptual"} <= set(inspect.signature(G.generate).parameters)
    for ok in ({"mask_box": (8, 8, 24, 24)}, {"restore_scale": 4}, {"restore_gray": True}, {"start_step": 3},
               {"dps_scale": 1.0, "blur_std": 1.0, "network_dtype": "bf16"},
               {"restore_scale": 2, "restore_report": "r.json", "quality_perceptual": True},
               {"mask_box": (0, 0, 8, 8), "image_size": 8}):
        V(**_generate_options(quality_report="q.json", **ok))
    for bad, match in (({"init_dir": None}, "needs --init_dir"), ({}, "keeps a ground truth"),
                       ({"invert_to": "o.pt"}, "--invert_to"), ({"likelihood_to": "o.json"}, "--likelihood_to"),
                       ({"mask_box": (0, 0, 32, 4)}, "no valid centre"), ({"mask_box": (28, 8, 32, 24)}, "no valid centre")):
        with pytest.raises(ValueError, match=match):
            V(**_generate_options(quality_report="q.json", **bad))
    with pytest.raises(ValueError, match="--quality_perceptual adds a column"):
        V(**_generate_options(quality_perceptual=True, restore_scale=4))
    assert V(**_generate_options(restore_scale=4)) == (False, True), "without the flags nothing changes"


# ------------------------------------------------------------------------------------------------ pairing of PNG indices
def _write_pngs(path, indices, seed, size=(6, 5), channels=3):
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    rng = _rng(seed)
    out = {}
    for i in indices:
        a = rng.integers(0, 256, size + (channels,), dtype=np.uint8)
        Image.fromarray(a if channels == 3 else a[:, :, 0]).save(os.path.join(path, f"{i}.png"))
        out[i] = a
    return out


def test_read_pairs(tmp_path):
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    wa, wb = _write_pngs(a_dir, [10, 2, 0], 1), _write_pngs(b_dir, [0, 2, 10], 2)
    idx, a, b = compare.read_pairs(a_dir, b_dir)
    assert idx == [0, 2, 10] and a.shape == b.shape == (3, 6, 5, 3) and a.dtype == np.uint8
    assert all(np.array_equal(a[k], wa[i]) and np.array_equal(b[k], wb[i]) for k, i in enumerate(idx)), "numeric order"
    _write_pngs(a_dir, [7], 3)
    with pytest.raises(ValueError, match=r"7\.png is in --image_dir but missing from --ref_image_dir"):
        compare.read_pairs(a_dir, b_dir)
    _write_pngs(b_dir, [7, 4], 4)
    with pytest.raises(ValueError, match=r"4\.png is in --ref_image_dir but missing from --image_dir"):
        compare.read_pairs(a_dir, b_dir)
    c_dir = str(tmp_path / "c")
    _write_pngs(c_dir, [0, 2, 4, 7, 10], 5, size=(6, 6))
    with pytest.raises(ValueError, match="expected uint8"):
        compare.read_pairs(b_dir, c_dir)
    open(os.path.join(c_dir, "x.png"), "wb").close()
    with pytest.raises(ValueError, match="not named <index>.png"):
        compare.read_pairs(c_dir, b_dir)
    os.makedirs(str(tmp_path / "empty"))
    with pytest.raises(ValueError, match="no PNG"):
        compare.read_pairs(str(tmp_path / "empty"), b_dir)


# ------------------------------------------------------------------------------------------------ the library surface
NEW = ("edm_pair_ssim_tiles", "edm_pair_ssim", "edm_f32_pair_feature_distance")


def test_header_binding_and_exports():
    with open(os.path.join(ROOT, "include", "tinyedm_hip.h")) as f:
        hdr = f.read()
    for name in NEW:
        m = re.search(r"\b(?:int|long) " + name + r"\(([^;]*?)\);", hdr, re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip() != "void"]) == len(_lib.SIGNATURES[name]), name
    assert "edm_pair_ssim_tiles" in _lib._NO_STATUS and _lib._RET["edm_pair_ssim_tiles"] is _lib.ctypes.c_long
    if os.path.exists(_lib.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
        assert set(NEW) <= set(re.findall(r"\bT (edm_[a-z0-9_]+)", nm.stdout))
        # host logic, no GPU needed: the tiling is a function of (H, W, win)
        tiles = lambda H, W, win: int(_lib.call("edm_pair_ssim_tiles", H, W, win))    # noqa: E731
        assert [tiles(32, 32, 11), tiles(64, 64, 11), tiles(37, 70, 3), tiles(11, 11, 11), tiles(26, 42, 11)] == [2, 8, 9, 1, 1]
        assert tiles(27, 43, 11) == 4 and tiles(8, 8, 11) == 0 and tiles(32, 32, 4) == 0 and tiles(32, 32, 17) == 0
    from tinyedm_amd import ops
    assert ops.SSIM_MAX_WIN == compare.MAX_WIN == 15 and ops.FEATURE_DISTANCE_MAX_C == 768
    import tinyedm
    import tinyedm.compare as shim
    assert tinyedm.PairedQuality is compare.PairedQuality and shim.main is compare.main
    assert shim.gaussian_window is compare.gaussian_window
    from tinyedm_amd.features import FeatureExtractor
    assert callable(FeatureExtractor.tapped_maps)


def test_ops_refusals_need_no_gpu():
    from tinyedm_amd import ops
    cpu = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.pair_ssim(cpu, cpu, compare.uniform_window(3), 255.0)
    for w, match in ((np.ones(4) / 4, "odd"), (np.ones(17) / 17, "odd"), (np.ones(3, np.float32), "fp64"),
                     (np.array([0.5, np.nan, 0.5]), "non-finite"), (np.ones((3, 3)), "1-d")):
        with pytest.raises(ValueError, match=match):
            ops._ssim_window(w)
    with pytest.raises(ValueError):
        ops.f32_pair_feature_distance(torch.zeros(1, 2, 2, 4), torch.zeros(1, 2, 2, 4))

