"""Loss by noise level on the GPU (tinyedm_amd/evaluate.py, ops.eval_diffuse / ops.eval_sqerr in sample_eval.hip):

 * the noise against the numpy restatement of tests/evaluate_ref.py on the dwordx4 path, the scalar path with a partial
   last quad and the scalar path of a misaligned tensor; clean + sigma*n on non-zero images; the noise of an (id, level,
   draw) does not depend on the batch, the row or the neighbours; other ids / levels / draws / seeds are uncorrelated;
 * the fp64 squared error against numpy, bit-identical across batch sizes and memory paths, exact zero, slice output;
 * the health bit and the refusals;
 * the evaluator on model-free known answers, against the CPU oracle (bf16 and "f32"), its uncertainty column, the CLI
   end to end and the LossByNoiseLevel callback."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate_ref as R
from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs
from parity_log import record

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x9E3779B97F4A7C15           # a non-zero high word
IDS = [5, 0, 1000003, 7, 4294967295, 2, 65536]
LEVELS = [0, 2, 1, 1, 0, 2, 2]
CASES = [((7, 3, 32, 32), 0), ((5, 3, 7, 9), 0), ((7, 3, 32, 32), 1)]
CASE_IDS = ["cifar-vec", "odd-scalar", "misaligned-scalar"]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _u32(v):
    return torch.from_numpy(np.asarray(v, dtype=np.uint32)).to(DEV)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _f32(v):
    return torch.tensor(list(v), dtype=torch.float32, device=DEV)


def _at(t, offset):
    """a contiguous copy of t that starts `offset` floats into a fresh allocation"""
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    assert (v.data_ptr() % 16 == 0) == (offset == 0) and v.is_contiguous()
    return v


def _noise(ops, shape, ids, levels, seed=SEED, draw=3, offset=0, L=3):
    """unit noise of the kernel: zeros in, every level at sigma = 1"""
    rec = ops.churn_record(seed, draw, DEV)
    x = _at(torch.zeros(shape, device=DEV), offset)
    n, s = ops.eval_diffuse(x, _u32(ids), _i32(levels), _f32([1.0] * L), rec)
    assert torch.equal(s, torch.ones(shape[0], device=DEV))
    return n


# ------------------------------------------------------------------ 1. the noise against the restatement
@pytest.mark.parametrize("shape,offset", CASES, ids=CASE_IDS)
def test_noise_vs_restatement(ops, shape, offset):
    B = shape[0]
    ids, levels = IDS[:B], LEVELS[:B]
    n = _noise(ops, shape, ids, levels, offset=offset)
    ops.check_health(DEV, "eval_diffuse")
    ref = R.eval_noise(shape, ids, levels, SEED, 3)
    err = float(np.abs(n.double().cpu().numpy() - ref).max())
    record(f"evaluate/noise_{'x'.join(map(str, shape))}_off{offset}_maxabs", err, 1e-5)
    print(f"noise {shape} offset {offset}: max abs {err:.3e}")
    assert err <= 1e-5, err          # the limit the churn's Box-Muller is held to; a wrong counter is O(1)
    if offset:                       # the scalar path of a misaligned tensor draws the dwordx4 path's bits
        assert torch.equal(n, _noise(ops, shape, ids, levels))


# ------------------------------------------------------------------ 2. the affine form
def test_affine_on_nonzero_images(ops):
    g = torch.Generator().manual_seed(1)
    clean = torch.randn(6, 3, 16, 16, generator=g).to(DEV)
    ids, levels = IDS[:6], LEVELS[:6]
    sig = _f32([0.002, 1.0, 80.0])
    rec = ops.churn_record(42, 0, DEV)
    n = _noise(ops, tuple(clean.shape), ids, levels, seed=42, draw=0)
    noisy, s = ops.eval_diffuse(clean, _u32(ids), _i32(levels), sig, rec)
    assert torch.equal(s, sig[torch.tensor(levels, device=DEV)])          # bit for bit
    ref = clean.double() + s.double().view(-1, 1, 1, 1) * n.double()
    e = rel(noisy, ref)
    worst = (noisy.double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"affine: rel {e:.3e}, max abs / max |ref| {worst:.3e}")
    assert e <= 1e-7                 # one fp32 fma
    assert worst <= 4e-7
    ops.check_health(DEV, "eval_diffuse affine")


# ------------------------------------------------------------------ 3. independence
def test_noise_belongs_to_the_image_not_the_row(ops):
    for shape in ((7, 3, 32, 32), (7, 3, 7, 9)):
        base = _noise(ops, shape, IDS, LEVELS)
        two = _noise(ops, (2,) + shape[1:], [IDS[4], IDS[1]], [LEVELS[4], LEVELS[1]])      # other batch, rows, neighbours
        assert torch.equal(two[0], base[4]) and torch.equal(two[1], base[1])
        rev = _noise(ops, shape, IDS[::-1], LEVELS[::-1])
        assert torch.equal(rev.flip(0), base)
        # the same id twice in one batch: the same noise twice
        twice = _noise(ops, (3,) + shape[1:], [IDS[2], 9, IDS[2]], [LEVELS[2], 0, LEVELS[2]])
        assert torch.equal(twice[0], base[2]) and torch.equal(twice[2], base[2]) and not torch.equal(twice[1], base[2])


def test_streams_uncorrelated(ops):
    shape = (1, 3, 128, 256)                    # 98 304 elements: corr / mean standard error 0.0032
    draws = {       # (id, level, draw, seed)
        "base": (5, 1, 0, 5), "id": (6, 1, 0, 5), "level": (5, 2, 0, 5), "draw": (5, 1, 1, 5), "seed": (5, 1, 0, 6),
        "seed_hi": (5, 1, 0, 5 + (1 << 32)),
    }
    ns = {k: _noise(ops, shape, [i], [l], seed=s, draw=d).double().flatten() for k, (i, l, d, s) in draws.items()}
    m = ns["base"].numel()
    assert m == 98304
    for k, v in ns.items():
        assert abs(v.mean().item()) < 5 / math.sqrt(m), k
        assert abs(v.std().item() - 1.0) < 5 / math.sqrt(2 * m), k
        if k != "base":
            corr = torch.corrcoef(torch.stack([ns["base"], v]))[0, 1].item()
            assert abs(corr) < 0.02, (k, corr)


# ------------------------------------------------------------------ 4. the squared error
@pytest.mark.parametrize("shape,offset", CASES, ids=CASE_IDS)
def test_sqerr_vs_numpy(ops, shape, offset):
    g = torch.Generator().manual_seed(2)
    D0, c0 = torch.randn(shape, generator=g), 0.5 * torch.randn(shape, generator=g)
    D, clean = _at(D0.to(DEV), offset), _at(c0.to(DEV), offset)
    se = ops.eval_sqerr(D, clean)
    ops.check_health(DEV, "eval_sqerr")
    assert se.dtype == torch.float64 and tuple(se.shape) == (shape[0],)
    d = D0.double().numpy() - c0.double().numpy()
    ref = (d * d).reshape(shape[0], -1).sum(axis=1)
    err = float(np.abs(se.cpu().numpy() - ref).max() / np.abs(ref).max())
    worst = float((np.abs(se.cpu().numpy() - ref) / ref).max())
    record(f"evaluate/sqerr_{'x'.join(map(str, shape))}_off{offset}_rel", worst, 1e-12)
    print(f"sqerr {shape} offset {offset}: rel {worst:.3e}")
    assert worst <= 1e-12 and err <= 1e-12
    # a sample's bits: the same in a batch of 2, at another row, on the other memory path
    two = ops.eval_sqerr(_at(D0[[4, 1]].to(DEV), offset), _at(c0[[4, 1]].to(DEV), offset))
    assert torch.equal(two, se[[4, 1]])
    if offset:
        assert torch.equal(se, ops.eval_sqerr(D0.to(DEV), c0.to(DEV)))
    assert torch.equal(ops.eval_sqerr(clean, clean), torch.zeros(shape[0], dtype=torch.float64, device=DEV))
    # into a slice of a larger buffer: the rest is untouched
    buf = torch.full((shape[0] + 13,), -7.0, dtype=torch.float64, device=DEV)
    out = ops.eval_sqerr(D, clean, out=buf[5:5 + shape[0]])
    assert out.data_ptr() == buf[5:].data_ptr() and torch.equal(buf[5:5 + shape[0]], se)
    assert bool((buf[:5] == -7.0).all()) and bool((buf[5 + shape[0]:] == -7.0).all())


# ------------------------------------------------------------------ 5. health and refusals
def test_nonfinite_sets_health(ops):
    rec = ops.churn_record(1, 0, DEV)
    ops.check_health(DEV, "before")
    for shape, where in (((7, 3, 32, 32), (3, 1, 5, 17)), ((5, 3, 7, 9), (4, 2, 6, 8))):     # vector body / scalar tail
        B = shape[0]
        x = torch.zeros(shape, device=DEV)
        x[where] = float("nan")
        noisy, _ = ops.eval_diffuse(x, _u32(IDS[:B]), _i32(LEVELS[:B]), _f32([1.0] * 3), rec)
        with pytest.raises(ops.GraphCorruptionError, match="non-finite"):
            ops.check_health(DEV, "eval_diffuse")
        ops.check_health(DEV, "cleared")
        ops.eval_sqerr(x, torch.zeros(shape, device=DEV))
        with pytest.raises(ops.GraphCorruptionError, match="non-finite"):
            ops.check_health(DEV, "eval_sqerr")
    ops.check_health(DEV, "after")


def test_refusals_before_launch(ops):
    from tinyedm_amd import _lib
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    ids, lev, sig = _u32([0, 1]), _i32([0, 1]), _f32([0.5, 1.0])
    rec = ops.churn_record(0, 0, DEV)
    ops.eval_diffuse(x, ids, lev, sig, rec)
    calls = _lib.N_CALLS
    bad = [
        lambda: ops.eval_diffuse(x, ids, _i32([0, 2]), sig, rec),                   # level == L
        lambda: ops.eval_diffuse(x, ids, _i32([-1, 0]), sig, rec),
        lambda: ops.eval_diffuse(x.double(), ids, lev, sig, rec),
        lambda: ops.eval_diffuse(x, ids.to(torch.int32), lev, sig, rec),
        lambda: ops.eval_diffuse(x, ids, lev.long(), sig, rec),
        lambda: ops.eval_diffuse(x, ids, lev, sig.double(), rec),
        lambda: ops.eval_diffuse(x.cpu(), ids, lev, sig, rec),
        lambda: ops.eval_diffuse(x, ids.cpu(), lev, sig, rec),
        lambda: ops.eval_diffuse(x, ids, lev, sig.cpu(), rec),
        lambda: ops.eval_diffuse(x, ids, lev, sig, rec.cpu()),
        lambda: ops.eval_diffuse(x.transpose(2, 3), ids, lev, sig, rec),
        lambda: ops.eval_diffuse(x, _u32([0, 1, 2]), lev, sig, rec),
        lambda: ops.eval_diffuse(x, ids, lev, sig.view(1, 2), rec),
        lambda: ops.eval_diffuse(x, ids, lev, torch.ones(65536, device=DEV), rec),
        lambda: ops.eval_diffuse(x, ids, lev, sig, rec[:3]),
        lambda: ops.eval_diffuse(torch.zeros(4, device=DEV), ids, lev, sig, rec),
        lambda: ops.eval_sqerr(x.double(), x),
        lambda: ops.eval_sqerr(x, x.cpu()),
        lambda: ops.eval_sqerr(x.transpose(2, 3), x),
        lambda: ops.eval_sqerr(x[:1], x),
        lambda: ops.eval_sqerr(x, x, out=torch.zeros(2, device=DEV)),
        lambda: ops.eval_sqerr(x, x, out=torch.zeros(3, dtype=torch.float64, device=DEV)),
        lambda: ops.eval_sqerr(x, x, out=torch.zeros(4, dtype=torch.float64, device=DEV)[::2]),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises((ValueError, _lib.HipKernelError)):
            fn()
        assert _lib.N_CALLS == calls, i          # nothing reached the library
    ops.check_health(DEV, "refusals")


# ------------------------------------------------------------------ 6. the evaluator, model-free known answers
@pytest.fixture(scope="module")
def images64():
    g = torch.Generator().manual_seed(5)
    return (0.5 * torch.randn(64, 3, 16, 16, generator=g)).to(DEV)


def _ev(**kw):
    from tinyedm_amd.evaluate import NoiseLevelEvaluator
    kw.setdefault("num_levels", 4)
    kw.setdefault("P_mean", -1.2)
    kw.setdefault("P_std", 1.2)
    return NoiseLevelEvaluator(**kw)


def test_evaluator_known_answers(ops, images64):
    def ident(x, s, l):
        return x
    N, chw = 64, 3 * 16 * 16
    for draws in (1, 2):
        res = _ev(num_draws=draws, batch_size=48).evaluate(ident, images64)
        assert res["count"] == [N] * 4 and res["expected_loss"] is not None and "uncertainty" not in res
        assert tuple(res["se"].shape) == (draws, 4, N)
        lim = 5 * math.sqrt(2.0 / (N * chw * draws))               # chi-square standard error
        for l, (s, mse) in enumerate(zip(res["sigma"], res["mse"])):
            print(f"identity model, draws {draws}, level {l}: mse / sigma^2 - 1 = {mse / s ** 2 - 1:+.3e} (limit {lim:.3e})")
            assert abs(mse / s ** 2 - 1.0) <= lim, (l, mse / s ** 2)
        want = sum((s * s + 0.25) / (s * 0.5) ** 2 * m for s, m in zip(res["sigma"], res["mse"])) / 4
        assert abs(res["expected_loss"] - want) <= 1e-12 * want
    ref = [float(np.float32(s)) for s in R.level_sigmas(-1.2, 1.2, 4)]
    assert res["sigma"] == ref
    # a model that returns the clean images: exactly zero (batch_size = N: a chunk is the images in id order)
    res0 = _ev(batch_size=64).evaluate(lambda x, s, l: images64, images64)
    assert res0["mse"] == [0.0] * 4 and res0["loss"] == [0.0] * 4 and not res0["se"].any()


def test_evaluator_independent_of_batch_size_and_order(ops, images64):
    def ident(x, s, l):
        return x * 0.75
    a = _ev(batch_size=48, seed=9).evaluate(ident, images64)
    b = _ev(batch_size=256, seed=9).evaluate(ident, images64)
    assert torch.equal(a["se"], b["se"])
    assert max(abs(x - y) / y for x, y in zip(a["mse"], b["mse"])) <= 1e-12
    # ids carry the noise: a permuted set with its ids gives the same matrix, default ids another one
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(1))
    c = _ev(batch_size=48, seed=9).evaluate(ident, images64[perm.to(DEV)].contiguous(), ids=perm)
    assert torch.equal(c["se"], a["se"]) and c["ids"] == list(range(64))
    # draws: the first of two is the one of one; two differ from one; the seed reproduces
    d1 = _ev(num_draws=2, seed=9).evaluate(ident, images64)
    d2 = _ev(num_draws=2, seed=9).evaluate(ident, images64)
    assert torch.equal(d1["se"], d2["se"]) and d1["mse"] == d2["mse"]
    assert torch.equal(d1["se"][0], a["se"][0]) and not torch.equal(d1["se"][1], a["se"][0])
    assert d1["mse"] != a["mse"]
    assert _ev(seed=10).evaluate(ident, images64)["mse"] != a["mse"]
    # explicit levels: no expected loss
    e = _ev(sigmas=[0.1, 1.0]).evaluate(ident, images64)
    assert e["expected_loss"] is None and e["sigma"] == [float(np.float32(0.1)), 1.0] and len(e["mse"]) == 2
    # the host merge of two shards of the matrix is the whole
    from tinyedm_amd.evaluate import level_stats, level_sums, merge_level_sums
    m = merge_level_sums([level_sums(a["se"].numpy()[:, :, r::2], 768) for r in range(2)])
    st = level_stats(m, a["sigma"], 0.5)
    assert max(abs(x - y) / y for x, y in zip(st["mse"], a["mse"])) <= 1e-12


# ------------------------------------------------------------------ 7. against the CPU oracle
def _edm(P, ecfg, dcfg, dtype, use_uncertainty=False):
    """an eval-mode EDM on the GPU with the oracle's parameters"""
    import tinyedm_amd as T
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), dcfg.dropout_rate,
                     dcfg.sigma_data, dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    emb.load_state_dict({k[len("embedding."):]: v for k, v in P.items() if k.startswith("embedding.")}, strict=True)
    den.load_state_dict({k[len("denoiser."):]: v for k, v in P.items() if k.startswith("denoiser.")}, strict=True)
    den.set_eval_dtype(dtype)
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False,
                  use_uncertainty=use_uncertainty, steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01)
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def tiny():
    em, dm = tiny_cfgs(10)
    P = O.init_params(em, dm, torch.Generator().manual_seed(7))
    g = torch.Generator().manual_seed(3)
    images = 0.5 * torch.randn(8, 3, 8, 8, generator=g)
    labels = torch.randint(0, 10, (8,), generator=g)
    return em, dm, P, images, labels


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_evaluator_vs_oracle(ops, tiny, dtype):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    em, dm, P, images, labels = tiny
    bf16 = dtype == "bf16"
    lim = 1e-2 if bf16 else 2e-4            # the project's limits: tests/test_network_gpu.py, tests/test_evalf32_gpu.py
    model = _edm(P, em, dm, "bf16")         # (the evaluator switches the precision itself)
    sigmas = [0.05, 0.8, 20.0]
    ids = [3, 11, 4, 100, 8, 9, 77, 5]
    seed, chw = 21, 3 * 8 * 8
    from tinyedm_amd.evaluate import NoiseLevelEvaluator
    # batch_size = 8: a chunk is one level in id order, the batch the direct calls below evaluate
    res = NoiseLevelEvaluator(sigmas=sigmas, seed=seed, batch_size=8, network_dtype=dtype).evaluate(
        model, images.to(DEV), labels.to(DEV), ids=ids)
    assert model.denoiser.eval_dtype == "bf16"          # restored
    order = np.argsort(ids)
    assert res["ids"] == sorted(ids)
    rec = ops.churn_record(seed, 0, DEV)
    sig_dev = _f32(sigmas)
    clean = images[order].contiguous()
    lab = labels[order]
    model.denoiser.set_eval_dtype(dtype)
    for l in range(3):
        noisy, s = ops.eval_diffuse(clean.to(DEV), _u32(sorted(ids)), _i32([l] * 8), sig_dev, rec)
        with torch.no_grad():
            D_gpu = model(noisy, s, lab.to(DEV)).float().cpu()
            D_or = O.edm_forward(P, em, dm, noisy.cpu(), s.cpu(), lab, bf16=bf16).float()
        ratio = rel(D_gpu, D_or)
        record(f"evaluate/{dtype}_level{l}_D_vs_oracle", ratio, lim)
        assert ratio <= lim, (l, ratio)
        se_or = float(((D_or.double() - clean.double()) ** 2).sum())
        se_gpu = res["mse"][l] * 8 * chw
        e = lim * float(D_or.double().norm())
        bound = (2.0 * math.sqrt(se_or) + e) * e
        record(f"evaluate/{dtype}_level{l}_se_vs_oracle_over_bound", abs(se_gpu - se_or) / bound, 1.0)
        print(f"{dtype} level {l}: D rel {ratio:.3e} (limit {lim}), |se - se_oracle| {abs(se_gpu - se_or):.3e} (bound {bound:.3e})")
        assert abs(se_gpu - se_or) <= bound, (l, se_gpu, se_or, bound)
        # and the matrix holds what the op computes on the same operands
        se_direct = ops.eval_sqerr(D_gpu.to(DEV), clean.to(DEV))
        assert torch.equal(se_direct.cpu(), res["se"][0, l])
    model.denoiser.set_eval_dtype("bf16")


# ------------------------------------------------------------------ 8. the uncertainty column
def test_uncertainty_column(ops, tiny):
    em, dm, P, images, labels = tiny
    torch.manual_seed(0)
    model = _edm(P, em, dm, "bf16", use_uncertainty=True)
    assert model.u is not None
    sigmas = [0.05, 0.8, 20.0]
    from tinyedm_amd.evaluate import NoiseLevelEvaluator
    res = NoiseLevelEvaluator(sigmas=sigmas).evaluate(model, images.to(DEV), labels.to(DEV))
    with torch.no_grad():
        four, _ = model.embedding(_f32(sigmas), None)
        want = model.u(four).flatten().float().cpu()
    got = torch.tensor(res["uncertainty"], dtype=torch.float32)
    assert got.shape == (3,) and torch.allclose(got, want, rtol=1e-6, atol=0.0)
    plain = NoiseLevelEvaluator(sigmas=sigmas).evaluate(_edm(P, em, dm, "bf16"), images.to(DEV), labels.to(DEV))
    assert "uncertainty" not in plain and plain["mse"] == res["mse"]


# ------------------------------------------------------------------ 9. the CLI end to end
def test_evaluate_cli(ops, tiny, tmp_path):
    from PIL import Image
    em, dm, P, images, labels = tiny
    paths = []
    for name, seed in (("a", 7), ("b", 11)):
        m = _edm(O.init_params(em, dm, torch.Generator().manual_seed(seed)), em, dm, "bf16")
        paths.append(str(tmp_path / f"{name}.ckpt"))
        torch.save({"hyper_parameters": dict(m.hparams), "state_dict": {k: v.cpu() for k, v in m.state_dict().items()}},
                   paths[-1])
    png = tmp_path / "png"
    png.mkdir()
    g = np.random.default_rng(0)
    for i in range(8):
        Image.fromarray(g.integers(0, 256, size=(8, 8, 3), dtype=np.uint8)).save(png / f"{i}.png")
    with open(tmp_path / "labels.json", "w") as f:
        json.dump([int(v) for v in labels], f)

    def run(report):
        cmd = [sys.executable, "-m", "tinyedm.evaluate", "--ckpt_path", *paths, "--image_dir", str(png), "--image_size",
               "8", "--labels_json", str(tmp_path / "labels.json"), "--num_levels", "3", "--num_images", "8", "--seed",
               "4", "--report", str(report)]
        env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        with open(report) as f:
            return r.stdout, json.load(f)
    out1, rep1 = run(tmp_path / "r1.json")
    out2, rep2 = run(tmp_path / "r2.json")
    assert sorted(rep1["checkpoints"]) == sorted(paths) and len(rep1["sigmas"]) == 3
    want = [float(np.float32(s)) for s in R.level_sigmas(-1.2, 1.2, 3)]
    assert rep1["sigmas"] == want
    for p in paths:
        e = rep1["checkpoints"][p]
        assert len(e["mse"]) == len(e["loss"]) == len(e["sigma"]) == 3 and e["count"] == [8] * 3
        assert all(math.isfinite(v) and v > 0 for v in e["mse"])
        assert e["mse"] == rep2["checkpoints"][p]["mse"]            # bit for bit (repr round trip)
    assert rep1["checkpoints"][paths[0]]["mse"] != rep1["checkpoints"][paths[1]]["mse"]
    best = min(paths, key=lambda p: rep1["checkpoints"][p]["expected_loss"])
    assert rep1["best"] == best and rep1["criterion"] == "expected_loss"
    line = [ln for ln in out1.splitlines() if ln.startswith("lowest expected_loss")]
    assert len(line) == 1 and best in line[0] and not any(p in line[0] for p in paths if p != best)
    assert out1.splitlines()[:-1] == out2.splitlines()[:-1]          # (the last line names the report file)


# ------------------------------------------------------------------ 10. the callback
def test_loss_by_noise_level_callback(ops, tiny):
    import tinyedm_amd as T
    from tinyedm_amd.callbacks import LossByNoiseLevel
    from tinyedm_amd.datamodules import SyntheticImageDataModule
    em, dm, P, _, _ = tiny
    model = _edm(P, em, dm, "bf16")
    data = SyntheticImageDataModule(8, (3, 8, 8), num_classes=10, num_samples=16)
    data.setup()
    cb = LossByNoiseLevel(num_images=8, num_levels=3)
    tr = T.Trainer(max_epochs=1, callbacks=[cb])
    tr.datamodule = data
    logged = []
    for _ in range(2):                      # two validation epochs, no training step in between
        tr.validate(model, data.val_dataloader())
        logged.append({k: v for k, v in tr.callback_metrics.items() if k.startswith("val_")})
    names = {"val_expected_loss", "val_loss_sigma/0", "val_loss_sigma/1", "val_loss_sigma/2"}
    assert names <= set(logged[0]) and "val_loss" in logged[0]
    for k in names:
        assert math.isfinite(logged[0][k]) and logged[0][k] > 0
        assert logged[0][k] == logged[1][k], k
        assert model._logged[k] == logged[1][k]
    assert abs(logged[0]["val_expected_loss"] - sum(logged[0][f"val_loss_sigma/{l}"] for l in range(3)) / 3) <= 1e-12
    assert tuple(cb.images.shape) == (8, 3, 8, 8) and cb.last["count"] == [8, 8, 8]
    # off unless due: every_n_epochs = 2 skips epoch 1
    cb2 = LossByNoiseLevel(num_images=8, every_n_epochs=2, num_levels=3)
    tr2 = T.Trainer(max_epochs=1, callbacks=[cb2])
    tr2.datamodule, tr2.current_epoch = data, 1
    tr2.validate(model, data.val_dataloader())
    assert "val_expected_loss" not in tr2.callback_metrics and cb2.images is None
