"""The diffusion classifier on the GPU (tinyedm_amd/classify.py, ops.eval_diffuse_classes / ops.eval_sqerr_classes in
sample_eval.hip):

 * the two class-sweep kernels bit for bit against the pair they extend, on the dwordx4 path, the scalar path with a
   partial last quad, a misaligned tensor and C = 1; the squared error against numpy fp64; health bit and refusals;
 * the classifier on model-free known answers and its invariances (batch size, order, seed, draws);
 * the [levels, images, classes] matrix and the label-free row against the CPU oracle ("bf16" and "f32"), predictions
   on the images the oracle decides ("f32" only: in bf16 the evaluation error bound exceeds every margin of this
   random-weight network, so no image is decided and only the matrix is checked);
 * true_class_loss against NoiseLevelEvaluator, the CLI end to end with generate --labels_to, the callback."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import classify_ref as CR
from oracle import edm_oracle as O
from oracle.make_golden import tiny_cfgs
from parity_log import record

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x9E3779B97F4A7C15           # a non-zero high word
IDS = [5, 4294967295, 1000003]
LEVELS = [0, 2, 1]
# (P, C, image shape, offset in floats into the allocation)
CASES = [(3, 4, (3, 32, 32), 0), (2, 3, (3, 7, 9), 0), (3, 4, (3, 32, 32), 1), (3, 1, (3, 32, 32), 0)]
CASE_IDS = ["cifar-vec", "odd-scalar", "misaligned-scalar", "one-class"]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as _ops
    return _ops


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


# ------------------------------------------------------------------ 1. the noise of a pair, stored to its C rows
@pytest.mark.parametrize("P,C,shape,offset", CASES, ids=CASE_IDS)
def test_diffuse_classes_rows_are_the_pairs_bits(ops, P, C, shape, offset):
    g = torch.Generator().manual_seed(1)
    clean = _at((0.5 * torch.randn((P,) + shape, generator=g)).to(DEV), offset)
    ids, lev, sig = _u32(IDS[:P]), _i32(LEVELS[:P]), _f32([0.002, 1.0, 80.0])
    rec = ops.churn_record(SEED, 3, DEV)
    want, want_s = ops.eval_diffuse(clean, ids, lev, sig, rec)
    noisy, s = ops.eval_diffuse_classes(clean, ids, lev, sig, rec, C)
    ops.check_health(DEV, "eval_diffuse_classes")
    assert tuple(noisy.shape) == (P * C,) + shape and tuple(s.shape) == (P * C,) and noisy.dtype == s.dtype == torch.float32
    for p in range(P):
        for c in range(C):
            assert torch.equal(noisy[p * C + c], want[p]), (p, c)
    assert torch.equal(s, want_s.repeat_interleave(C)) and torch.equal(s, sig[lev.long()].repeat_interleave(C))
    assert not torch.equal(want[0], clean[0])                      # (noise was added)
    if offset:      # the scalar path of a misaligned tensor draws the dwordx4 path's bits
        again, _ = ops.eval_diffuse_classes(clean.clone(), ids, lev, sig, rec, C)
        assert torch.equal(again, noisy)


def test_diffuse_classes_bad_level_is_nan_and_health(ops):
    """the kernel's documented answer to a level outside [0, L) that the caller did not check: NaN rows and the health
    bit, never an index"""
    rec = ops.churn_record(1, 0, DEV)
    ops.check_health(DEV, "before")
    for shape in ((3, 32, 32), (3, 7, 9)):
        x = torch.zeros((3,) + shape, device=DEV)
        noisy, s = ops.eval_diffuse_classes(x, _u32([0, 1, 2]), _i32([0, 3, -1]), _f32([1.0] * 3), rec, 4,
                                            check_levels=False)
        with pytest.raises(ops.GraphCorruptionError, match="non-finite"):
            ops.check_health(DEV, "eval_diffuse_classes")
        ops.check_health(DEV, "cleared")
        assert bool(torch.isnan(noisy[4:]).all()) and bool(torch.isnan(s[4:]).all())
        assert bool(torch.isfinite(noisy[:4]).all()) and torch.equal(s[:4], torch.ones(4, device=DEV))
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    x[1, 2, 3, 4] = float("nan")
    ops.eval_diffuse_classes(x, _u32([0, 1]), _i32([0, 1]), _f32([1.0] * 3), rec, 2)
    with pytest.raises(ops.GraphCorruptionError, match="non-finite"):
        ops.check_health(DEV, "eval_diffuse_classes")
    ops.check_health(DEV, "after")


# ------------------------------------------------------------------ 2. the squared error against an unreplicated clean
@pytest.mark.parametrize("P,C,shape,offset", CASES, ids=CASE_IDS)
def test_sqerr_classes_vs_replicated_and_numpy(ops, P, C, shape, offset):
    g = torch.Generator().manual_seed(2)
    D0, c0 = torch.randn((P * C,) + shape, generator=g), 0.5 * torch.randn((P,) + shape, generator=g)
    D, clean = _at(D0.to(DEV), offset), _at(c0.to(DEV), offset)
    se = ops.eval_sqerr_classes(D, clean, C)
    ops.check_health(DEV, "eval_sqerr_classes")
    assert se.dtype == torch.float64 and tuple(se.shape) == (P * C,)
    assert torch.equal(se, ops.eval_sqerr(D, _at(clean.repeat_interleave(C, 0), offset)))
    assert torch.equal(se, ops.eval_sqerr(D0.to(DEV), c0.to(DEV).repeat_interleave(C, 0)))        # whatever the memory path
    d = D0.double().numpy() - np.repeat(c0.double().numpy(), C, axis=0)
    ref = (d * d).reshape(P * C, -1).sum(axis=1)
    worst = float((np.abs(se.cpu().numpy() - ref) / ref).max())
    record(f"classify/sqerr_P{P}_C{C}_{'x'.join(map(str, shape))}_off{offset}_rel", worst, 1e-12)
    print(f"sqerr_classes P {P} C {C} {shape} offset {offset}: rel {worst:.3e}")
    assert worst <= 1e-12
    # every row equal to its pair's clean image: exactly zero
    same = _at(clean.repeat_interleave(C, 0), offset)
    assert torch.equal(ops.eval_sqerr_classes(same, clean, C), torch.zeros(P * C, dtype=torch.float64, device=DEV))
    # into a slice of a larger buffer: the rest is untouched
    buf = torch.full((P * C + 13,), -7.0, dtype=torch.float64, device=DEV)
    out = ops.eval_sqerr_classes(D, clean, C, out=buf[5:5 + P * C])
    assert out.data_ptr() == buf[5:].data_ptr() and torch.equal(buf[5:5 + P * C], se)
    assert bool((buf[:5] == -7.0).all()) and bool((buf[5 + P * C:] == -7.0).all())


def test_sqerr_classes_nonfinite_sets_health(ops):
    ops.check_health(DEV, "before")
    for shape, where in (((3, 32, 32), (7, 1, 5, 17)), ((3, 7, 9), (4, 2, 6, 8))):       # vector body / scalar tail
        D = torch.zeros((8,) + shape, device=DEV)
        D[where] = float("nan")
        se = ops.eval_sqerr_classes(D, torch.zeros((2,) + shape, device=DEV), 4)
        with pytest.raises(ops.GraphCorruptionError, match="non-finite"):
            ops.check_health(DEV, "eval_sqerr_classes")
        assert bool(torch.isnan(se[where[0]])) and int(torch.isnan(se).sum()) == 1
    ops.check_health(DEV, "after")


# ------------------------------------------------------------------ 3. refusals
def test_refusals_before_launch(ops):
    from tinyedm_amd import _lib
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    D = torch.zeros(6, 3, 8, 8, device=DEV)
    ids, lev, sig = _u32([0, 1]), _i32([0, 1]), _f32([0.5, 1.0])
    rec = ops.churn_record(0, 0, DEV)
    ops.eval_diffuse_classes(x, ids, lev, sig, rec, 3)
    ops.eval_sqerr_classes(D, x, 3)
    calls = _lib.N_CALLS
    f64 = dict(dtype=torch.float64, device=DEV)
    bad = [
        lambda: ops.eval_diffuse_classes(x, ids, _i32([0, 2]), sig, rec, 3),                   # level == L
        lambda: ops.eval_diffuse_classes(x, ids, _i32([-1, 0]), sig, rec, 3),
        lambda: ops.eval_diffuse_classes(x.double(), ids, lev, sig, rec, 3),
        lambda: ops.eval_diffuse_classes(x, ids.to(torch.int32), lev, sig, rec, 3),
        lambda: ops.eval_diffuse_classes(x, ids, lev.long(), sig, rec, 3),
        lambda: ops.eval_diffuse_classes(x, ids, lev, sig.double(), rec, 3),
        lambda: ops.eval_diffuse_classes(x.cpu(), ids, lev, sig, rec, 3),
        lambda: ops.eval_diffuse_classes(x, ids.cpu(), lev, sig, rec, 3),
        lambda: ops.eval_diffuse_classes(x, ids, lev, sig.cpu(), rec, 3),
        lambda: ops.eval_diffuse_classes(x, ids, lev, sig, rec.cpu(), 3),
        lambda: ops.eval_diffuse_classes(x.transpose(2, 3), ids, lev, sig, rec, 3),
        lambda: ops.eval_diffuse_classes(x, _u32([0, 1, 2]), lev, sig, rec, 3),
        lambda: ops.eval_diffuse_classes(x, ids, lev, sig.view(1, 2), rec, 3),
        lambda: ops.eval_diffuse_classes(x, ids, lev, torch.ones(65536, device=DEV), rec, 3),
        lambda: ops.eval_diffuse_classes(x, ids, lev, sig, rec[:3], 3),
        lambda: ops.eval_diffuse_classes(torch.zeros(4, device=DEV), ids, lev, sig, rec, 3),
        lambda: ops.eval_diffuse_classes(x, ids, lev, sig, rec, 0),
        lambda: ops.eval_diffuse_classes(x, ids, lev, sig, rec, -1),
        lambda: ops.eval_diffuse_classes(x, ids, lev, sig, rec, 3.0),
        lambda: ops.eval_diffuse_classes(x, ids, lev, sig, rec, True),
        lambda: ops.eval_sqerr_classes(D.double(), x, 3),
        lambda: ops.eval_sqerr_classes(D, x.double(), 3),
        lambda: ops.eval_sqerr_classes(D, x.cpu(), 3),
        lambda: ops.eval_sqerr_classes(D.cpu(), x, 3),
        lambda: ops.eval_sqerr_classes(D.transpose(2, 3), x, 3),
        lambda: ops.eval_sqerr_classes(D, x.transpose(2, 3), 3),
        lambda: ops.eval_sqerr_classes(D, x, 0),
        lambda: ops.eval_sqerr_classes(D, x, 2),                                                # 6 rows are not 2 * 2
        lambda: ops.eval_sqerr_classes(D, x, 4),
        lambda: ops.eval_sqerr_classes(D[:5], x, 3),
        lambda: ops.eval_sqerr_classes(D, x, 32768),                                            # P * C = 65536
        lambda: ops.eval_sqerr_classes(D, x, 3, out=torch.zeros(6, device=DEV)),
        lambda: ops.eval_sqerr_classes(D, x, 3, out=torch.zeros(5, **f64)),
        lambda: ops.eval_sqerr_classes(D, x, 3, out=torch.zeros(2, **f64)),
        lambda: ops.eval_sqerr_classes(D, x, 3, out=torch.zeros(12, **f64)[::2]),
        lambda: ops.eval_sqerr_classes(D, x, 3, out=torch.zeros(6, dtype=torch.float64)),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
        assert _lib.N_CALLS == calls, i          # nothing reached the library
    ops.check_health(DEV, "refusals")


# ------------------------------------------------------------------ 4. known answers without a network
def _clf(**kw):
    from tinyedm_amd.classify import DiffusionClassifier
    kw.setdefault("num_levels", 4)
    kw.setdefault("P_mean", -1.2)
    kw.setdefault("P_std", 1.2)
    return DiffusionClassifier(**kw)


def test_known_answers_with_prototypes(ops):
    g = torch.Generator().manual_seed(11)
    proto = torch.randn(4, 3, 16, 16, generator=g)
    proto[3] = proto[1]
    y = torch.arange(32) % 4
    x = proto[y] + 0.01 * torch.randn(32, 3, 16, 16, generator=g)
    proto_d, chw = proto.to(DEV), 3 * 16 * 16

    def model(noisy, sigma, c):
        return proto_d[c]
    want_pred = torch.where(y == 3, torch.ones_like(y), y)           # classes 1 and 3 tie exactly: the lower index
    res = {}
    for draws in (1, 2):
        res[draws] = r = _clf(num_classes=4, num_draws=draws, batch_size=44).classify(model, x.to(DEV), y.to(DEV))
        assert tuple(r["se"].shape) == (draws, 4, 32, 4) and tuple(r["scores"].shape) == (32, 4)
        assert torch.equal(r["pred"], want_pred)
        w = r["weights"]
        assert w == [(s * s + 0.25) / (s * 0.5) ** 2 for s in r["sigma"]]
        d = proto.double().numpy()[None] - x.double().numpy()[:, None]            # [n, C, ...]
        ref = (d * d).reshape(32, 4, -1).sum(axis=2) / chw * math.fsum(w)
        worst = float((np.abs(r["scores"].numpy() - ref) / ref).max())
        record(f"classify/prototype_scores_draws{draws}_rel", worst, 1e-12)
        print(f"prototype scores, draws {draws}: rel {worst:.3e}")
        assert worst <= 1e-12
        # by hand: 8 images of each class; classes 0, 1, 2 are right, every class 3 image is answered as 1
        assert r["accuracy"] == 0.75 and r["count"] == 32 and r["per_class_accuracy"] == [1.0, 1.0, 1.0, 0.0]
        assert abs(r["accuracy_stderr"] - math.sqrt(0.75 * 0.25 / 32)) <= 1e-15
        assert r["confusion"] == [[8, 0, 0, 0], [0, 8, 0, 0], [0, 0, 8, 0], [0, 8, 0, 0]]
        assert r["level_accuracy"] == [0.75] * 4 and r["pred_histogram"] == [8, 16, 8, 0]
        m = r["margin"].numpy()
        assert (m[(y == 1) | (y == 3)] == 0.0).all() and (m[(y == 0) | (y == 2)] > 0.0).all()
        assert r["margin_quantiles"]["min"] == 0.0 and r["num_classes"] == 4 and r["num_draws"] == draws
    # the noise does not enter: one draw and two give the same numbers
    assert torch.equal(res[1]["scores"], res[2]["scores"]) and torch.equal(res[1]["se"][0], res[2]["se"][1])
    assert res[1]["confusion"] == res[2]["confusion"] and res[1]["true_class_loss"] == res[2]["true_class_loss"]
    # without labels: predictions and margins only; labels outside [0, C) and too small a batch are refused
    plain = _clf(num_classes=4).classify(model, x.to(DEV))
    assert "accuracy" not in plain and "confusion" not in plain and torch.equal(plain["pred"], want_pred)
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        _clf(num_classes=4).classify(model, x.to(DEV), (y + 1).to(DEV))
    with pytest.raises(ValueError, match="num_classes"):
        _clf().classify(model, x.to(DEV))


# ------------------------------------------------------------------ 5. invariances
def test_invariance_with_callables(ops):
    g = torch.Generator().manual_seed(5)
    x = (0.5 * torch.randn(24, 3, 16, 16, generator=g)).to(DEV)
    y = (torch.arange(24) % 10).to(DEV)

    def model(noisy, sigma, c):
        return 0.75 * noisy + 0.01 * c.float().view(-1, 1, 1, 1)
    a = _clf(num_classes=10, batch_size=40, seed=9).classify(model, x, y)
    b = _clf(num_classes=10, batch_size=320, seed=9).classify(model, x, y)
    assert torch.equal(a["se"], b["se"]) and torch.equal(a["scores"], b["scores"]) and a["confusion"] == b["confusion"]
    assert bool((a["se"] > 0).all()) and not torch.equal(a["se"][..., 0], a["se"][..., 1])
    # ids carry the noise: a permuted set with its ids gives the same matrix
    perm = torch.randperm(24, generator=torch.Generator().manual_seed(1))
    c = _clf(num_classes=10, batch_size=40, seed=9).classify(model, x[perm.to(DEV)].contiguous(), y[perm.to(DEV)], ids=perm)
    assert torch.equal(c["se"], a["se"]) and c["ids"] == list(range(24)) and torch.equal(c["pred"], a["pred"])
    assert c["confusion"] == a["confusion"]
    # the seed reproduces, another seed differs, draw 0 of two draws is the single draw
    assert torch.equal(_clf(num_classes=10, batch_size=40, seed=9).classify(model, x, y)["se"], a["se"])
    assert not torch.equal(_clf(num_classes=10, batch_size=40, seed=10).classify(model, x, y)["se"], a["se"])
    d2 = _clf(num_classes=10, batch_size=70, seed=9, num_draws=2).classify(model, x, y)
    assert torch.equal(d2["se"][0], a["se"][0]) and not torch.equal(d2["se"][1], a["se"][0])
    # label_gain with a callable that ignores a missing label
    def model_n(noisy, sigma, c):
        return 0.75 * noisy + (0.0 if c is None else 0.01 * c.float().view(-1, 1, 1, 1))
    e = _clf(num_classes=10, batch_size=40, seed=9, label_gain=True).classify(model_n, x, y)
    assert torch.equal(e["se"], a["se"]) and len(e["label_gain"]) == len(e["label_gain_stderr"]) == 4
    true_se = e["se"][0].numpy()[:, np.arange(24), y.cpu().numpy()]
    want = ((e["se_unlabelled"][0].numpy() - true_se) / 768).mean(axis=1)
    assert np.abs(np.asarray(e["label_gain"]) - want).max() <= 1e-12 * np.abs(want).max()


# ------------------------------------------------------------------ 6. against the CPU oracle
def _edm(P, ecfg, dcfg, dtype):
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
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                  steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01)
    return model.to(DEV).eval()


SIGMAS = [0.05, 0.8, 20.0]
TINY_IDS = [3, 11, 4, 100, 8, 9, 77, 5]


@pytest.fixture(scope="module")
def tiny():
    em, dm = tiny_cfgs(10)
    P = O.init_params(em, dm, torch.Generator().manual_seed(7))
    g = torch.Generator().manual_seed(3)
    images = 0.5 * torch.randn(8, 3, 8, 8, generator=g)
    labels = torch.randint(0, 10, (8,), generator=g)
    return em, dm, P, images, labels


@pytest.fixture(scope="module")
def oracle_se(ops, tiny):
    """per precision, computed once: the oracle's squared errors [3, 8, 10] and [3, 8] (label-free) of the images in id
    order under the kernel's noise, and the norms of its outputs"""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    em, dm, P, images, labels = tiny
    order = np.argsort(TINY_IDS)
    clean = images[order].contiguous()
    rec = ops.churn_record(21, 0, DEV)
    cache = {}

    def get(bf16):
        if bf16 not in cache:
            se, nrm = np.zeros((3, 8, 11)), np.zeros((3, 8, 11))
            for l in range(3):
                noisy, s = ops.eval_diffuse(clean.to(DEV), _u32(sorted(TINY_IDS)), _i32([l] * 8), _f32(SIGMAS), rec)
                noisy, s = noisy.cpu(), s.cpu()
                with torch.no_grad():
                    D = O.edm_forward(P, em, dm, noisy.repeat_interleave(10, 0), s.repeat_interleave(10),
                                      torch.arange(10).repeat(8), bf16=bf16).double().view(8, 10, -1)
                    D0 = O.edm_forward(P, em, dm, noisy, s, None, bf16=bf16).double().view(8, 1, -1)
                D = torch.cat([D, D0], dim=1)                                  # column 10: no label
                se[l] = ((D - clean.double().view(8, 1, -1)) ** 2).sum(dim=2).numpy()
                nrm[l] = D.norm(dim=2).numpy()
            cache[bf16] = (se, nrm)
        return cache[bf16]
    return get


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_classifier_vs_oracle(ops, tiny, oracle_se, dtype):
    """every entry of the se matrix, and of the label-free row, within the bound test_evaluate_gpu.py uses, taken per
    image: (2 sqrt(se_or) + e) e with e = lim * ||D_or||.  Predictions are compared in f32 only, on the images the oracle
    decides (oracle margin > twice the largest weighted bound over the image's classes); at least 6 of 8 must be.
    Measured on an MI355X, images in id order: margin / threshold 5.72, 2.85, 4.6, 1.78, 4.88, 6.59, 5.8, 11.32 (all 8
    decided, oracle predictions [2 2 2 2 2 2 7 3]); at the level 0.8 alone >= 3.86.  In bf16 the same ratios are 0.04 to
    0.21: the bound exceeds every margin of this random-weight network, no image is decided there, and only the matrix
    is checked.  Worst |se - se_oracle| / bound: 0.16 (bf16), 2.2e-3 (f32)."""
    from tinyedm_amd import classify as K
    em, dm, P, images, labels = tiny
    bf16 = dtype == "bf16"
    lim = 1e-2 if bf16 else 2e-4            # the project's limits: tests/test_network_gpu.py, tests/test_evalf32_gpu.py
    model = _edm(P, em, dm, "bf16")         # (the classifier switches the precision itself)
    chw = 3 * 8 * 8
    res = K.DiffusionClassifier(sigmas=SIGMAS, seed=21, batch_size=80, network_dtype=dtype, weighting="edm",
                                label_gain=True).classify(model, images.to(DEV), labels.to(DEV), ids=TINY_IDS)
    assert model.denoiser.eval_dtype == "bf16"          # restored
    assert res["ids"] == sorted(TINY_IDS) and tuple(res["se"].shape) == (1, 3, 8, 10) and res["num_classes"] == 10
    se_or, nrm = oracle_se(bf16)
    e = lim * nrm
    bound = (2.0 * np.sqrt(se_or) + e) * e                                  # [3, 8, 11]
    got = np.concatenate([res["se"][0].numpy(), res["se_unlabelled"][0].numpy()[:, :, None]], axis=2)
    ratio = np.abs(got - se_or) / bound
    for l in range(3):
        record(f"classify/{dtype}_level{l}_se_vs_oracle_over_bound", float(ratio[l, :, :10].max()), 1.0)
        record(f"classify/{dtype}_level{l}_unlabelled_se_vs_oracle_over_bound", float(ratio[l, :, 10].max()), 1.0)
        print(f"{dtype} level {l}: worst |se - se_oracle| / bound {ratio[l, :, :10].max():.3e} (classes), "
              f"{ratio[l, :, 10].max():.3e} (no label)")
    assert (ratio <= 1.0).all(), ratio.max(axis=(1, 2))
    # the label gain is the mean of the two columns' difference
    y = labels[np.argsort(TINY_IDS)].numpy()
    true_se = got[:, np.arange(8), y]
    want_gain = ((got[:, :, 10] - true_se) / chw).mean(axis=1)
    assert np.abs(np.asarray(res["label_gain"]) - want_gain).max() <= 1e-12 * np.abs(want_gain).max()
    # what the oracle decides: an image whose oracle margin exceeds twice the largest weighted bound over its classes
    w = CR.class_weights(res["sigma"], "edm", 0.5)
    sc_or = CR.class_scores(se_or[None, :, :, :10], chw, w)
    pred_or, margin_or = CR.predict(sc_or)
    thr = 2.0 * CR.class_scores(bound[None, :, :, :10], chw, w).max(axis=1)
    decided = margin_or > thr
    print(f"{dtype}: oracle margin / threshold {np.round(margin_or / thr, 2).tolist()}, oracle predictions {pred_or.tolist()}")
    lp_or = CR.level_predictions(se_or[None, :, :, :10])
    two = np.sort(se_or[1, :, :10], axis=1)
    decided_1 = (two[:, 1] - two[:, 0]) > 2.0 * bound[1, :, :10].max(axis=1)
    print(f"{dtype}: level 1 alone: oracle margin / threshold "
          f"{np.round((two[:, 1] - two[:, 0]) / (2.0 * bound[1, :, :10].max(axis=1)), 2).tolist()}")
    if bf16:
        return
    assert int(decided.sum()) >= 6, (margin_or / thr).tolist()
    assert np.array_equal(res["pred"].numpy()[decided], pred_or[decided])
    assert decided_1.all()
    assert np.array_equal(K.level_predictions(res["se"].numpy())[1], lp_or[1])
    right = (K.level_predictions(res["se"].numpy()) == y[None]).sum(axis=1)
    assert res["level_accuracy"] == [int(v) / 8 for v in right]


# ------------------------------------------------------------------ 7. the true-class loss is evaluate's loss
def test_true_class_loss_is_the_evaluators_loss(ops, tiny):
    """the network's convolution kernels are chosen by the pixel count of a call, so both sides get calls of 10 rows:
    the evaluator 10 (image, level) pairs, the classifier one pair under its 10 classes.  The figure for calls of
    different sizes (8 and 80 rows) is printed beside it; on this network both measured exactly 0 on an MI355X."""
    from tinyedm_amd.classify import DiffusionClassifier
    from tinyedm_amd.evaluate import NoiseLevelEvaluator
    em, dm, P, images, labels = tiny
    model = _edm(P, em, dm, "bf16")
    sig = [0.05, 0.3, 0.8, 3.0, 20.0]                      # 5 levels x 8 images = 4 evaluator calls of 10 pairs
    x, y = images.to(DEV), labels.to(DEV)
    ev = NoiseLevelEvaluator(sigmas=sig, seed=21, batch_size=10).evaluate(model, x, y, ids=TINY_IDS)
    cl = DiffusionClassifier(sigmas=sig, seed=21, batch_size=10).classify(model, x, y, ids=TINY_IDS)
    worst = max(abs(a - b) / b for a, b in zip(cl["true_class_loss"], ev["loss"]))
    other = DiffusionClassifier(sigmas=sig, seed=21, batch_size=80).classify(model, x, y, ids=TINY_IDS)
    ev8 = NoiseLevelEvaluator(sigmas=sig, seed=21, batch_size=8).evaluate(model, x, y, ids=TINY_IDS)
    print(f"true_class_loss vs evaluate's loss: rel {worst:.3e} (10-row calls); "
          f"{max(abs(a - b) / b for a, b in zip(other['true_class_loss'], ev8['loss'])):.3e} (80-row against 8-row calls)")
    record("classify/true_class_loss_vs_evaluate_rel", worst, 1e-12)
    assert worst <= 1e-12, (cl["true_class_loss"], ev["loss"])
    assert cl["ids"] == ev["ids"] and cl["sigma"] == ev["sigma"]


# ------------------------------------------------------------------ 8. the CLI end to end
def test_classify_cli_and_generate_labels(ops, tiny, tmp_path):
    from PIL import Image
    from tinyedm_amd import classify as K
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
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    report = tmp_path / "r.json"
    cmd = [sys.executable, "-m", "tinyedm.classify", "--ckpt_path", *paths, "--image_dir", str(png), "--image_size", "8",
           "--labels_json", str(tmp_path / "labels.json"), "--num_levels", "3", "--num_images", "8", "--seed", "4",
           "--batch_size", "40", "--label_gain", "--report", str(report)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(report) as f:
        rep = json.load(f)
    assert sorted(rep["checkpoints"]) == sorted(paths) and len(rep["sigmas"]) == 3 and rep["num_images"] == 8
    assert rep["weighting"] == "edm" and rep["criterion"] == "accuracy" and rep["labelled"] is True
    # the direct call on the same images
    from tinyedm_amd.edm import EDM
    from tinyedm_amd.generate import CIFAR_MEAN, CIFAR_STD, load_images
    x = load_images(str(png), CIFAR_MEAN, CIFAR_STD, 8, 3).to(DEV)
    clf = K.DiffusionClassifier(num_levels=3, seed=4, batch_size=40, label_gain=True)
    for p in paths:
        e = rep["checkpoints"][p]
        d = clf.classify(EDM.load_from_checkpoint(p).to(DEV).eval(), x, labels.to(DEV))
        assert e["confusion"] == d["confusion"] and e["accuracy"] == d["accuracy"] and e["count"] == 8
        assert e["level_accuracy"] == d["level_accuracy"] and e["true_class_loss"] == d["true_class_loss"]
        assert e["label_gain"] == d["label_gain"] and e["margin_quantiles"] == d["margin_quantiles"]
        assert not any(k in e for k in ("se", "scores", "pred", "ids", "margin", "se_unlabelled"))
        assert np.asarray(e["confusion"]).sum() == 8 and f"{e['accuracy']:.4f}" in r.stdout
    best = paths[0] if rep["checkpoints"][paths[0]]["accuracy"] >= rep["checkpoints"][paths[1]]["accuracy"] else paths[1]
    assert rep["best"] == best
    assert "confusion (true class = row" in r.stdout and "gain[0]" in r.stdout
    # generate --labels_to: a list of the sample count's length that --labels_json accepts
    out, lab = tmp_path / "samples", tmp_path / "drawn.json"
    cmd = [sys.executable, "-m", "tinyedm.generate", "--ckpt_path", paths[0], "--output_dir", str(out), "--num_samples",
           "6", "--image_size", "8", "--num_classes", "10", "--batch_size", "4", "--num_steps", "4", "--network_dtype",
           "bf16", "--seed", "2", "--labels_to", str(lab)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(lab) as f:
        drawn = json.load(f)
    assert isinstance(drawn, list) and len(drawn) == 6 and all(isinstance(v, int) and 0 <= v < 10 for v in drawn)
    assert sorted(os.listdir(out)) == [f"{i}.png" for i in range(6)]
    rep2 = K.main(["--ckpt_path", paths[0], "--image_dir", str(out), "--image_size", "8", "--labels_json", str(lab),
                   "--sigmas", "0.5", "2.0", "--num_images", "6", "--batch_size", "20", "--report",
                   str(tmp_path / "r2.json")])
    e2 = rep2["checkpoints"][paths[0]]
    assert e2["count"] == 6 and np.asarray(e2["confusion"]).sum(axis=1).tolist() == np.bincount(drawn, minlength=10).tolist()
    # without labels: the predicted-class histogram and the margins, no accuracy
    rep3 = K.main(["--ckpt_path", paths[0], "--image_dir", str(out), "--image_size", "8", "--sigmas", "0.5", "2.0",
                   "--num_images", "6", "--batch_size", "20", "--report", str(tmp_path / "r3.json")])
    e3 = rep3["checkpoints"][paths[0]]
    assert "accuracy" not in e3 and "confusion" not in e3 and rep3["best"] is None and rep3["labelled"] is False
    assert sum(e3["pred_histogram"]) == 6 and e3["pred_histogram"] == e2["pred_histogram"]
    assert set(e3["margin_quantiles"]) == {"min", "p05", "p50"}


# ------------------------------------------------------------------ 9. the callback
def test_classifier_accuracy_callback(ops, tiny):
    import tinyedm_amd as T
    from tinyedm_amd.callbacks import ClassifierAccuracy
    from tinyedm_amd.datamodules import SyntheticImageDataModule
    em, dm, P, _, _ = tiny
    model = _edm(P, em, dm, "bf16")
    data = SyntheticImageDataModule(8, (3, 8, 8), num_classes=10, num_samples=16)
    data.setup()
    cb = ClassifierAccuracy(num_images=8, num_levels=3, batch_size=40)
    tr = T.Trainer(max_epochs=1, callbacks=[cb])
    tr.datamodule = data
    logged = []
    for _ in range(2):                      # two validation epochs, no training step in between
        tr.validate(model, data.val_dataloader())
        logged.append({k: v for k, v in tr.callback_metrics.items() if k.startswith("val_")})
    names = {"val_class_acc", "val_class_acc_sigma/0", "val_class_acc_sigma/1", "val_class_acc_sigma/2"}
    assert names <= set(logged[0]) and "val_loss" in logged[0]
    for k in names:
        assert 0.0 <= logged[0][k] <= 1.0 and logged[0][k] * 8 == round(logged[0][k] * 8)
        assert logged[0][k] == logged[1][k], k
        assert model._logged[k] == logged[1][k]
    assert tuple(cb.images.shape) == (8, 3, 8, 8) and cb.last["count"] == 8
    assert logged[0]["val_class_acc"] == cb.last["accuracy"]
    # off unless due: every_n_epochs = 2 skips epoch 1
    cb2 = ClassifierAccuracy(num_images=8, every_n_epochs=2, num_levels=3)
    tr2 = T.Trainer(max_epochs=1, callbacks=[cb2])
    tr2.datamodule, tr2.current_epoch = data, 1
    tr2.validate(model, data.val_dataloader())
    assert "val_class_acc" not in tr2.callback_metrics and cb2.images is None
    # an unconditional model has no classes to tell apart
    em0, dm0 = tiny_cfgs(None)
    plain = _edm(O.init_params(em0, dm0, torch.Generator().manual_seed(7)), em0, dm0, "bf16")
    tr3 = T.Trainer(max_epochs=1, callbacks=[ClassifierAccuracy(num_images=8, num_levels=3)])
    tr3.datamodule = data
    with pytest.raises(RuntimeError, match="unconditional"):
        tr3.validate(plain, data.val_dataloader())
    from tinyedm_amd.classify import DiffusionClassifier
    with pytest.raises(ValueError, match="unconditional"):
        DiffusionClassifier(num_levels=3).classify(plain, torch.zeros(2, 3, 8, 8, device=DEV))
