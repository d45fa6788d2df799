"""The ideal denoiser of a training set on the GPU (csrc/ideal.hip through ops.ideal_denoise, IdealDenoiser, the solvers,
NoiseLevelEvaluator and the gap report) against the fp64 numpy restatement tests/ideal_ref.py.

Tolerances.  For D, lse and entropy of a case: tol = 8 * max(err_b, err_c) + floor, where err_b / err_c are the max-abs
errors of the restatement's fp32 direct and fp32 expansion forms against its fp64 form ON THAT CASE'S INPUTS (computed
here, never from the code under test), floor = 2^-20 for D (eight ulps of a convex combination of values in [-1, 1]) and
2^-20 max(1, |value|) for the statistics.  Every test prints err_gpu / max(err_b, err_c) before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ideal_cases as IC
import ideal_ref as IR

DEV = "cuda"
ULP8 = 2.0 ** -20


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tinyedm_amd import ops as o
    o.health(DEV).zero_()
    return o


def _dev_u8(data, misaligned=False):
    """the set on the device; misaligned: its first byte at an odd address"""
    t = torch.from_numpy(np.ascontiguousarray(data))
    if not misaligned:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=torch.uint8, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 2 == 1 and v.is_contiguous()
    return v


def _dev_f32(x, misaligned=False):
    """the queries on the device; misaligned: one element past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if not misaligned:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _ideal(data, name=None, labels=None, **kw):
    from tinyedm_amd.ideal import IdealDenoiser
    chunk, mis = (IC.SHAPES[name][5], IC.SHAPES[name][6]) if name is not None else (None, False)
    kw.setdefault("ref_chunk", chunk)
    return IdealDenoiser(_dev_u8(data, mis), labels, **kw)


def _np(t):
    return t.detach().double().cpu().numpy()


def _compare(tag, st, truth, tol, errs):
    """D, lse and entropy of a stats() result against the fp64 truth under the tolerance rule; prints the ratios first"""
    Q = truth["D"].shape[0]
    got = {"D": _np(st["D"]).reshape(Q, -1), "lse": _np(st["lse"]), "entropy": _np(st["entropy"])}
    err = {k: float(np.abs(got[k] - truth[k]).max()) for k in got}
    print(f"[ideal] {tag}: " + "  ".join(
        f"{k} err {err[k]:.3e} tol {tol[k]:.3e} ratio {err[k] / errs[k] if errs[k] > 0 else float('nan'):.2f}" for k in got))
    for k in got:
        assert np.isfinite(got[k]).all(), (tag, k)
        assert err[k] <= tol[k], (tag, k, err[k], tol[k])
    return got


# ------------------------------------------------------------------ 1. parity with fp64
@pytest.mark.parametrize("name", list(IC.SHAPES))
@pytest.mark.parametrize("kind", ["soft", "hard"])
def test_parity(ops, name, kind):
    inp, truth, tol, errs = IC.cached(kind, name)
    data, x, sig = inp[:3]
    R = data.shape[0]
    if kind == "soft" and R > 1:          # the case is soft on the truth alone, or it proves nothing about the softmax
        eff = float(truth["effective_count"].mean())
        print(f"[ideal] {name}: mean effective count {eff:.2f} of {R}")
        assert 2.0 <= eff <= R / 2.0
    ideal = _ideal(data, name)
    mis = IC.SHAPES[name][6]
    st = ideal.stats(_dev_f32(x, mis), torch.from_numpy(sig).to(DEV))
    ops.check_health(DEV, "test_parity")
    _compare(f"{name}/{kind}", st, truth, tol, errs)
    # where one image holds the weight the index is that image's, and the weight agrees
    sure = truth["top_weight"] > 0.99
    assert np.array_equal(st["top_index"].cpu().numpy()[sure], truth["top_index"][sure])
    assert np.abs(_np(st["top_weight"]) - truth["top_weight"]).max() <= tol["entropy"] + tol["D"]
    assert np.abs(_np(st["effective_count"]) - np.exp(_np(st["entropy"]))).max() <= 1e-4 * R
    lp = IR.log_density(_np(st["lse"]), R, x[0].size, sig.astype(np.float64))
    assert np.allclose(st["log_density"], lp, rtol=1e-13, atol=0.0)
    D = ideal(_dev_f32(x, mis), torch.from_numpy(sig).to(DEV))
    assert D.shape == tuple(x.shape) and D.dtype == torch.float32 and torch.equal(D, st["D"])


def test_scalar_sigma(ops):
    """a Python float and a 0-d tensor (what the solvers pass) are the [B] tensor of that value, bit for bit, and correct"""
    data, x, _ = IC.soft_case("chunks")
    ideal = _ideal(data, "chunks")
    xd = _dev_f32(x)
    a = ideal(xd, 0.5)
    b = ideal(xd, torch.tensor(0.5, device=DEV))
    c = ideal(xd, torch.full((x.shape[0],), 0.5, device=DEV))
    assert torch.equal(a, b) and torch.equal(a, c)
    truth, tol, errs = IC.references(data, x, np.float32(0.5))
    _compare("chunks/sigma=0.5", ideal.stats(xd, 0.5), truth, tol, errs)
    with pytest.raises(ValueError):
        ideal(xd, 0.0)
    with pytest.raises(ValueError):
        ideal(xd, float("nan"))
    with pytest.raises(RuntimeError):
        ideal(torch.from_numpy(x), 0.5)           # a CPU tensor
    with pytest.raises(ValueError):
        ideal(xd[:, :2], 0.5)


# ------------------------------------------------------------------ 2. the one-hot regime
@pytest.mark.parametrize("name", list(IC.SHAPES))
def test_one_hot(ops, name):
    Q, R, C, H, W, _, mis = IC.SHAPES[name]
    rng = np.random.default_rng(31 + R)
    data = rng.integers(0, 256, (R, C, H, W), dtype=np.uint8)
    j = rng.integers(0, R, Q)
    y = IR.normalize(data).reshape(R, C, H, W)
    x = (y[j] + 0.002 * rng.standard_normal((Q, C, H, W))).astype(np.float32)
    st = _ideal(data, name).stats(_dev_f32(x, mis), 0.002)
    assert np.array_equal(st["top_index"].cpu().numpy(), j)
    err = np.abs(_np(st["D"]) - y[j]).max()
    print(f"[ideal] one-hot {name}: |D - y_j| {err:.3e}")
    assert err <= ULP8
    assert torch.equal(st["top_weight"], torch.ones(Q, device=DEV))
    assert float(st["entropy"].abs().max()) == 0.0


# ------------------------------------------------------------------ 3. ties
def test_ties(ops):
    Q, R, C, H, W, chunk, _ = IC.SHAPES["chunks"]
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, (R, C, H, W), dtype=np.uint8)
    data[130] = data[3]                   # the pair in two chunks of 64
    data[11] = data[10]                   # the pair in one
    data[199] = data[70]
    first = np.array([3, 10, 70, 3, 10])
    y = IR.normalize(data).reshape(R, C, H, W)
    x = (y[first] + 0.05 * rng.standard_normal((5, C, H, W))).astype(np.float32)
    for ref_chunk in (chunk, None):
        st = _ideal(data, ref_chunk=ref_chunk).stats(_dev_f32(x), 0.05)
        assert np.array_equal(st["top_index"].cpu().numpy(), first)          # the lower index of each pair
        assert np.abs(_np(st["D"]) - y[first]).max() <= ULP8
        assert torch.equal(st["top_weight"], torch.full((5,), 0.5, device=DEV))
        assert np.abs(_np(st["entropy"]) - np.log(2.0)).max() <= ULP8


# ------------------------------------------------------------------ 4. class restriction
def test_class_restriction(ops):
    data, x, sig = IC.soft_case("chunks")
    Q, R = x.shape[0], data.shape[0]
    ref_labels = np.arange(R) % 3
    ref_labels[5] = 3                                   # a class with a single image
    labels = np.array([q % 4 for q in range(Q)])
    truth, tol, errs = IC.references(data, x, sig, ref_labels, labels)
    ideal = _ideal(data, "chunks", ref_labels)
    assert ideal.num_classes == 4
    xd, sd = _dev_f32(x), torch.from_numpy(sig).to(DEV)
    st = ideal.stats(xd, sd, torch.from_numpy(labels).to(DEV))
    _compare("chunks/classes", st, truth, tol, errs)
    got_idx = st["top_index"].cpu().numpy()
    assert (ref_labels[got_idx] == labels).all()
    counts = np.bincount(ref_labels)
    assert np.allclose(st["log_density"], IR.log_density(_np(st["lse"]), counts[labels], x[0].size, sig.astype(np.float64)),
                       rtol=1e-13, atol=0.0)
    # the class with one image returns it at every sigma
    y5 = IR.normalize(data)[5]
    for s in (0.002, 0.5, 80.0):
        one = ideal.stats(xd[:3], s, torch.full((3,), 3, device=DEV))
        assert np.abs(_np(one["D"]).reshape(3, -1) - y5).max() <= ULP8
        assert (one["top_index"] == 5).all() and torch.equal(one["top_weight"], torch.ones(3, device=DEV))
    # no labels in the call: every image, and the bits of the object that never had labels
    assert torch.equal(ideal(xd, sd), _ideal(data, "chunks")(xd, sd))
    # a set without labels is unconditional: labels handed to it (a guide's) change nothing
    assert torch.equal(ideal(xd, sd), _ideal(data, "chunks")(xd, sd, torch.from_numpy(labels).to(DEV)))


# ------------------------------------------------------------------ 5. bit stability
def test_bit_stability(ops):
    (data, x, sig), truth, tol, errs = IC.cached("soft", "cifar")
    ideal = _ideal(data, "cifar")
    xd, sd = _dev_f32(x), torch.from_numpy(sig).to(DEV)
    full = ideal.stats_device(xd, sd)
    again = ideal.stats_device(xd, sd)
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    for lo in (0, 65):                    # the first rows, and rows that sit elsewhere in their tile when they come alone
        part = ideal.stats_device(xd[lo:lo + 3].contiguous(), sd[lo:lo + 3].contiguous())
        for a, b in zip(full, part):
            assert torch.equal(a[lo:lo + 3], b), lo
    # another chunking is another summation order: within the tolerance, not bit for bit
    st = _ideal(data, ref_chunk=64).stats(xd, sd)
    _compare("cifar/ref_chunk=64", st, truth, tol, errs)
    assert np.abs(_np(st["D"]) - _np(full[0])).max() <= tol["D"]


# ------------------------------------------------------------------ 6. bad values
def test_bad_values(ops):
    from tinyedm_amd.ops import GraphCorruptionError
    data, x, sig = IC.soft_case("chunks")
    R = data.shape[0]
    ref_labels = np.arange(R) % 3
    ideal = _ideal(data, "chunks", ref_labels)
    xd = _dev_f32(x)
    labels = torch.from_numpy(np.arange(x.shape[0]) % 3).to(DEV)
    good = ideal.stats_device(xd, torch.from_numpy(sig).to(DEV), labels)
    ops.check_health(DEV, "clean call")
    for what in ("sigma", "label", "nan"):
        s, l = torch.from_numpy(sig).to(DEV), labels.clone()
        if what == "sigma":
            s[4] = 0.0
        elif what == "nan":
            s[4] = float("nan")
        else:
            l[4] = 3
        l[9] = -1 if what == "label" else l[9]
        bad = ideal.stats_device(xd, s, l)
        rows = [4, 9] if what == "label" else [4]
        keep = [q for q in range(x.shape[0]) if q not in rows]
        for g, b in zip(good, bad):
            assert torch.equal(g[keep], b[keep]), what
        assert torch.isnan(bad[0][rows]).all() and torch.isnan(bad[1][rows]).all() and torch.isnan(bad[2][rows]).all()
        assert (bad[4][rows] == -1).all()
        with pytest.raises(GraphCorruptionError):
            ops.check_health(DEV, "bad " + what)
        ops.check_health(DEV, "cleared")


def test_wrapper_refusals(ops):
    data, x, sig = IC.soft_case("tails")
    refs, xd, sd = _dev_u8(data), _dev_f32(x), torch.from_numpy(sig).to(DEV)
    norms = ops.u8_norms(refs)
    ops.ideal_denoise(xd, sd, refs, norms)
    for args, kw in (((xd.double(), sd, refs, norms), {}), ((xd, sd[:2], refs, norms), {}),
                     ((xd, sd, refs.float(), norms), {}), ((xd, sd, refs, norms[:2]), {}),
                     ((xd[:, :, :2], sd, refs, norms), {}), ((xd, sd, refs, norms), {"ref_chunk": 0}),
                     ((xd, sd, refs, norms, 0.5, 0.0), {}), ((xd.cpu(), sd, refs, norms), {}),
                     ((xd, sd, refs, norms), {"labels": torch.zeros(3, dtype=torch.int64, device=DEV)})):
        with pytest.raises(ValueError):
            ops.ideal_denoise(*args, **kw)


# ------------------------------------------------------------------ 7. the solvers end on training images
class _Recorder:
    """the ideal denoiser as a model that remembers the top index of its last evaluation"""
    sigma_data = 0.5

    def __init__(self, ideal):
        self.ideal, self.last, self.calls = ideal, None, 0

    def __call__(self, x, sigma, class_labels=None):
        out = self.ideal.stats_device(x, sigma, class_labels)
        self.last, self.calls = out[4], self.calls + 1
        return out[0]


@pytest.fixture(scope="module")
def small_set():
    rng = np.random.default_rng(77)
    data = rng.integers(0, 256, (16, 3, 8, 8), dtype=np.uint8)
    return data, IR.normalize(data).reshape(16, 3, 8, 8), np.arange(16) % 4


@pytest.mark.parametrize("which", ["heun", "churn", "dpmpp"])
@pytest.mark.parametrize("labelled", [False, True])
def test_solvers_end_on_training_images(ops, small_set, which, labelled):
    from tinyedm_amd.solvers import DeterministicSolver, MultistepSolver, StochasticSolver
    data, y, ref_labels = small_set
    model = _Recorder(_ideal(data, labels=ref_labels if labelled else None))
    solver = {"heun": lambda: DeterministicSolver(num_steps=18),
              "churn": lambda: StochasticSolver(num_steps=18, S_churn=10.0, seed=3),
              "dpmpp": lambda: MultistepSolver(num_steps=18, order=2)}[which]()
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(6, 3, 8, 8, generator=g).to(DEV)
    labels = torch.tensor([0, 1, 2, 3, 0, 1], device=DEV) if labelled else None
    out = solver.solve(model, x0, labels)
    ops.check_health(DEV, "solve")
    top = model.last.cpu().numpy()
    assert model.calls >= 18 and (top >= 0).all()
    err = np.abs(_np(out) - y[top]).max()
    print(f"[ideal] {which}{' labelled' if labelled else ''}: ends {err:.3e} from images {top.tolist()}")
    assert err <= ULP8
    if labelled:
        assert np.array_equal(ref_labels[top], labels.cpu().numpy())


def test_guided_solve(ops, small_set):
    from tinyedm_amd.solvers import DeterministicSolver
    data, y, ref_labels = small_set
    cond = _ideal(data, labels=ref_labels)
    solver = DeterministicSolver(num_steps=8, guide=_ideal(data), guidance=1.5)
    x0 = torch.randn(4, 3, 8, 8, generator=torch.Generator().manual_seed(2)).to(DEV)
    out = solver.solve(cond, x0, torch.tensor([0, 1, 2, 3], device=DEV))
    ops.check_health(DEV, "guided solve")
    assert out.shape == x0.shape and torch.isfinite(out).all()


# ------------------------------------------------------------------ 8. NoiseLevelEvaluator
def _train24():
    rng = np.random.default_rng(24)
    data = np.zeros((24, 3, 8, 8), dtype=np.uint8)
    for g, s in enumerate((2, 4, 8, 16)):               # spreads for sigma ~ 0.2 .. 2 at K = 192, by trial on the fp64 form
        base = rng.integers(60, 196, (3, 8, 8))
        data[g::4] = np.clip(base[None] + rng.integers(-s, s + 1, (6, 3, 8, 8)), 0, 255).astype(np.uint8)
    return data


def test_evaluate(ops):
    import evaluate_ref as ER
    from tinyedm_amd.evaluate import NoiseLevelEvaluator
    data = _train24()
    ideal = _ideal(data)
    y = IR.normalize(data).reshape(24, 3, 8, 8)
    images = ops.u8_gather_normalize(ideal.data, torch.arange(24, device=DEV), 0.5, 0.5)
    assert np.abs(_np(images) - y).max() <= 2.0 ** -22
    res = {b: NoiseLevelEvaluator(num_levels=4, P_mean=-0.4, P_std=1.0, seed=5, batch_size=b).evaluate(ideal, images)
           for b in (7, 64)}
    assert torch.equal(res[7]["se"], res[64]["se"]) and res[7]["mse"] == res[64]["mse"]
    sigmas = res[7]["sigma"]
    clean = _np(images)
    effs = []
    for l, s in enumerate(sigmas):
        n = ER.eval_noise((24, 3, 8, 8), list(range(24)), [l] * 24, 5, 0)
        x = (clean + s * n).astype(np.float32)
        truth, tol, errs = IC.references(data, x, np.float32(s))
        effs.append(truth["effective_count"].mean())
        mse = float(((truth["D"] - clean.reshape(24, -1)) ** 2).mean())
        bound = 2.0 * np.sqrt(mse) * tol["D"] + tol["D"] ** 2
        print(f"[ideal] evaluate level {l} sigma {s:.4f}: mse {res[7]['mse'][l]:.6e} truth {mse:.6e} bound {bound:.2e} "
              f"eff {effs[-1]:.2f}")
        assert abs(res[7]["mse"][l] - mse) <= bound
    assert 2.0 <= float(np.mean(effs)) <= 12.0
    assert res[7]["sigma_data"] == 0.5


# ------------------------------------------------------------------ 9. the gap report
def test_gap_report(ops):
    import tinyedm_amd as T
    from oracle import edm_oracle as O
    from oracle.make_golden import tiny_cfgs
    from tinyedm_amd.evaluate import NoiseLevelEvaluator
    from tinyedm_amd.ideal import gap_report
    data = _train24()
    ideal = _ideal(data)
    train = ops.u8_gather_normalize(ideal.data, torch.arange(8, device=DEV), 0.5, 0.5)
    rng = np.random.default_rng(9)
    held = np.clip(data[:8].astype(np.int64) + rng.integers(-30, 31, data[:8].shape), 0, 255).astype(np.uint8)
    test = ops.u8_gather_normalize(torch.from_numpy(held).to(DEV), torch.arange(8, device=DEV), 0.5, 0.5)
    ecfg, dcfg = tiny_cfgs()
    P = O.init_params(ecfg, dcfg, torch.Generator().manual_seed(7))
    emb = T.Embedding(ecfg.fourier_dim, ecfg.embedding_dim, ecfg.num_classes, ecfg.add_factor)
    den = T.Denoiser(dcfg.in_channels, dcfg.out_channels, tuple(dcfg.encoder_block_types),
                     tuple(dcfg.decoder_block_types), tuple(dcfg.encoder_out_channels),
                     tuple(dcfg.decoder_out_channels), tuple(dcfg.skip_connections), 0.0, dcfg.sigma_data,
                     dcfg.encoder_add_factor, dcfg.decoder_add_factor, dcfg.embedding_dim, dcfg.num_heads)
    emb.load_state_dict({k[len("embedding."):]: v for k, v in P.items() if k.startswith("embedding.")})
    den.load_state_dict({k[len("denoiser."):]: v for k, v in P.items() if k.startswith("denoiser.")})
    model = T.EDM(diffuser=T.Diffuser(-1.2, 1.2), embedding=emb, denoiser=den, use_ema=False, use_uncertainty=False,
                  steady_steps=10, rampup_steps=10, scheduler_interval="step", lr=0.01).to(DEV).eval()
    ev = NoiseLevelEvaluator(num_levels=4, P_mean=-0.4, P_std=1.0, seed=1, batch_size=16)
    rep = gap_report(ev, ideal, train, test, model=model)
    L = 4
    assert len(rep["sigma"]) == L and rep["num_train"] == 8 and rep["num_references"] == 24
    for l in range(L):
        assert rep["ideal_train_mse"][l] <= rep["train_mse"][l]
        for k in ("to_ideal_train", "to_ideal_test"):
            assert np.isfinite(rep[k][l]) and rep[k][l] >= 0.0
        assert rep["excess_train"][l] == rep["train_mse"][l] - rep["ideal_train_mse"][l]
        assert rep["weighted"]["train_mse"][l] == rep["weight"][l] * rep["train_mse"][l]
        assert 1.0 <= rep["effective_count_train"][l] <= 24.0
    alone = gap_report(ev, ideal, train, test)
    assert "train_mse" not in alone and alone["ideal_train_mse"] == rep["ideal_train_mse"]
    # the ideal denoiser in the network's place is at distance zero from itself, exactly
    same = gap_report(ev, ideal, train, test, model=ideal)
    assert same["to_ideal_train"] == [0.0] * L and same["to_ideal_test"] == [0.0] * L
    assert same["excess_train"] == [0.0] * L and same["train_mse"] == same["ideal_train_mse"]
