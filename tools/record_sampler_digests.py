"""Digests of the per-sample fp32 kernels (solver updates, likelihood, evaluation, adaptive and parallel solvers,
restoration, the guard and the training-step elementwise ops) at the smallest shapes at which they can go wrong.

Every case builds its inputs with numpy.random.default_rng(seed) in fp64 cast to fp32 (never torch's RNG), calls one
`ops` entry point and hashes the bytes of its output tensors in a fixed order.  Run on the GPU at a commit whose kernels
are the reference:
    python tools/record_sampler_digests.py [COMMIT [FILE]]
writes {"parent": COMMIT, "rows": [[case id, sha256], ...]} to FILE.  COMMIT is the 40-hex commit the library was built
from (default: git's HEAD), FILE defaults to tests/sampler_kernels_parent.json.  Every case is run twice and a row whose
two runs differ is refused.  tests/test_sampler_digests_gpu.py recomputes every row on later commits: a refactor of
these kernels must not move a bit."""
import hashlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tinyedm_amd import ops  # noqa: E402

OUT = os.path.join(ROOT, "tests", "sampler_kernels_parent.json")
BATCHES = (1, 3)
# 5: element path, one partial quad; 1024: exactly one chunk; 1028: a second chunk of one quad; 3072; 65540: the 64-chunk
# cap, so a workgroup takes a second trip of its stride loop
SIZES = (5, 1024, 1028, 3072, 65540)
WINDOWS = (1, 3)
TABLE_N = 6
# [C, H, W], scale, gray of the restoration operator: every block size, W % 4 != 0, the channel mean
RESTORE = (((3, 8, 8), 2, False), ((3, 8, 12), 4, True), ((2, 6, 6), 2, False), ((3, 16, 16), 8, False),
           ((3, 5, 7), 1, True))
T0, T1 = 2.5, 1.75


class Inputs:
    """fp32 device tensors from one numpy generator; off = 1 puts each on a view offset by one element (4 bytes off the
    16-byte alignment, which sends every kernel down its element path)"""

    def __init__(self, case_id, off, dev):
        self.rng = np.random.default_rng(zlib.crc32(case_id.encode()))
        self.off, self.dev = off, dev

    def place(self, a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        buf = torch.empty(t.numel() + self.off, dtype=t.dtype, device=self.dev)
        v = buf[self.off:].view(t.shape)
        v.copy_(t)
        return v

    def normal(self, *shape, scale=1.0):
        return self.place((scale * self.rng.standard_normal(shape)).astype(np.float32))

    def uniform(self, lo, hi, *shape):
        return self.place(self.rng.uniform(lo, hi, shape).astype(np.float32))

    def ints(self, lo, hi, shape, dtype):
        return torch.from_numpy(self.rng.integers(lo, hi, shape).astype(dtype)).to(self.dev)


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def _img(B, n):
    """[B, C, HW] of n elements per sample for inpaint_blend"""
    C = 3 if n % 3 == 0 else 1
    return (B, C, n // C)


def _per_sample_cases(B, n, off, dev):
    """(name, fn(inp) -> output tensors) over [B, n] operands"""
    w = lambda: torch.tensor([1.75], dtype=torch.float32, device=dev)        # noqa: E731
    rec = lambda: ops.churn_record(0x123456789ABCDEF0, 3, dev)               # noqa: E731
    zl = lambda rows=B: torch.zeros(rows, dtype=torch.float64, device=dev)   # noqa: E731
    K = 2
    E = (1 + 2 * K) * B

    def times(i):
        """per-sample (t, t1); the middle sample of a batch of three is inactive (t1 == t)"""
        t = i.rng.uniform(0.5, 3.0, B).astype(np.float32)
        t1 = (t * np.float32(0.75)).astype(np.float32)
        if B == 3:
            t1[1] = t[1]
        return i.place(t), i.place(t1)

    def adapt_control(i):
        state = ops.adapt_begin(B, 80.0, 0.002, -8.0, dev)
        if B == 3:
            ops.adapt_rows(state).status[1] = ops.ADAPT_DONE
        chunks = ops.adapt_chunks(n)
        part = torch.from_numpy(i.rng.uniform(0.0, 2.0 * n / chunks, (B, ops.NLL_MAX_CHUNKS))).to(dev)
        active = torch.zeros(1, dtype=torch.int32, device=dev)
        accept = ops.adapt_control(part, n, state, 0.002, active)
        return accept, state, active

    def adapt_correct(i):
        t, t1 = times(i)
        part = torch.zeros((B, ops.NLL_MAX_CHUNKS), dtype=torch.float64, device=dev)
        return ops.adapt_correct(i.normal(B, n), i.normal(B, n), i.normal(B, n), i.normal(B, n), t, t1, 1e-3, 1e-2,
                                 part=part)

    def eval_args(i):
        return (i.ints(0, 1 << 32, B, np.uint32), i.ints(0, 4, B, np.int32),
                torch.tensor([0.02, 0.5, 3.0, 80.0], dtype=torch.float32, device=dev), rec())

    def div_euler(i):
        L = zl()
        dx, E1 = ops.heun_euler_div(i.normal(E, n), i.normal(E, n), T0, T1, 0.01, 0.02, rec(), 7, L, num_probes=K)
        return dx, E1, L

    def div_correct(i, h_next):
        L = zl()
        out = ops.heun_correct_div(i.normal(E, n), i.normal(B, n), i.normal(E, n), i.normal(E, n), T0, T1, 0.02, rec(),
                                   7, L, num_probes=K, h_next=h_next)
        return out, L

    def dpm(i, H, guided):
        m_out = torch.empty((B, n), dtype=torch.float32, device=dev)
        hist = [i.normal(B, n) for _ in range(H)]
        out = ops.dpm_multistep(i.normal(B, n), i.normal(B, n), 0.4, 0.9, -0.35 if H >= 1 else 0.0,
                                0.05 if H >= 2 else 0.0, Dg=i.normal(B, n) if guided else None,
                                w_dev=w() if guided else None, m1=hist[0] if H >= 1 else None,
                                m2=hist[1] if H >= 2 else None, m_out=m_out)
        return out, m_out

    def blend(i, t):
        shape = _img(B, n)
        mask = i.ints(0, 2, (1 if t == 0.0 else B, shape[2]), np.uint8)
        return (ops.inpaint_blend(i.normal(*shape), i.normal(*shape), mask, t, rec(), 5),)

    cases = [
        ("heun_euler", lambda i: ops.heun_euler(i.normal(B, n), i.normal(B, n), T0, T1)),
        ("heun_correct", lambda i: (ops.heun_correct(i.normal(B, n), i.normal(B, n), i.normal(B, n), i.normal(B, n), T0,
                                                     T1),)),
        ("heun_euler_guided", lambda i: ops.heun_euler_guided(i.normal(B, n), i.normal(B, n), i.normal(B, n), w(), T0,
                                                              T1)),
        ("heun_correct_guided", lambda i: (ops.heun_correct_guided(i.normal(B, n), i.normal(B, n), i.normal(B, n),
                                                                   i.normal(B, n), i.normal(B, n), w(), T0, T1),)),
        ("heun_churn", lambda i: (ops.heun_churn(i.normal(B, n), 0.6, rec(), 5),)),
        ("state_init", lambda i: (ops.state_init(i.normal(B, n), T0),)),
        ("state_init_image", lambda i: (ops.state_init(i.normal(B, n), T0, image=i.normal(B, n)),)),
        ("inpaint_blend", lambda i: blend(i, T0)),
        ("inpaint_blend_t0", lambda i: blend(i, 0.0)),
        ("nll_probe", lambda i: (ops.nll_probe(i.normal(B, n), 0.01, rec(), 7, ev=1, num_probes=K),)),
        ("heun_euler_div", div_euler),
        ("heun_correct_div", lambda i: div_correct(i, None)),
        ("heun_correct_div_next", lambda i: div_correct(i, 0.015)),
        ("nll_prior", lambda i: (ops.nll_prior(i.normal(B, n), T0, zl()),)),
        ("eval_diffuse", lambda i: ops.eval_diffuse(i.normal(B, n), *eval_args(i))),
        ("eval_diffuse_classes", lambda i: ops.eval_diffuse_classes(i.normal(B, n), *eval_args(i), 3)),
        ("eval_sqerr", lambda i: (ops.eval_sqerr(i.normal(B, n), i.normal(B, n)),)),
        ("eval_sqerr_classes", lambda i: (ops.eval_sqerr_classes(i.normal(3 * B, n), i.normal(B, n), 3),)),
        ("scale_f32", lambda i: (ops.scale_f32(i.normal(B, n), 0.3),)),
        ("adapt_begin", lambda i: (ops.adapt_begin(B, 80.0, 0.002, -8.0, dev),)),
        ("adapt_euler", lambda i: ops.adapt_euler(i.normal(B, n), i.normal(B, n), *times(i))),
        ("adapt_correct", adapt_correct),
        ("adapt_control", adapt_control),
        ("adapt_commit", lambda i: (ops.adapt_commit(i.normal(B, n), i.normal(B, n), i.ints(0, 2, B, np.uint8)),)),
        ("dps_residual", lambda i: ops.dps_residual(i.normal(B, n), i.normal(B, n))),
        ("dps_update", lambda i: (ops.dps_update(i.normal(B, n), i.normal(B, n), i.uniform(0.5, 2.0, B), 0.7),)),
        ("diffuse", lambda i: ops.diffuse(i.normal(B, n), -1.2, 1.2, 0x0BADC0FFEE123457, 11)),
        ("weighted_mse_grad", lambda i: (ops.weighted_mse(i.normal(B, n), i.normal(B, n), i.uniform(0.1, 3.0, B), 0.5)[1],)),
    ]
    for H in (0, 1, 2):
        for guided in (False, True):
            cases.append((f"dpm_multistep_o{H + 1}{'_guided' if guided else ''}",
                          lambda i, H=H, guided=guided: dpm(i, H, guided)))
    return cases


def _picard_chain(B, n, P, heun, off, dev, case_id):
    """begin -> scan -> control -> slide on one window; one row per stage.  Of a batch of three, sample 1 has a single live
    position and sample 2 a window past the table's end (nothing live)."""
    N = TABLE_N
    i = Inputs(case_id, off, dev)
    table = np.array([80.0, 20.0, 5.0, 1.0, 0.2, 0.002], dtype=np.float32)
    t_table = torch.from_numpy(table).to(dev)
    X, T, state = ops.picard_begin(i.normal(B, n), t_table, N, P)
    rows = [("begin", digest((X, T, state)))]
    starts = np.array([0, N - 2, N - 1][:B], dtype=np.int32)
    ops.picard_rows(state).start.copy_(torch.from_numpy(starts))
    T.copy_(torch.from_numpy(table[np.minimum(starts[None, :] + np.arange(P + 1)[:, None], N - 1)]))
    X = i.normal(P + 1, B, n)
    dx = i.normal(P, B, n, scale=0.01)
    X1, D1 = (i.normal(P, B, n), i.normal(P, B, n)) if heun else (None, None)
    Xnew, part = ops.picard_scan(X, dx, X1, D1, T, state, 1.0, 0.5, N=N)
    rows.append(("scan", digest((Xnew, part))))
    active = torch.zeros(1, dtype=torch.int32, device=dev)
    err = torch.zeros((B, P), dtype=torch.float64, device=dev)
    stride = ops.picard_control(part, n, state, N, P, active, err=err)
    rows.append(("control", digest((stride, state, err, active))))
    Xs, Ts = ops.picard_slide(Xnew, i.normal(P, B, n), stride, state, t_table, N=N)
    rows.append(("slide", digest((Xs, Ts))))
    return rows


def _restore_cases(B, dev):
    w = lambda: torch.tensor([1.75], dtype=torch.float32, device=dev)        # noqa: E731
    cases = []
    for (C, H, W), scale, gray in RESTORE:
        tag = f"{C}x{H}x{W}_s{scale}{'g' if gray else ''}"
        ys = ops.measurement_shape((B, C, H, W), scale, gray)
        cases += [
            (f"degrade_{tag}", lambda i, s=(B, C, H, W), sc=scale, g=gray: (ops.degrade(i.normal(*s), sc, g),)),
            (f"project_denoised_{tag}", lambda i, s=(B, C, H, W), ys=ys, sc=scale, g=gray:
                (ops.project_denoised(i.normal(*s), i.normal(*ys), sc, g),)),
            (f"project_denoised_guided_{tag}", lambda i, s=(B, C, H, W), ys=ys, sc=scale, g=gray:
                (ops.project_denoised(i.normal(*s), i.normal(*ys), sc, g, Dg=i.normal(*s), w_dev=w()),)),
            (f"degrade_adjoint_{tag}", lambda i, ys=ys, C=C, sc=scale, g=gray:
                (ops.degrade_adjoint(i.normal(*ys), C, sc, g),)),
        ]
    for radius in (1, 4):
        cases.append((f"blur2d_r{radius}", lambda i, r=radius: (ops.blur2d(i.normal(B, 3, 9, 7),
                                                                           ops.gaussian_taps(1.3, r)),)))
    return cases


def _guard_case(off, dev, case_id):
    """grad_guard over an arena of tensors of the sizes above, 16 elements of padding between them"""
    i = Inputs(case_id, off, dev)
    offsets, pos = [], 0
    for s in SIZES:
        offsets.append(pos)
        pos += (s + 19) // 4 * 4
    grad = i.normal(pos, scale=1e-2)
    table = ops.grad_guard_table(offsets, SIZES, pos, dev)
    sumsq = torch.zeros(len(SIZES), dtype=torch.float64, device=dev)
    record = ops.guard_record(dev)
    ops.grad_guard(grad, table, sumsq, record, grad_scale=0.5, max_norm=1.0, clip_value=0.5, skip_nonfinite=True)
    return digest((sumsq, record))


def _adam_case(form, n, dev, case_id):
    """one optimizer pass over an arena of n elements in one of its four forms (every arena 16-byte aligned)"""
    i = Inputs(case_id, 0, dev)
    theta, grad, m, ema = (i.normal(n) for _ in range(4))
    v = i.uniform(0.0, 1.0, n)
    hyper = (1e-2, 0.9, 0.99, 1e-8, 3, 0.999)
    extra = []
    if form == "adam_ema":
        ops.adam_ema(theta, grad, m, v, ema, *hyper, grad_scale=0.5, zero_grad=True)
    elif form == "adam_ema_ranges":           # the arena but for one slice in its middle, which stays untouched
        ranges, chunks = ops.adam_ranges_table([(n // 3, n // 3)], n, dev)
        ops.adam_ema_ranges(theta, grad, m, v, ema, ranges, chunks, *hyper, grad_scale=0.5, zero_grad=True)
    elif form == "adam_ema_phema":
        extra = [i.normal(n), i.normal(n)]
        betas = torch.tensor([0.9, 0.99], dtype=torch.float32, device=dev)
        ops.adam_ema_phema(theta, grad, m, v, ema, extra, betas, *hyper, grad_scale=0.5, zero_grad=True)
    else:                                     # behind a guard record that clips the norm and the values
        table = ops.grad_guard_table([0], [n], n, dev)
        sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        record = ops.guard_record(dev)
        ops.grad_guard(grad, table, sumsq, record, grad_scale=0.5, max_norm=1.0, clip_value=0.05)
        ops.adam_ema_guarded(theta, grad, m, v, ema, record, *hyper, grad_scale=0.5, zero_grad=True)
        extra = [record]
    return digest([theta, grad, m, v, ema] + extra)


def compute(dev=None):
    """every (case id, sha256) row, in a fixed order"""
    dev = torch.device("cuda", 0) if dev is None else dev
    rows = []
    for off in (0, 1):
        al = "off1" if off else "al16"
        for B in BATCHES:
            for n in SIZES:
                for name, fn in _per_sample_cases(B, n, off, dev):
                    cid = f"{name}/B{B}/n{n}/{al}"
                    rows.append((cid, digest(fn(Inputs(cid, off, dev)))))
                for P in WINDOWS:
                    for heun in (False, True):
                        cid = f"picard_o{2 if heun else 1}/B{B}/n{n}/P{P}/{al}"
                        rows += [(f"{cid}/{stage}", d) for stage, d in _picard_chain(B, n, P, heun, off, dev, cid)]
            for name, fn in _restore_cases(B, dev):
                cid = f"{name}/B{B}/{al}"
                rows.append((cid, digest(fn(Inputs(cid, off, dev)))))
        rows.append((f"grad_guard/{al}", _guard_case(off, dev, f"grad_guard/{al}")))
    for form in ("adam_ema", "adam_ema_ranges", "adam_ema_phema", "adam_ema_guarded"):
        for n in SIZES:
            rows.append((f"{form}/n{n}", _adam_case(form, n, dev, f"{form}/n{n}")))
    ops.check_health(dev, "sampler digests")
    return rows


def main():
    first, second = compute(), compute()
    differ = [a[0] for a, b in zip(first, second) if a != b]
    if differ or len(first) != len(second):
        raise SystemExit(f"refusing to write: {len(differ)} rows differ between two runs, e.g. {differ[:5]}")
    if len(sys.argv) > 1:
        head = sys.argv[1]
    else:
        head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    if len(head) != 40 or any(c not in "0123456789abcdef" for c in head):
        raise SystemExit("refusing to write: pass the 40-hex commit the kernels were built from (no git checkout here)")
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    with open(out, "w") as f:
        json.dump({"parent": head, "rows": [list(r) for r in first]}, f, indent=0)
        f.write("\n")
    print(f"wrote {len(first)} rows for {head} to {out}")


if __name__ == "__main__":
    main()
