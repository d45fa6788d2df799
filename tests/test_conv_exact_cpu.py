"""The integer-operand recipes of tests/conv_exact_ref.py are exact: for every case tests/test_conv_exact_gpu.py runs, the
fp64 reference is representable in the kernel's output type and every partial sum stays below 2^24.  These are conditions
on the inputs, not tolerances; no GPU is needed (the plan queries are host logic of the library)."""
import pytest
import torch

import conv_exact_ref as X


def _shapes(cases):
    return sorted({(c[:6], c[7]) for c in cases}, key=str)


_FWD = _shapes(X.forward_cases())


@pytest.mark.parametrize("shape,imgs", _FWD, ids=["x".join(map(str, s)) for s, _ in _FWD])
def test_forward_operands_give_a_bf16_exact_reference(shape, imgs):
    c = X.conv_case(*shape, imgs)
    assert set(c.x.float().unique().tolist()) <= {-1.0, 0.0, 1.0} and set(c.wp.float().unique().tolist()) == {-1.0, 1.0}
    assert c.ref.abs().max().item() <= 128 and torch.equal(c.ref, c.ref.round())
    assert X.is_bf16_exact(c.ref) and X.is_bf16_exact(X.ALPHA * c.ref)
    assert (c.ref == 0).double().mean().item() < 0.2               # not a degenerate, mostly-zero output


def test_forward_cases_cover_what_the_issue_lists():
    cases = X.forward_cases()
    assert len(cases) == len(set(c[:8] for c in cases))
    for shape in X.CONV_SHAPES:
        for taps in (9, 1):
            assert {c[6] for c in cases if c[:6] == shape + (taps,)} == {0, 1, 2, 5, 6}
    for s in X.BORDER_SHAPES:
        for taps in (9, 1):
            assert {c[6] for c in cases if c[:6] == tuple(s[:5]) + (taps,)} == {0, 1, 2, 5, 6}
    assert X.DEGENERATE == [(3, 1, 1, 64, 64), (2, 2, 2, 64, 72), (1, 1, 16, 256, 64), (2, 3, 64, 64, 64), (1, 2, 33, 64, 64)]
    for s in X.DEGENERATE:
        assert {c[6] for c in cases if c[:5] == s} >= {0, 1, 2, 6}
    assert any(c[:5] == (32, 64, 64, 64, 256) and c[7] == (0, 17, 31) for c in cases)


def test_expected_kernels_are_what_the_plan_runs_when_forced():
    """conv_exact_ref.covers restates the kernels' covers-rules: for every forward, residual and descriptor case the kernel
    the table expects is the one edm_conv_plan names for the forced generation; every generation runs itself somewhere"""
    from tinyedm_amd import _lib
    plan = _lib.lib().edm_conv_plan
    shapes = {c[:6] for c in X.forward_cases()} | set(X.RESIDUAL_SHAPES) | {c[:6] for c in X.DESCRIPTOR_CASES}
    ran = set()
    for (B, H, W, Cin, Cout, taps) in shapes:
        for v in (1, 2, 5, 6):
            want = X.expected_kernel(v, W, Cin, taps)
            assert plan(B, H, W, Cin, Cout, taps, v) & 0xff == want, ((B, H, W, Cin, Cout, taps), v, want)
            ran.add((want, taps))
    assert ran >= {(1, 9), (2, 9), (5, 9), (6, 9), (1, 1), (2, 1)}
    for c in X.forward_cases():
        assert c[8] == X.expected_kernel(c[6], c[2], c[3], c[5])


@pytest.mark.parametrize("case", X.RESIDUAL_SHAPES + [c[:6] for c in X.DESCRIPTOR_CASES], ids=str)
def test_residual_form_stays_exact(case):
    c, r, ref = X.residual_case(*case)
    assert r.float().abs().max().item() <= X.RES_LIM and torch.equal(r.float(), r.float().round())
    assert ref.abs().max().item() <= 128 and torch.equal(2 * ref, (2 * ref).round()) and X.is_bf16_exact(ref)


@pytest.mark.parametrize("case", X.FOLD_SHAPES, ids=str)
def test_fold_operands_give_a_bf16_exact_reference(case):
    B, H, W, Cin, Cout, C2, imgs = case
    c = X.fold_case(B, H, W, Cin, Cout, C2, tuple(imgs))
    for a in (X.FOLD_A3, X.FOLD_A1):
        m, e = torch.frexp(torch.tensor(a))
        assert m.item() == 0.5                                      # a power of two
    assert c.ref.abs().max().item() <= 128 and torch.equal(2 * c.ref, (2 * c.ref).round()) and X.is_bf16_exact(c.ref)


def test_fold_shapes_use_the_smallest_batch_the_fold_supports():
    from tinyedm_amd import _lib
    assert len(X.FOLD_SHAPES) == len(X.FOLD_FULL_SHAPES)
    for (B, H, W, Cin, Cout, C2, imgs), full in zip(X.FOLD_SHAPES, X.FOLD_FULL_SHAPES):
        assert (H, W, Cin, Cout, C2) == tuple(full[1:6]) and B <= full[0]
        assert _lib.call("edm_conv3x3_fold_supported", B, H, W, Cin, Cout, C2)
        assert not _lib.call("edm_conv3x3_fold_supported", B - 1, H, W, Cin, Cout, C2)
        assert sorted(set(imgs)) == imgs and 0 <= imgs[0] and imgs[-1] == B - 1


@pytest.mark.parametrize("case", X.WGRAD_CASES + [s + (1, 1) for s in X.GROUP_1X1[-1:]], ids=str)
def test_weight_gradient_sums_stay_below_2_to_24(case):
    B, H, W = case[:3]
    c = X.wgrad_case(*case)
    assert c.x.float().abs().max().item() <= 2 and c.dy.float().abs().max().item() <= 2
    assert X.wgrad_sum_bound(B, H, W) < 2 ** 24
    assert c.ref.abs().max().item() <= X.wgrad_sum_bound(B, H, W) and torch.equal(c.ref, c.ref.round())
    assert torch.equal(c.ref, c.ref.float().double())


def test_weight_gradient_reference_is_the_definition():
    """wgrad_f64 (autograd of F.conv2d) against the sum written out, on a shape small enough to loop over"""
    B, H, W, Cin, Cout = 2, 3, 4, 5, 6
    c = X.wgrad_case(B, H, W, Cin, Cout, 9)
    x, dy = c.x.double(), c.dy.double()
    ref = torch.zeros(9, Cout, Cin, dtype=torch.float64)
    for t in range(9):
        for h in range(H):
            for w in range(W):
                hh, ww = h + t // 3 - 1, w + t % 3 - 1
                if 0 <= hh < H and 0 <= ww < W:
                    ref[t] += dy[:, h, w].t() @ x[:, hh, ww]
    assert torch.equal(c.ref, ref)
    c1 = X.wgrad_case(B, H, W, Cin, Cout, 1)
    assert torch.equal(c1.ref[0], torch.einsum("bhwo,bhwi->oi", c1.dy.double(), c1.x.double()))


def test_ksplit_groups_use_the_smallest_batch_that_still_splits():
    from tinyedm_amd import ops
    for name, orig in X.W3_SPLIT_GROUPS.items():
        shape = lambda kw, B: (B, kw["H"], kw["W"], kw["Cin"], kw["Cout"])
        ks0 = ops.wgrad3_plan_ksplit([shape(kw, kw["B"]) for kw in orig])
        small = X.W3_GROUPS[name]
        ks = ops.wgrad3_plan_ksplit([shape(kw, kw["B"]) for kw in small])
        assert [k > 1 for k in ks] == [k > 1 for k in ks0], (name, ks, ks0)          # the same layers split
        for kw0, kw, k in zip(orig, small, ks):
            assert {a: b for a, b in kw.items() if a != "B"} == {a: b for a, b in kw0.items() if a != "B"}
            if k > 1:
                assert kw["B"] == 1 or ops.wgrad3_plan_ksplit([shape(kw, kw["B"] - 1)]) == [1], (name, kw)
            else:
                assert kw["B"] == kw0["B"]


@pytest.mark.parametrize("name", sorted(X.W3_GROUPS))
def test_grouped_wgrad_layers_are_transparent_to_the_projection(name):
    """one-hot master rows: ss = 1 exactly, the integer gradient G below 2^24, and away from the 1.0 the fp64 autograd
    gradient through O.effective_weight is c0 * scale * G (to the fp32 roundings inside the oracle's normalisation)"""
    seen = set()
    for kw, L in zip(X.W3_GROUPS[name], X.w3_group(name)):
        key = tuple(sorted(kw.items()))
        if key in seen:
            continue
        seen.add(key)
        Cout, I = L.wm.shape[:2]
        n = I * 9
        rows = L.wm.view(Cout, n)
        assert torch.equal((rows * rows).sum(1), torch.ones(Cout)) and int(L.star.sum()) == Cout
        r = torch.arange(Cout)
        assert bool((rows[r, X.star_column(r, n)] == 1).all())
        assert torch.equal(L.G, L.G.round()) and L.G.abs().max().item() <= X.wgrad_sum_bound(kw["B"], kw["H"], kw["W"]) < 2 ** 24
        off = ~L.star
        want = L.c0 * L.scale * L.G + L.g0.double()
        assert ((L.ref - want)[off].abs() <= 2.0 ** -22 * (L.c0 * L.scale * L.G)[off].abs()).all()
        assert bool(((L.ref == L.g0.double()) | (L.G != 0))[off].all())
        if L.accumulate:      # the bound of the GPU test gives the accumulate's rounding its share only under this condition
            nz = (L.G != 0) & off
            assert (L.g0.double().abs()[nz] <= 5 * (L.c0 * L.scale * L.G).abs()[nz]).all()
        if L.perm is not None:
            assert sorted(L.perm.tolist()) == list(range(Cout))
