"""The identity behind the factored output end, in fp64 on the CPU: the factored dgrad and both factored weight gradients
(tests/tail_lowrank_ref.py) equal autograd of conv2d followed by the 1x1 output conv -- tap flip and zero padding included.
This pins the reference the GPU tests compare the kernels with."""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_lowrank_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("B,H,W,C,Ci,Co", [(3, 5, 7, 6, 4, 3), (2, 8, 8, 8, 8, 4), (1, 1, 1, 8, 8, 3), (2, 1, 4, 5, 3, 1)])
def test_factored_equals_autograd(B, H, W, C, Ci, Co):
    g = torch.Generator().manual_seed(7)
    dd = dict(generator=g, dtype=torch.float64)
    a2 = torch.randn(B, Ci, H, W, **dd).requires_grad_(True)
    W2 = torch.randn(C, Ci, 3, 3, **dd).requires_grad_(True)
    Wout = torch.randn(Co, C, **dd).requires_grad_(True)
    dF = torch.randn(B, Co, H, W, **dd)
    b = 0.6
    h = b * F.conv2d(a2, W2, padding=1)
    Fout = F.conv2d(h, Wout[:, :, None, None])
    ga2, gW2, gWout = torch.autograd.grad((Fout * dF).sum(), (a2, W2, Wout))
    # the dense route of before: g_h = dF . Wout, then the full-rank transposed conv
    g_h = torch.einsum("bohw,oc->bchw", dF, Wout.detach())
    assert torch.allclose(F.conv_transpose2d(g_h, W2.detach(), padding=1) * b, ga2, rtol=1e-12, atol=1e-12)
    Wc = R.wc_from(Wout.detach(), W2.detach())
    assert Wc.shape == (Co, 9, Ci)
    assert torch.allclose(R.dgrad(dF, Wc, b), ga2, rtol=1e-11, atol=1e-11)
    G9 = R.wgrad(dF, a2.detach(), 9)
    assert G9.shape == (Co, 9, Ci)
    assert torch.allclose(R.expand_dw(Wout.detach(), G9, b), gW2, rtol=1e-11, atol=1e-11)
    G1 = R.wgrad(dF, h.detach(), 1)
    assert G1.shape == (Co, 1, C)
    assert torch.allclose(G1[:, 0], gWout, rtol=1e-11, atol=1e-11)


def test_tap_flip_is_not_optional():
    """an unflipped Wc (or a transposed tap order) must NOT reproduce the gradient: the check above can tell them apart"""
    g = torch.Generator().manual_seed(3)
    dd = dict(generator=g, dtype=torch.float64)
    W2, Wout, dF = torch.randn(4, 4, 3, 3, **dd), torch.randn(3, 4, **dd), torch.randn(1, 3, 4, 5, **dd)
    g_h = torch.einsum("bohw,oc->bchw", dF, Wout)
    ref = F.conv_transpose2d(g_h, W2, padding=1)
    Wc = R.wc_from(Wout, W2)
    assert torch.allclose(R.dgrad(dF, Wc), ref, rtol=1e-11, atol=1e-11)
    assert not torch.allclose(R.dgrad(dF, Wc.flip(1)), ref, rtol=1e-3, atol=1e-3)


def test_entry_points_declared_and_bound():
    from tinyedm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    declared = set(re.findall(r"\b(edm_[a-z0-9_]+)\s*\(", hdr))
    for name in ("edm_lowrank_df", "edm_lowrank_dgrad3x3", "edm_lowrank_wgrad", "edm_lowrank_wgrad_workspace",
                 "edm_lowrank_expand_wc", "edm_lowrank_expand_slab"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["edm_lowrank_dgrad3x3"]) == 23 and len(_lib.SIGNATURES["edm_lowrank_wgrad"]) == 14


def test_switch_default_on():
    import tinyedm_amd.networks as N
    assert N.TAIL_LOWRANK is (os.environ.get("EDM_TAIL_LOWRANK", "1") != "0")
    assert not N._tail_slot
