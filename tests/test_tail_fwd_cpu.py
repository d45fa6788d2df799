"""The four identities behind the forward half of the factored output end (tests/tail_fwd_ref.py), in fp64 on the CPU,
against autograd of the dense composition conv3x3 + conv1x1 -> mp_add -> 1x1 output conv: relative 1e-10."""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_fwd_ref as T  # noqa: E402
import tail_lowrank_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 5, 7, 16, 24, 3), (2, 6, 4, 16, 16, 1), (2, 9, 33, 24, 48, 4)]      # B, H, W, C, Cc, Co


def _rel(x, ref):
    return ((x - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("has1", [True, False])
@pytest.mark.parametrize("B,H,W,C,Cc,Co", SHAPES)
def test_factored_equals_autograd(B, H, W, C, Cc, Co, has1):
    if not has1:
        Cc = C          # (a block without a 1x1 conv adds its input itself)
    g = torch.Generator().manual_seed(13)
    dd = dict(generator=g, dtype=torch.float64)
    a2 = torch.randn(B, C, H, W, **dd)
    cat = torch.randn(B, Cc, H, W, **dd).requires_grad_(True)
    W2 = torch.randn(C, C, 3, 3, **dd).requires_grad_(True)
    W1 = torch.randn(C, Cc, **dd).requires_grad_(True) if has1 else None
    Wout = torch.randn(Co, C, **dd).requires_grad_(True)
    dF = torch.randn(B, Co, H, W, **dd)
    tw = torch.randn(B, Cc, H, W, **dd)             # a second consumer of cat: its gradient is the dense part t
    a, b = 0.8, 0.6
    h = b * F.conv2d(a2, W2, padding=1) + a * (F.conv2d(cat, W1[:, :, None, None]) if has1 else cat)
    Fd = F.conv2d(h, Wout[:, :, None, None])
    loss = (Fd * dF).sum() + (cat * tw).sum()
    gs = torch.autograd.grad(loss, (cat, W2, Wout) + ((W1,) if has1 else ()))
    Wo, W2d, W1d, catd = Wout.detach(), W2.detach(), (W1.detach() if has1 else None), cat.detach()
    Wc, Wp = R.wc_from(Wo, W2d), T.wp_from(Wo, W1d)
    assert Wp.shape == (Co, Cc)
    assert _rel(T.fwd(a2, catd, Wc, Wp, b, a), Fd.detach()) <= 1e-10
    G, G1 = R.wgrad(dF, a2, 9), R.wgrad(dF, catd, 1)[:, 0]
    assert _rel(T.dwout(G, W2d, G1, W1d, b, a), gs[2]) <= 1e-10
    assert _rel(T.gcat(tw, dF, Wp, a), gs[0]) <= 1e-10
    assert _rel(R.expand_dw(Wo, G, b), gs[1]) <= 1e-10
    if has1:
        assert _rel(T.dw1(Wo, G1, a), gs[3]) <= 1e-10
        assert _rel(R.expand_dw(Wo, G1[:, None], a)[:, :, 0, 0], gs[3]) <= 1e-10      # = expand_slab with one tap


def test_entry_points_declared_and_bound():
    from tinyedm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    declared = set(re.findall(r"\b(edm_[a-z0-9_]+)\s*\(", hdr))
    for name in ("edm_lowrank_tail_supported", "edm_lowrank_tail_fwd", "edm_lowrank_tail_dwout_supported",
                 "edm_lowrank_tail_dwout", "edm_lowrank_gcat_supported", "edm_lowrank_gcat_add"):
        assert name in declared and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["edm_lowrank_tail_fwd"]) == 20 and len(_lib.SIGNATURES["edm_lowrank_gcat_add"]) == 12


def test_host_queries():
    from tinyedm_amd import ops
    assert ops.lowrank_tail_supported(256, 512, 3, 32) and ops.lowrank_tail_supported(64, 64, 3, 28)
    assert ops.lowrank_tail_supported(16, 24, 1, 7) and ops.lowrank_tail_supported(256, 512, 4, 32)
    assert not ops.lowrank_tail_supported(256, 512, 8, 32)          # 90 KB of tables
    assert not ops.lowrank_tail_supported(260, 512, 3, 32) and not ops.lowrank_tail_supported(256, 500, 3, 32)
    assert not ops.lowrank_tail_supported(256, 512, 9, 32)
    assert ops.lowrank_tail_dwout_supported(256, 512, 3, True) and ops.lowrank_tail_dwout_supported(64, 64, 3, False)
    assert not ops.lowrank_tail_dwout_supported(64, 128, 3, False)
    assert ops.lowrank_gcat_supported(512, 256, 3) and not ops.lowrank_gcat_supported(512, 260, 3)


def test_switch_default_on():
    import tinyedm_amd.networks as N
    assert N.TAIL_FWD is (os.environ.get("EDM_TAIL_FWD", "1") != "0")
    assert not N._tail_fwd_slot and not N._tail_slot
