"""The algebra of csrc/attention_long.hip in fp64 (tests/attention_long_ref.py: fixed offset sqrt(d), 64-key tiles, masked
tail, stat, two-pass backward from stat and delta) against plain softmax autograd, to 1e-12 of the result's scale: the tiled
form is EXACT for pixel-normalised q and k, not an approximation.  The shapes are those of tests/test_attention_long_gpu.py."""
import math
import os

import pytest
import torch

import attention_long_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 17, 17, 1, 64), (2, 18, 18, 2, 64), (1, 24, 24, 1, 32), (1, 17, 17, 1, 144), (1, 20, 20, 1, 128),
          (1, 17, 17, 2, 192), (2, 32, 32, 1, 64), (1, 64, 64, 1, 64), (3, 16, 16, 2, 64)]
EXTREME = [(1, 32, 32, 1, 64), (1, 20, 20, 1, 192)]


def _check(q, k, v, gy):
    q, k, v = (R.pixel_norm(t).requires_grad_(True) for t in (q, k, v))
    d = q.shape[-1]
    s = q @ k.transpose(-1, -2) / math.sqrt(d)
    y_ref = torch.softmax(s, dim=-1) @ v
    y_ref.backward(gy)
    lse_ref = torch.logsumexp(s.detach(), dim=-1)
    with torch.no_grad():
        y, stat = R.forward(q, k, v)
        dq, dk, dv, delta = R.backward(q, k, v, y, gy, stat)

    def close(a, b, what):
        err, scale = (a - b).abs().max().item(), max(1.0, b.abs().max().item())
        assert err <= 1e-12 * scale, f"{what}: {err:.3e} (scale {scale:.3e})"

    close(y, y_ref.detach(), "y")
    close(stat, lse_ref, "stat")
    close(delta, (gy * y_ref.detach()).sum(-1), "delta")
    close(dq, q.grad, "dq")
    close(dk, k.grad, "dk")
    close(dv, v.grad, "dv")
    return s.detach()


@pytest.mark.parametrize("B,H,W,heads,hd", SHAPES)
def test_tiled_form_is_softmax_attention(B, H, W, heads, hd):
    g = torch.Generator().manual_seed(B + H + heads + hd)
    N = H * W
    q, k, v, gy = (torch.randn(B, heads, N, hd, generator=g, dtype=torch.float64) for _ in range(4))
    _check(q, k, v, gy)


@pytest.mark.parametrize("B,H,W,heads,hd", EXTREME)
def test_tiled_form_at_both_ends_of_the_fixed_offset(B, H, W, heads, hd):
    """k = q, second half of the tokens negated: logits +sqrt(d) and -sqrt(d) in every row, p from 1 down to exp(-2 sqrt(d))"""
    g = torch.Generator().manual_seed(hd)
    N = H * W
    q, k, v = R.extreme_qkv(B, heads, N, hd, g)
    gy = torch.randn(B, heads, N, hd, generator=g, dtype=torch.float64)
    s = _check(q, k, v, gy)
    assert s.max().item() > 0.999 * math.sqrt(hd) and s.min().item() < -0.999 * math.sqrt(hd)
    # the smallest probability the kernel forms is a normal fp32 and a normal bf16 (both have 8 exponent bits)
    assert math.exp(-2.0 * math.sqrt(192)) > 2.0 ** -126


def test_c_abi_declares_the_long_attention_entry_points():
    from tinyedm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tinyedm_hip.h")).read()
    for name, nargs in (("edm_attention_long_supported", 3), ("edm_attention_long_fwd", 8), ("edm_attention_long_bwd", 11)):
        assert f"int {name}(" in hdr and len(_lib.SIGNATURES[name]) == nargs
    assert "edm_attention_long_supported" in _lib._NO_STATUS       # returns 1 / 0, not a status
