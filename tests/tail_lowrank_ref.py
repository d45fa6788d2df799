"""fp64 restatement of the factored output end (tinyedm_amd/csrc/tail_lowrank.hip), pure torch.

conv_out maps C channels to Co: its input gradient g_h[p, c] = sum_o dF[p, o] Wout[o, c] has rank Co per pixel.  With
h = b * conv3x3(a2, W2) (zero padding 1, cross-correlation: h[p] = b sum_t W2[:, :, t] a2[p + d(t)], t = 3 ky + kx,
d(t) = (ky - 1, kx - 1)) in front of it:

    ga2[p, ci]    = b sum_t sum_o dF[p - d(t), o] Wc[o, t, ci]       Wc[o, t, ci] = sum_c Wout[o, c] W2[c, ci, t]
    dW2[c, ci, t] = b sum_o Wout[o, c] G9[o, t, ci]                  G9[o, t, ci] = sum_p dF[p, o] a2[p + d(t), ci]
    dWout[o, c]   = G1[o, 0, c]                                      G1[o, 0, c]  = sum_p dF[p, o] h[p, c]

Layouts are the kernels': dF (B, Co, H, W), activations (B, C, H, W) here (NCHW for torch), Wc (Co, 9, C), G (Co, taps, C).
tests/test_tail_lowrank_cpu.py pins these against autograd; the GPU tests compare the kernels with them."""
import torch
import torch.nn.functional as F


def wc_from(Wout, W2):
    """Wout (Co, C), W2 (C, Ci, 3, 3) -> Wc (Co, 9, Ci)"""
    C, Ci = W2.shape[:2]
    return torch.einsum("oc,cit->oti", Wout, W2.reshape(C, Ci, 9))


def _shift(x, dy, dx):
    """y[..., r, s] = x[..., r + dy, s + dx], zero outside the image"""
    H, W = x.shape[-2:]
    xp = F.pad(x, (1, 1, 1, 1))
    return xp[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def dgrad(dF, Wc, b=1.0):
    """ga2 (B, Ci, H, W) = b sum_t sum_o dF[p - d(t), o] Wc[o, t, ci]"""
    out = 0
    for ky in range(3):
        for kx in range(3):
            out = out + torch.einsum("bohw,oi->bihw", _shift(dF, -(ky - 1), -(kx - 1)), Wc[:, ky * 3 + kx])
    return b * out


def wgrad(dF, X, taps):
    """G (Co, taps, C) = sum_p dF[p, o] X[p + d(t), c]"""
    if taps == 1:
        return torch.einsum("bohw,bchw->oc", dF, X)[:, None]
    return torch.stack([torch.einsum("bohw,bchw->oc", dF, _shift(X, ky - 1, kx - 1)) for ky in range(3) for kx in range(3)], 1)


def wgrad_abs(dF, X, taps):
    """sum of |terms| of wgrad: the scale of its fp32 summation error"""
    return wgrad(dF.abs(), X.abs(), taps)


def expand_dw(Wout, G, b=1.0):
    """dW (C, Ci, 3, 3) = b sum_o Wout[o, c] G[o, t, ci]"""
    Co, taps, Ci = G.shape
    k = 3 if taps == 9 else 1
    return b * torch.einsum("oc,oti->cit", Wout, G).reshape(Wout.shape[1], Ci, k, k)
