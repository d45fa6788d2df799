"""fp64 restatement of the forward half of the factored output end (tinyedm_amd/csrc/tail_lowrank.hip).

The last decoder block ends in h = b * conv3x3(a2, W2) + a * conv1x1(cat, W1) (zero padding 1, cross-correlation, t = 3 ky + kx,
d(t) = (ky - 1, kx - 1)) and conv_out reduces h to Co channels at once, F = Wout . h.  With Wc (tail_lowrank_ref.wc_from)
and Wp[o, cj] = sum_c Wout[o, c] W1[c, cj] (Wp = Wout when the block has no 1x1 conv: W1 = identity):

    F[p, o]      = b sum_t sum_ci a2[p + d(t), ci] Wc[o, t, ci]  +  a sum_cj cat[p, cj] Wp[o, cj]
    dWout[o, c]  = b sum_{t, ci} W2[c, ci, t] G[o, t, ci]  +  a sum_cj W1[c, cj] G1[o, cj]
    g_cat[p, cj] = t[p, cj] + a sum_o dF[p, o] Wp[o, cj]              (t: the part of the gradient that reaches cat otherwise)
    dW1[c, cj]   = a sum_o Wout[o, c] G1[o, cj]

G = wgrad(dF, a2, 9), G1 = wgrad(dF, cat, 1)[:, 0].  Layouts as tail_lowrank_ref: activations NCHW here, dF (B, Co, H, W).
tests/test_tail_fwd_cpu.py pins the four against autograd of the dense composition; the GPU tests compare the kernels with
them."""
import torch

import tail_lowrank_ref as R


def wp_from(Wout, W1=None):
    """Wout (Co, C), W1 (C, Cc) or None -> Wp (Co, Cc)"""
    return Wout if W1 is None else Wout @ W1


def fwd(a2, cat, Wc, Wp, b, a):
    """F (B, Co, H, W)"""
    out = 0
    for ky in range(3):
        for kx in range(3):
            out = out + torch.einsum("bihw,oi->bohw", R._shift(a2, ky - 1, kx - 1), Wc[:, ky * 3 + kx])
    return b * out + a * torch.einsum("bjhw,oj->bohw", cat, Wp)


def fwd_abs(a2, cat, Wc, Wp, b, a):
    """sum of |terms| of fwd: the scale of its fp32 summation error"""
    return fwd(a2.abs(), cat.abs(), Wc.abs(), Wp.abs(), abs(b), abs(a))


def dwout(G, W2, G1, W1, b, a):
    """G (Co, 9, Ci), W2 (C, Ci, 3, 3), G1 (Co, Cc), W1 (C, Cc) or None -> dWout (Co, C)"""
    C, Ci = W2.shape[:2]
    first = b * torch.einsum("cit,oti->oc", W2.reshape(C, Ci, 9), G)
    return first + a * (G1 if W1 is None else G1 @ W1.t())


def gcat(t, dF, Wp, a):
    """t (B, Cc, H, W), dF (B, Co, H, W), Wp (Co, Cc) -> g_cat (B, Cc, H, W)"""
    return t + a * torch.einsum("bohw,oj->bjhw", dF, Wp)


def dw1(Wout, G1, a):
    """Wout (Co, C), G1 (Co, Cc) -> dW1 (C, Cc)"""
    return a * Wout.t() @ G1
