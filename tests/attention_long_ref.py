"""fp64 restatement of the tiled cosine attention of csrc/attention_long.hip, step for step: fixed offset sqrt(d) instead of a
running maximum, key tiles of 64 whose rows past N are zeros AND masked to p = 0, stat = sqrt(d) + log sum p, and the two-pass
backward that recomputes P = exp(s - stat) -- query-major for dQ and delta = <dO, y>, key-major (blocks of 128 keys, query
tiles of 64) for dK and dV.  Operands are the pixel-normalised q, k, v of networks.py:195, shape [..., N, d].

tests/test_attention_long_cpu.py checks it against plain softmax autograd; the GPU tests take their log-sum-exp from here."""
import math

import torch

TILE = 64      # rows per streamed tile
BLOCK = 128    # rows a workgroup owns


def _tile(x, t0):
    """rows [t0, t0 + TILE) of x [..., N, d], zero rows past N (what the kernel stages), and the mask of the real rows"""
    N = x.shape[-2]
    out = x.new_zeros(*x.shape[:-2], TILE, x.shape[-1])
    n = max(0, min(TILE, N - t0))
    out[..., :n, :] = x[..., t0:t0 + n, :]
    return out, torch.arange(TILE) < n


def forward(q, k, v):
    """-> y [..., N, d], stat [..., N]"""
    N, d = q.shape[-2:]
    off, scale = math.sqrt(d), 1.0 / math.sqrt(d)
    l = q.new_zeros(q.shape[:-1])
    acc = torch.zeros_like(q)
    for t0 in range(0, N, TILE):
        kt, real = _tile(k, t0)
        vt, _ = _tile(v, t0)
        p = torch.exp(q @ kt.transpose(-1, -2) * scale - off)
        p = p * real            # a zero key has s = 0, p = exp(-sqrt(d)) != 0: masked
        l += p.sum(-1)
        acc += p @ vt
    return acc / l[..., None], off + torch.log(l)


def backward(q, k, v, y, gy, stat):
    """-> dq, dk, dv, delta"""
    N, d = q.shape[-2:]
    scale = 1.0 / math.sqrt(d)
    delta = (gy * y).sum(-1)
    # query-major pass
    dq = torch.zeros_like(q)
    for t0 in range(0, N, TILE):
        kt, real = _tile(k, t0)
        vt, _ = _tile(v, t0)
        p = torch.exp(q @ kt.transpose(-1, -2) * scale - stat[..., None]) * real
        ds = p * (gy @ vt.transpose(-1, -2) - delta[..., None])
        dq += ds @ kt * scale
    # key-major pass: rows of a query tile past N carry stat = +huge (p = 0) and delta = 0
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    for b0 in range(0, N, BLOCK):
        kb, vb = k[..., b0:b0 + BLOCK, :], v[..., b0:b0 + BLOCK, :]
        for t0 in range(0, N, TILE):
            qt, real = _tile(q, t0)
            gt, _ = _tile(gy, t0)
            n = int(real.sum())
            st = stat.new_full((*stat.shape[:-1], TILE), 1e30)
            dl = stat.new_zeros(*stat.shape[:-1], TILE)
            st[..., :n], dl[..., :n] = stat[..., t0:t0 + n], delta[..., t0:t0 + n]
            p = torch.exp(qt @ kb.transpose(-1, -2) * scale - st[..., None])       # [queries of the tile, keys of the block]
            ds = p * (gt @ vb.transpose(-1, -2) - dl[..., None])
            dv[..., b0:b0 + BLOCK, :] += p.transpose(-1, -2) @ gt
            dk[..., b0:b0 + BLOCK, :] += ds.transpose(-1, -2) @ qt * scale
    return dq, dk, dv, delta


def pixel_norm(x, eps=1e-4):
    """networks.py:9-14 over the last dim"""
    return x / (eps + x.norm(dim=-1, keepdim=True) / math.sqrt(x.shape[-1]))


def extreme_qkv(B, heads, N, d, generator, dtype=torch.float64):
    """raw q, k, v [B, heads, N, d] whose logits reach both ends of the fixed offset: every token's q and k are one vector
    per (sample, head), negated for the second half of the tokens, so that s = +sqrt(d) within a half and -sqrt(d) across
    the halves; v is random"""
    base = torch.randn(B, heads, 1, d, generator=generator, dtype=dtype)
    sign = torch.ones(N, 1, dtype=dtype)
    sign[N // 2:] = -1.0
    qk = base * sign
    return qk.clone(), qk.clone(), torch.randn(B, heads, N, d, generator=generator, dtype=dtype)
