"""numpy fp64 restatement of the guarded optimizer step (csrc/grad_guard.hip): the chunk table, the per-tensor and total
sums of squares of fp32(g) * grad_scale, the non-finite rule, the clip coefficient and the guarded Adam + EMA update.
Written from the formulas of the issue (torch.nn.utils.clip_grad_norm_ / clip_grad_value_), not from the kernels."""
import math

import numpy as np

BIG = 3.0e38


BLOCK = 1024            # elements per partial sum, counted from a tensor's first element


def chunk_table(offsets, numels, n, chunk):
    """(chunks [(tensor, first, len)], tensors [(first chunk, count, first block, blocks)]): tensor p is tiled by
    consecutive chunks of at most `chunk` elements and owns ceil(numel / BLOCK) consecutive partial-sum blocks; refuses
    slices that overlap or leave [0, n)"""
    spans = sorted((int(o), int(c)) for o, c in zip(offsets, numels) if int(c) > 0)
    pos = 0
    for o, c in spans:
        if o < pos or o + c > n:
            raise ValueError(f"slice ({o}, {c}) overlaps another or leaves the arena of {n}")
        pos = o + c
    chunks, tensors, blocks = [], [], 0
    for p, (o, c) in enumerate(zip(offsets, numels)):
        first = len(chunks)
        done = 0
        while done < c:
            length = min(chunk, c - done)
            chunks.append((p, o + done, length))
            done += length
        tensors.append((first, len(chunks) - first, blocks, -(-c // BLOCK)))
        blocks += -(-c // BLOCK)
    return chunks, tensors


def scaled64(g32, grad_scale):
    """fp32(g) * fp32(grad_scale) as an exact fp64 product (24 + 24 significand bits)"""
    return np.asarray(g32, dtype=np.float32).astype(np.float64) * float(np.float32(grad_scale))


def sumsq(arena32, offsets, numels, grad_scale):
    """(per-tensor fp64 sums of squares, their total): math.fsum, i.e. correctly rounded sums of the fp64 squares"""
    with np.errstate(all="ignore"):     # (squares are >= 0: fsum never meets inf - inf)
        per = np.array([math.fsum((scaled64(arena32[o:o + c], grad_scale) ** 2).tolist()) for o, c in zip(offsets, numels)],
                       dtype=np.float64)
        return per, math.fsum(per.tolist())


def nonfinite(arena32, offsets, numels, grad_scale):
    """an element of a tensor (not of the padding) is NaN, or |g| or |fp32(g * grad_scale)| exceeds 3e38"""
    gs = np.float32(grad_scale)
    with np.errstate(all="ignore"):
        for o, c in zip(offsets, numels):
            g = np.asarray(arena32[o:o + c], dtype=np.float32)
            if (~(np.abs(g) <= BIG)).any() or (~(np.abs(g * gs) <= BIG)).any():
                return True
    return False


def coef(total, max_norm):
    """(norm, coef) in fp64: coef = min(1, max_norm / (norm + 1e-6)), exactly 1 with max_norm off (None / inf)"""
    norm = math.sqrt(total) if total == total and total >= 0 else float("nan")
    if max_norm is None or math.isinf(max_norm):
        return norm, 1.0
    c = float(np.float32(max_norm)) / (norm + 1e-6)
    return norm, (1.0 if c >= 1.0 else c)


def guarded_adam64(theta, g, m, v, ema, *, lr, b1, b2, eps, bc1, bc2sqrt, ema_beta, scale, clip_value=None, profiles=(),
                   profile_betas=()):
    """tests/test_fused_opt_gpu.py adam64 with `scale` (= fp32(grad_scale * coef)) on the gradient and every scaled element
    limited to +-clip_value; all operands fp64 arrays holding fp32 values.  -> theta, m, v, ema, [profiles]"""
    gj = g * scale
    if clip_value is not None and not math.isinf(clip_value):
        gj = np.clip(gj, -clip_value, clip_value)
    m = b1 * m + (1 - b1) * gj
    v = b2 * v + (1 - b2) * gj * gj
    theta = theta - (lr / bc1) * m / (np.sqrt(v) / bc2sqrt + eps)
    ema = ema_beta * ema + (1 - ema_beta) * theta
    return theta, m, v, ema, [pb * p + (1 - pb) * theta for p, pb in zip(profiles, profile_betas)]
