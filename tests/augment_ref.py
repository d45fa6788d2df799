"""numpy restatement of the non-leaking augmentation of csrc/data.hip (edm_u8_gather_augment_normalize; Karras et al. 2022,
EDM, App. F.2 -- exact subset: xflip, yflip, whole-pixel translation with a reflected border, rot90).

Two descriptions of the same transform live here: `forward_image` applies the ops one after the other with np.flip,
np.pad(mode="reflect") + a slice and np.rot90; `inverse_index` is the composed inverse index map the kernel evaluates per
output element, written once.  tests/test_augment_cpu.py checks them against each other; the GPU tests compare the kernel
with `forward_image`.

Word -> draw mapping (the header comment of aug_draw in csrc/data.hip), per sample b of a launch (seed, epoch):
  E   = philox((b, 0, TAG, epoch), seed): op i of OPS is enabled iff mask bit i is set and word i of E < thr
  D_j = philox((b, 1 + j, TAG, epoch), seed): xflip bit = D_0[0] & 1, yflip bit = (D_0[0] >> 1) & 1, k = (D_0[0] >> 2) & 3;
        sx = u(D_j[1], 2 (W // 8) + 1) - W // 8, sy = u(D_j[2], 2 (H // 8) + 1) - H // 8 with u(word, n) = word % n of the
        first j whose word < (2^32 // n) * n (rejection: unbiased), the TRIES-th word unconditionally.
"""
import numpy as np

from likelihood_ref import philox4x32_10

OPS = ("xflip", "yflip", "translate", "rot90")
TAG = 0x41554731
FLIP_TAG = 0x0DA7          # the unlabelled left-right flip of edm_u8_gather_normalize
TRIES = 16
ROT_LABELS = ((0.0, 0.0), (-1.0, 1.0), (-2.0, 0.0), (-1.0, -1.0))     # (cos(k pi/2) - 1, sin(k pi/2))


def threshold(p):
    """round(p * 2^32) clamped to [0, 2^32] (ops.label_drop_threshold)"""
    return min(max(int(round(float(p) * 4294967296.0)), 0), 1 << 32)


def mask_of(ops):
    return sum(1 << OPS.index(o) for o in ops)


def unbiased(words, n):
    """first word of `words` below (2^32 // n) * n, reduced mod n; the TRIES-th word is taken whatever it is"""
    lim = (1 << 32) // n * n
    for j, w in enumerate(words):
        if int(w) < lim or j == TRIES - 1:
            return int(w) % n
    raise ValueError("ran out of words")


def _words(b, c1, tag, epoch, seed):
    return [int(v) for v in philox4x32_10(b, c1, tag, epoch, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)]


def draws(b, H, W, p, mask, seed, epoch):
    """-> dict(xflip, yflip, sx, sy, k, enabled=(4 bools)) of sample b"""
    thr = threshold(p)
    out = dict(xflip=0, yflip=0, sx=0, sy=0, k=0, enabled=(False,) * 4)
    if thr == 0 or mask == 0:
        return out
    en = _words(b, 0, TAG, epoch, seed)
    enabled = tuple(bool(mask >> i & 1) and en[i] < thr for i in range(4))
    cache = {}

    def D(j):
        if j not in cache:
            cache[j] = _words(b, 1 + j, TAG, epoch, seed)
        return cache[j]

    if enabled[0]:
        out["xflip"] = D(0)[0] & 1
    if enabled[1]:
        out["yflip"] = (D(0)[0] >> 1) & 1
    if enabled[2]:
        out["sx"] = unbiased((D(j)[1] for j in range(TRIES)), 2 * (W // 8) + 1) - W // 8
        out["sy"] = unbiased((D(j)[2] for j in range(TRIES)), 2 * (H // 8) + 1) - H // 8
    if enabled[3]:
        out["k"] = (D(0)[0] >> 2) & 3
    out["enabled"] = enabled
    return out


def flip_bit(b, seed, epoch):
    return _words(b, 0, FLIP_TAG, epoch, seed)[0] & 1


def labels(d, H, W):
    """fp32 [6]: (xflip, yflip, sx / W, sy / H, cos(k pi/2) - 1, sin(k pi/2)), one fp32 divide each"""
    return np.array([d["xflip"], d["yflip"], np.float32(d["sx"]) / np.float32(W), np.float32(d["sy"]) / np.float32(H),
                     ROT_LABELS[d["k"]][0], ROT_LABELS[d["k"]][1]], dtype=np.float32)


def forward_image(img, d, flip=0):
    """img (C, H, W): flip (unlabelled), xflip, yflip, translate, rot90 -- the ops one after the other, in numpy"""
    C, H, W = img.shape
    x = img
    if flip:
        x = np.flip(x, axis=2)
    if d["xflip"]:
        x = np.flip(x, axis=2)
    if d["yflip"]:
        x = np.flip(x, axis=1)
    Mh, Mw = H // 8, W // 8
    if Mh or Mw:
        pad = np.pad(x, ((0, 0), (Mh, Mh), (Mw, Mw)), mode="reflect")
        x = pad[:, Mh - d["sy"]:Mh - d["sy"] + H, Mw - d["sx"]:Mw - d["sx"] + W]     # positive shift: content moves right / down
    else:
        assert d["sx"] == 0 and d["sy"] == 0
    if d["k"]:
        x = np.rot90(x, d["k"], axes=(1, 2))
    return np.ascontiguousarray(x)


def inverse_index(H, W, d, flip=0):
    """(src_i, src_j) int arrays [H, W]: output pixel (i, j) reads input pixel (src_i, src_j) -- the kernel's per-element
    chain: rot90 backwards, translate backwards with one reflection, yflip, then xflip XOR flip"""
    h, w = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    k = d["k"]
    if k == 0:
        i, j = h, w
    elif k == 1:
        i, j = w, W - 1 - h
    elif k == 2:
        i, j = H - 1 - h, W - 1 - w
    else:
        i, j = W - 1 - w, h
    i = i - d["sy"]
    i = np.where(i < 0, -i, np.where(i >= H, 2 * (H - 1) - i, i))
    j = j - d["sx"]
    j = np.where(j < 0, -j, np.where(j >= W, 2 * (W - 1) - j, j))
    if d["yflip"]:
        i = H - 1 - i
    if bool(d["xflip"]) != bool(flip):
        j = W - 1 - j
    return i, j


def normalize(u8, mean=0.5, std=0.5):
    """the byte -> float arithmetic of k_u8_gather_normalize: separately rounded fp32 /255, - mean, / std"""
    x = u8.astype(np.float32) / np.float32(255.0)
    return (x - np.float32(mean)) / np.float32(std)


def batch(data, index, p, ops, flip, seed, epoch, mean=0.5, std=0.5):
    """data uint8 (N, C, H, W), index (B,) -> (x fp32 (B, C, H, W), aug fp32 (B, 6), draws list) through forward_image"""
    _, C, H, W = data.shape
    mask = mask_of(ops)
    xs, ls, ds = [], [], []
    for b, n in enumerate(np.asarray(index).tolist()):
        d = draws(b, H, W, p, mask, seed, epoch)
        f = flip_bit(b, seed, epoch) if flip else 0
        xs.append(normalize(forward_image(data[n], d, f), mean, std))
        ls.append(labels(d, H, W))
        ds.append(d)
    return np.stack(xs), np.stack(ls), ds
