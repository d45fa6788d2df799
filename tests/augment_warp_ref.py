"""numpy restatement of the continuous half of the non-leaking augmentation of csrc/data.hip
(edm_u8_gather_augment_warp_normalize; Karras et al. 2022, EDM, App. F.2: zoom, rotate, stretch, shift), evaluable in fp64
and in fp32.  The exact half (flip, xflip, yflip, translate, rot90) is tests/augment_ref.py; this file starts where it ends.

The transform of one channel plane S [H][W] in byte units ("Continuous augmentation"):
  S~(i)   = S(r), m = i mod 2 (n - 1) >= 0, r = m < n ? m : 2 (n - 1) - m          reflection without edge repeat
  U[u][v] = 2 sum_ij S~[i][j] h[u - 2 i + O] h[v - 2 j + O]                          up x2 (sym6 taps h, O = 5), any integers u, v
  V[u][v] = bilinear interpolation of U at q = Theta (u, v, 1)^T                     u in [-O, 2 H + 4], v in [-O, 2 W + 4]
  D[i][j] = 1/2 sum_uv V[u][v] h[u - 2 i + O] h[v - 2 j + O]                         down x2, the same taps as a correlation
  out     = ((D / 255) - mean) / std                                                 no clamp

Draws of sample b (same Philox key and TAG as augment_ref.draws, counter words it never reads):
  E' = philox((b, 32, TAG, epoch)): op i of WARP_OPS is enabled iff mask bit i is set and word i of E' < thr
  W0 = philox((b, 33, ...)), W1 = philox((b, 34, ...));  uni(w) = ((w >> 8) + 0.5) 2^-24;
  bm(a, b) = sqrt(-2 ln uni(a)) (cos, sin)(2 pi uni(b))
  zoom: n_s = bm(W0[0], W0[1]).cos, s = 2^(0.2 n_s);  rotate: theta = pi (2 uni(W0[2]) - 1);
  stretch: n_a = bm(W0[3], W1[0]).cos, phi = pi (2 uni(W1[1]) - 1), a = 2^(0.2 n_a);
  shift: (n_x, n_y) = bm(W1[2], W1[3]), t = (0.125 H n_y, 0.125 W n_x)
"""
import functools
import math

import numpy as np

import augment_ref as R

WARP_OPS = ("zoom", "rotate", "stretch", "shift")
DIM = 13
O = 5
TAPS = np.array([0.015404109327027373, 0.0034907120842174702, -0.11799011114819057, -0.048311742585633,
                 0.4910559419267466, 0.787641141030194, 0.3379294217276218, -0.07263752278646252,
                 -0.021060292512300564, 0.04472490177066578, 0.0017677118642428036, -0.007800708325034148])
CENTROID = float((np.arange(12) * TAPS).sum() / TAPS.sum() - O)        # 0.09826089954573...: where a 2x-grid sample sits
U32 = 2.0 ** -24
IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def mask_of(ops):
    return sum(1 << WARP_OPS.index(o) for o in ops)


def reflect(i, n):
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


# ------------------------------------------------------------------------------------------------ draws, labels, Theta
def uni(w):
    return ((int(w) >> 8) + 0.5) * U32


def bm(a, b):
    """-> (r cos, r sin, r)"""
    r = math.sqrt(-2.0 * math.log(uni(a)))
    ang = 2.0 * math.pi * uni(b)
    return r * math.cos(ang), r * math.sin(ang), r


def draws(b, H, W, p, mask, seed, epoch):
    """fp64 parameters of sample b -> dict(enabled=(4 bools), n_s, theta, n_a, phi, n_x, n_y, s, a, ty, tx, r=(r_s, r_a, r_t));
    a disabled op has its neutral parameters (its draws are made and ignored)"""
    thr = R.threshold(p)
    d = dict(enabled=(False,) * 4, n_s=0.0, theta=0.0, n_a=0.0, phi=0.0, n_x=0.0, n_y=0.0, r=(0.0, 0.0, 0.0))
    if thr != 0 and mask != 0:
        en = R._words(b, 32, R.TAG, epoch, seed)
        w0 = R._words(b, 33, R.TAG, epoch, seed)
        w1 = R._words(b, 34, R.TAG, epoch, seed)
        enabled = tuple(bool(mask >> i & 1) and en[i] < thr for i in range(4))
        ns, _, rs = bm(w0[0], w0[1])
        na, _, ra = bm(w0[3], w1[0])
        nx, ny, rt = bm(w1[2], w1[3])
        d["enabled"] = enabled
        d["r"] = (rs, ra, rt)
        if enabled[0]:
            d["n_s"] = ns
        if enabled[1]:
            d["theta"] = math.pi * (2.0 * uni(w0[2]) - 1.0)
        if enabled[2]:
            d["n_a"], d["phi"] = na, math.pi * (2.0 * uni(w1[1]) - 1.0)
        if enabled[3]:
            d["n_x"], d["n_y"] = nx, ny
    d["s"], d["a"] = 2.0 ** (0.2 * d["n_s"]), 2.0 ** (0.2 * d["n_a"])
    d["ty"], d["tx"] = 0.125 * H * d["n_y"], 0.125 * W * d["n_x"]
    return d


def labels(d):
    """fp64 [7]: (n_s, cos(theta) - 1, sin(theta), n_a cos(phi), n_a sin(phi), n_x, n_y); zeros for a disabled op"""
    return np.array([d["n_s"], math.cos(d["theta"]) - 1.0, math.sin(d["theta"]), d["n_a"] * math.cos(d["phi"]),
                     d["n_a"] * math.sin(d["phi"]), d["n_x"], d["n_y"]])


def label_tolerance(d):
    """64 u max(1, r) per column, r = sqrt(-2 ln uni) of the Box-Muller pair the column comes from (1 for the rotation)"""
    rs, ra, rt = d["r"]
    return 64 * U32 * np.array([max(1.0, rs), 1.0, 1.0, max(1.0, ra), max(1.0, ra), max(1.0, rt), max(1.0, rt)])


def rot(t):
    return np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]])


def forward_map(s=1.0, theta=0.0, a=1.0, phi=0.0):
    """F on (y, x) offsets: zoom by s, rotate by theta, stretch by a along phi and 1 / a across it"""
    return rot(phi) @ np.diag([a, 1.0 / a]) @ rot(-phi) @ rot(theta) * s


def p_src(H, W, py, px, s=1.0, theta=0.0, a=1.0, phi=0.0, ty=0.0, tx=0.0):
    """source position (y, x) of the output position (py, px): ctr + F^-1 (p_out - ctr - t)"""
    Fi = np.linalg.inv(forward_map(s, theta, a, phi))
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    dy, dx = py - cy - ty, px - cx - tx
    return cy + Fi[0, 0] * dy + Fi[0, 1] * dx, cx + Fi[1, 0] * dy + Fi[1, 1] * dx


def theta_matrix(H, W, s=1.0, theta=0.0, a=1.0, phi=0.0, ty=0.0, tx=0.0, c=CENTROID):
    """Theta [2][3] on the 2x grid: u -> 2 p_src((u - c) / 2) + c = k + F^-1 (u - k - 2 t), k = 2 ctr + c"""
    Fi = np.linalg.inv(forward_map(s, theta, a, phi))
    k = np.array([H - 1 + c, W - 1 + c])
    off = k - Fi @ (k + 2.0 * np.array([ty, tx]))
    return np.concatenate([Fi, off[:, None]], axis=1)


def theta_of(d, H, W):
    return theta_matrix(H, W, d["s"], d["theta"], d["a"], d["phi"], d["ty"], d["tx"])


# ------------------------------------------------------------------------------------------------ the three stages
def _up_matrix(n, taps):
    return _up_matrix_cached(n, taps.dtype.str, taps.tobytes())


def _down_matrix(n, taps):
    return _down_matrix_cached(n, taps.dtype.str, taps.tobytes())


@functools.lru_cache(maxsize=None)
def _up_matrix_cached(n, dtype, raw):
    """M [4 (n - 1)][n]: one period of U along an axis, U[u] = sum_r M[u][r] S[r] (without the factor 2 of the 2-d stage)"""
    taps = np.frombuffer(raw, dtype=dtype)
    period = 4 * (n - 1)
    M = np.zeros((period, n), dtype=taps.dtype)
    for u in range(period):
        for k in range(12):
            if (u + O - k) % 2 == 0:
                M[u, reflect((u + O - k) // 2, n)] += taps[k]
    return M


@functools.lru_cache(maxsize=None)
def _down_matrix_cached(n, dtype, raw):
    """G [n][2 n + 10]: D[i] = sum_a G[i][a] V[a - O]"""
    taps = np.frombuffer(raw, dtype=dtype)
    G = np.zeros((n, 2 * n + 10), dtype=taps.dtype)
    for i in range(n):
        G[i, 2 * i:2 * i + 12] = taps
    return G


def warp_plane(S, theta, dtype=np.float64, detail=False):
    """S [H][W] byte units, theta [2][3] -> D [H][W] byte units, every operation in `dtype`.
    detail=True -> (D, dict(L, max_q, abs_sum)): L the largest neighbour difference of U, max_q the largest |q| coordinate,
    abs_sum the three stages run on |S| with |h|: sum |weights * values| per output element"""
    H, W = S.shape
    taps = TAPS.astype(dtype)
    S = S.astype(dtype)
    th = np.asarray(theta).astype(dtype)
    uu = np.arange(-O, 2 * H + 5).astype(dtype)[:, None]
    vv = np.arange(-O, 2 * W + 5).astype(dtype)[None, :]
    qy = th[0, 0] * uu + th[0, 1] * vv + th[0, 2]
    qx = th[1, 0] * uu + th[1, 1] * vv + th[1, 2]
    y0, x0 = np.floor(qy), np.floor(qx)
    fy, fx = qy - y0, qx - x0
    one = dtype(1)
    y0, x0 = y0.astype(np.int64), x0.astype(np.int64)
    Gy, Gx = _down_matrix(H, taps), _down_matrix(W, taps)

    def stages(plane, My, Mx, Gy, Gx):
        U = dtype(2) * (My @ plane @ Mx.T)
        py, px = U.shape
        V = ((one - fy) * ((one - fx) * U[y0 % py, x0 % px] + fx * U[y0 % py, (x0 + 1) % px])
             + fy * ((one - fx) * U[(y0 + 1) % py, x0 % px] + fx * U[(y0 + 1) % py, (x0 + 1) % px]))
        return U, dtype(0.5) * (Gy @ V @ Gx.T)

    U, D = stages(S, _up_matrix(H, taps), _up_matrix(W, taps), Gy, Gx)
    if not detail:
        return D
    ataps = np.abs(TAPS)
    _, A = stages(np.abs(S).astype(np.float64), _up_matrix(H, ataps), _up_matrix(W, ataps), _down_matrix(H, ataps),
                  _down_matrix(W, ataps))
    L = max(np.abs(U - np.roll(U, 1, axis=0)).max(), np.abs(U - np.roll(U, 1, axis=1)).max())
    return D, dict(L=float(L), max_q=float(max(np.abs(qy).max(), np.abs(qx).max())), abs_sum=A)


def gamma(n):
    return n * U32 / (1 - n * U32)


def plane_bound(S, theta):
    """fp64 D and the a-priori bound of an fp32 evaluation of the three stages, both [H][W] in byte units:
    2 L delta (delta = 8 u max |q|: the fp32 coordinate moves the bilinear point) + gamma(256) sum |weights * values|"""
    D, info = warp_plane(S, theta, np.float64, detail=True)
    return D, 2.0 * info["L"] * 8 * U32 * info["max_q"] + gamma(256) * info["abs_sum"]


def normalize64(D, mean=0.5, std=0.5):
    return ((D / 255.0) - mean) / std


def batch(data, index, p, ops, warp_ops, flip, seed, epoch, mean=0.5, std=0.5, thetas=None):
    """data uint8 (N, C, H, W), index (B,) -> (x fp64 (B, C, H, W), bound fp64 (B, C, H, W) (0 on exact samples), aug fp64
    (B, 13), label tolerance (B, 13), Theta fp64 (B, 2, 3), exact draws list, warp draws list).  `thetas` (B, 6): the
    matrices to warp with instead of the fp64 ones (the kernel's own, so that the image check is not a coordinate check).
    Exact samples hold augment_ref's fp32 result; the bound of a warped one includes 3 u |result| for the final arithmetic."""
    _, C, H, W = data.shape
    mask, wmask = R.mask_of(ops), mask_of(warp_ops)
    B = len(index)
    x = np.zeros((B, C, H, W))
    bound = np.zeros((B, C, H, W))
    aug, tol, th = np.zeros((B, DIM)), np.zeros((B, DIM)), np.zeros((B, 2, 3))
    ds, wds = [], []
    for b, n in enumerate(np.asarray(index).tolist()):
        d = R.draws(b, H, W, p, mask, seed, epoch)
        wd = draws(b, H, W, p, wmask, seed, epoch)
        f = R.flip_bit(b, seed, epoch) if flip else 0
        exact = R.forward_image(data[n], d, f)
        aug[b, :6], aug[b, 6:] = R.labels(d, H, W), labels(wd)
        tol[b, 6:] = label_tolerance(wd)
        th[b] = theta_of(wd, H, W)
        if any(wd["enabled"]):
            use = th[b] if thetas is None else np.asarray(thetas[b], dtype=np.float64).reshape(2, 3)
            for c in range(C):
                D, bd = plane_bound(exact[c].astype(np.float64), use)
                x[b, c] = normalize64(D, mean, std)
                bound[b, c] = bd / 255.0 / abs(std) + 3 * U32 * np.abs(x[b, c])
        else:
            x[b] = R.normalize(exact, mean, std)
        ds.append(d)
        wds.append(wd)
    return x, bound, aug, tol, th, ds, wds
