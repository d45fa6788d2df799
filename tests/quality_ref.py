"""Plain numpy fp64 references of the paired image quality kernels (tinyedm_amd/csrc/quality.hip): SSIM by explicit
separable correlation over the valid region, the integer squared error, the region rules, the feature distance in the
two-pass form and the PSNR floor.  Nothing here imports the package under test."""
import numpy as np


def gaussian_taps(win, sigma):
    k = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return w / w.sum()


def filter_valid(x, w):
    """x fp64 [..., H, W] -> the separable correlation with the taps w over the valid region [..., H-win+1, W-win+1]:
    rows (along W) first, then columns, each an explicit sum over the taps in ascending order"""
    win = w.shape[0]
    H, W = x.shape[-2:]
    r = np.zeros(x.shape[:-1] + (W - win + 1,), dtype=np.float64)
    for k in range(win):
        r = r + w[k] * x[..., :, k:k + W - win + 1]
    c = np.zeros(x.shape[:-2] + (H - win + 1, W - win + 1), dtype=np.float64)
    for k in range(win):
        c = c + w[k] * r[..., k:k + H - win + 1, :]
    return c


def filter_valid_2d(x, w):
    """the same quantity by the brute-force 2-D outer-product window"""
    win = w.shape[0]
    H, W = x.shape[-2:]
    w2 = np.outer(w, w)
    out = np.zeros(x.shape[:-2] + (H - win + 1, W - win + 1), dtype=np.float64)
    for i in range(win):
        for j in range(win):
            out = out + w2[i, j] * x[..., i:i + H - win + 1, j:j + W - win + 1]
    return out


def ssim_map(a, b, w, L, filt=filter_valid):
    """a, b fp64 [..., H, W] in pixel units -> the SSIM map over the valid region (biased variances)"""
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    ma, mb = filt(a, w), filt(b, w)
    va = filt(a * a, w) - ma * ma
    vb = filt(b * b, w) - mb * mb
    cov = filt(a * b, w) - ma * mb
    return ((2.0 * ma * mb + c1) * (2.0 * cov + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))


def to_nchw(x):
    """uint8 [n, H, W, C] or float32 [n, C, H, W] -> fp64 [n, C, H, W]"""
    x = np.asarray(x)
    return (x.transpose(0, 3, 1, 2) if x.dtype == np.uint8 else x).astype(np.float64)


def pair_ssim(a, b, w, L, region=None):
    """-> (ssim fp64 [n, C], sse fp64 [n, C], counts int32 [n, 2]) by the rules of ops.pair_ssim: sse over the counted
    pixels, the SSIM mean over the valid centres that are themselves counted; no counted centre: NaN and a count of 0"""
    A, B = to_nchw(a), to_nchw(b)
    n, C, H, W = A.shape
    win = w.shape[0]
    half = (win - 1) // 2
    S = ssim_map(A, B, np.asarray(w, dtype=np.float64), float(L))
    if region is None:
        reg = np.ones((n, H, W), dtype=bool)
    else:
        reg = np.broadcast_to(np.asarray(region) != 0, (n, H, W))
    cen = reg[:, half:H - half, half:W - half]
    ssim = np.full((n, C), np.nan)
    sse = np.zeros((n, C))
    counts = np.zeros((n, 2), dtype=np.int32)
    for i in range(n):
        counts[i] = (int(reg[i].sum()), int(cen[i].sum()))
        for c in range(C):
            if np.asarray(a).dtype == np.uint8:
                d = np.asarray(a)[i, :, :, c].astype(np.int64) - np.asarray(b)[i, :, :, c].astype(np.int64)
                sse[i, c] = float(int((d * d)[reg[i]].sum()))
            else:
                d = A[i, c] - B[i, c]
                sse[i, c] = (d * d)[reg[i]].sum()
            if counts[i, 1]:
                ssim[i, c] = S[i, c][cen[i]].sum() / counts[i, 1]
    return ssim, sse, counts


def feature_distance(a, b):
    """a, b float32 [B, HW, C] (or [B, H, W, C]) -> fp64 [B]: (1/HW) sum_p sum_c (a/(|a_p| + 1e-10) - b/(|b_p| + 1e-10))^2,
    the norms first, then the squared differences of the scaled values"""
    A = np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1, a.shape[-1])
    B = np.asarray(b, dtype=np.float64).reshape(A.shape)
    na = np.sqrt((A * A).sum(axis=2, keepdims=True)) + 1e-10
    nb = np.sqrt((B * B).sum(axis=2, keepdims=True)) + 1e-10
    d = A / na - B / nb
    return (d * d).sum(axis=(1, 2)) / A.shape[1]


def psnr(sse, count, L):
    """-10 log10 of the MSE in [0, 1] pixel units, floored at 1e-12 (identical images: 120 dB)"""
    mse = np.asarray(sse, dtype=np.float64) / (np.asarray(count, dtype=np.float64) * float(L) ** 2)
    return -10.0 * np.log10(np.maximum(mse, 1e-12))
