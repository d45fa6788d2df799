"""numpy restatement of the ideal (empirical) denoiser of a training set (Karras et al. 2022, App. B.3, eq. 57),

    D*(x; sigma) = sum_i w_i y_i,   w = softmax_i(l_i),   l_i = -|x - y_i|^2 / (2 sigma^2),   y = (u / 255 - mean) / std,

in three forms: (a) "f64", the direct sum of squared differences in fp64 -- the truth; (b) "f32", the same in fp32;
(c) "f32x", fp32 in the expansion s.y - |y|^2 / (2 sigma^2) with s = x / sigma^2 (the query's own term, constant over i, is
added to lse alone).  The errors of (b) and (c) against (a) set the tolerance of a test case: tol = 8 max(err_b, err_c) + floor.
Also the chunked running merge of a softmax (max, sum, sum p (l - max)) that the kernels use, in fp64."""
import numpy as np

FORMS = ("f64", "f32", "f32x")


def normalize(u8, mean=0.5, std=0.5, dtype=np.float64):
    """uint8 [R, ...] -> [R, K] in dtype: (u / 255 - mean) / std"""
    u = np.asarray(u8)
    assert u.dtype == np.uint8
    dt = np.dtype(dtype).type
    return ((u.reshape(u.shape[0], -1).astype(dtype) / dt(255.0)) - dt(mean)) / dt(std)


def _softmax_stats(l, y, dt):
    """one query: logits l [R'] and rows y [R', K], both of type dt -> D, lse, entropy, top weight, top index (ties: lower)"""
    m = l.max()
    p = np.exp(l - m)
    s = p.sum(dtype=dt)
    w = p / s
    lse = m + np.log(s)
    nz = p > 0
    ent = np.log(s) - (p[nz] * (l[nz] - m)).sum(dtype=dt) / s           # lse - E_w[l]
    top = int(np.argmax(l))                                              # first of equal logits
    return w @ y, lse, ent, w[top], top


def ideal(x, sigma, data_u8, mean=0.5, std=0.5, form="f64", ref_labels=None, labels=None):
    """x [Q, ...], sigma scalar or [Q], data_u8 uint8 [R, ...] -> dict of D [Q, K], lse, entropy, effective_count,
    top_weight [Q] (all fp64 holding the values of the form's precision) and top_index [Q] (in data_u8's order).
    ref_labels [R] and labels [Q]: the softmax of query q runs over the references of class labels[q]."""
    assert form in FORMS
    dt = np.float64 if form == "f64" else np.float32
    y = normalize(data_u8, mean, std, dt)
    R, K = y.shape
    x = np.asarray(x).reshape(len(x), -1).astype(dt)
    Q = x.shape[0]
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (Q,)).astype(dt)
    out = {"D": np.zeros((Q, K)), "lse": np.zeros(Q), "entropy": np.zeros(Q), "top_weight": np.zeros(Q),
           "top_index": np.zeros(Q, dtype=np.int64)}
    yy = (y * y).sum(axis=1, dtype=dt) if form == "f32x" else None
    for q in range(Q):
        keep = np.arange(R) if labels is None else np.nonzero(np.asarray(ref_labels) == int(labels[q]))[0]
        yq = y[keep]
        s2 = sig[q] * sig[q]
        if form == "f32x":
            sx = x[q] / s2
            l = yq @ sx - dt(0.5) * yy[keep] / s2
            shift = dt(0.5) * (x[q] * x[q]).sum(dtype=dt) / s2
        else:
            d = x[q][None, :] - yq
            l = -(d * d).sum(axis=1, dtype=dt) / (dt(2.0) * s2)
            shift = dt(0.0)
        assert l.dtype == dt
        D, lse, ent, tw, ti = _softmax_stats(l, yq, dt)
        out["D"][q], out["lse"][q], out["entropy"][q], out["top_weight"][q] = D, lse - shift, ent, tw
        out["top_index"][q] = keep[ti]
    out["effective_count"] = np.exp(out["entropy"])
    return out


def log_density(lse, n_refs, K, sigma):
    """the exact log density (nats) of the noised empirical distribution: lse - log R' - K / 2 log(2 pi sigma^2)"""
    sigma = np.asarray(sigma, dtype=np.float64)
    return np.asarray(lse, dtype=np.float64) - np.log(np.asarray(n_refs, dtype=np.float64)) - 0.5 * K * np.log(
        2.0 * np.pi * sigma * sigma)


def chunked_merge(l, y, chunk):
    """the running merge of the kernels in fp64: logits l [R], rows y [R, K], chunks of `chunk` rows in order.  The state
    (m, s, t = sum p (l - m), acc = sum p y) is rescaled by alpha = exp(m - m') when the maximum moves:
    s' = alpha s + s_c, t' = alpha (t + (m - m') s) + t_c, acc' = alpha acc + acc_c.  -> (D, lse, entropy)"""
    l = np.asarray(l, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    m, s, t, acc = -np.inf, 0.0, 0.0, np.zeros(y.shape[1])
    for a in range(0, l.shape[0], chunk):
        lc, yc = l[a:a + chunk], y[a:a + chunk]
        m_new = max(m, lc.max())
        p = np.exp(lc - m_new)
        alpha, s_prev, t_prev = 0.0, 0.0, 0.0
        if m > -np.inf:
            alpha = np.exp(m - m_new)
            s_prev, t_prev = alpha * s, alpha * (t + (m - m_new) * s)
        nz = p > 0
        s, t = s_prev + p.sum(), t_prev + (p[nz] * (lc[nz] - m_new)).sum()
        acc = alpha * acc + p @ yc
        m = m_new
    return acc / s, m + np.log(s), np.log(s) - t / s


def clustered_u8(rng, R, shape, spread, bases=3):
    """soft test data: a few uniform random base images plus a uniform integer perturbation in [-spread, spread]"""
    base = rng.integers(0, 256, (bases,) + tuple(shape)).astype(np.int64)
    pick = rng.integers(0, bases, R)
    x = base[pick] + rng.integers(-spread, spread + 1, (R,) + tuple(shape))
    return np.clip(x, 0, 255).astype(np.uint8)
