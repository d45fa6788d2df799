"""The adaptive solver restated in numpy, fp64 by default, for any callable D(x, t) with x [B, ...] and t [B]: the
embedded Heun(2) / Euler(1) pair with local extrapolation, the snap rule, the error norm, the step controller and the
counters of tinyedm_amd.AdaptiveSolver (csrc/adaptive.hip), sample by sample.  No GPU, no torch.

``dtype`` is the format the state (x and the per-sample t, t1, h) is STORED in: np.float64 is the reference proper,
np.float32 mirrors what the device keeps.  Every expression is evaluated in fp64 either way."""
from typing import NamedTuple

import numpy as np

ACTIVE, DONE, FAILED = 0, 1, 2


class Controller(NamedTuple):
    safety: float = 0.9
    fac_min: float = 0.2
    fac_max: float = 5.0
    h_floor: float = 1e-6


def snap(t, h, t_end, dtype=np.float64):
    """the trial time of a step h from t: t + h, or t_end exactly when t + h passes it or comes within 1 % of |h|"""
    tn = np.float64(t) + np.float64(h)
    passes = tn >= t_end if h > 0 else tn <= t_end
    close_by = abs(np.float64(t_end) - tn) <= 0.01 * abs(np.float64(h))
    return dtype(t_end) if (passes or close_by) else dtype(tn)


def error_norm(x, x1, y, atol, rtol):
    """E per sample: sqrt(mean_j ((y_j - x1_j) / (atol + rtol max(|x_j|, |y_j|)))^2), fp64"""
    x, x1, y = (np.asarray(v, dtype=np.float64).reshape(len(v), -1) for v in (x, x1, y))
    r = (y - x1) / (atol + rtol * np.maximum(np.abs(x), np.abs(y)))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((r * r).sum(axis=1) / x.shape[1])


class Row(NamedTuple):
    """one sample's controller state"""
    t: float
    t1: float
    h: float
    status: int = ACTIVE
    accepted: int = 0
    rejected: int = 0
    after_reject: bool = False
    err: float = 0.0


def control(row: Row, E, t_end, c: Controller = Controller(), dtype=np.float64):
    """one controlled step of one sample: (accept, the new row).  A sample that is not active is returned unchanged."""
    if row.status != ACTIVE:
        return False, row
    E = np.float64(E)
    ok = bool(E <= 1.0)                                     # (a NaN rejects)
    top = 1.0 if (not ok or row.after_reject) else c.fac_max
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.float64(c.safety) / np.sqrt(E)
    if not f >= c.fac_min:                                  # (a NaN lands here)
        f = np.float64(c.fac_min)
    if f > top:
        f = np.float64(top)
    h = dtype((np.float64(row.t1) - np.float64(row.t)) * f)
    t, status = row.t, ACTIVE
    accepted, rejected = row.accepted, row.rejected
    if ok:
        t = row.t1
        accepted += 1
        if t == dtype(t_end):
            status = DONE
    else:
        rejected += 1
    if status == ACTIVE and not abs(np.float64(h)) >= c.h_floor * abs(np.float64(t)):
        status = FAILED
    t1 = snap(t, h, t_end, dtype) if status == ACTIVE else t
    return ok, Row(t, t1, h, status, accepted, rejected, not ok, dtype(E))


def begin(B, t_start, t_end, h0, dtype=np.float64):
    return [Row(dtype(t_start), snap(dtype(t_start), dtype(h0), t_end, dtype), dtype(h0)) for _ in range(B)]


class Result(NamedTuple):
    x: np.ndarray
    accepted: np.ndarray
    rejected: np.ndarray
    iterations: int
    evaluations: int
    status: np.ndarray
    t: np.ndarray
    trace: list             # per iteration: (t [B] before, accept [B], E [B], x before as a copy or None)


def integrate(D, x, t_start, t_end, h0, *, rtol=1e-3, atol=1e-4, max_iterations=1024, controller=Controller(),
              dtype=np.float64, keep_states=False) -> Result:
    """x from t_start to t_end, every sample at its own pace; D(x, t) is called with the whole batch, twice an iteration"""
    x = np.array(x, dtype=dtype)
    B = x.shape[0]
    shape = (B,) + (1,) * (x.ndim - 1)
    rows = begin(B, t_start, t_end, h0, dtype)
    trace, iterations, evaluations = [], 0, 0
    while any(r.status == ACTIVE for r in rows) and iterations < max_iterations:
        t = np.array([r.t for r in rows], dtype=np.float64)
        t1 = np.array([r.t1 for r in rows], dtype=np.float64)
        live = (t1 != t).reshape(shape)
        X = x.astype(np.float64)
        dx = np.where(live, (X - np.asarray(D(X, t), dtype=np.float64)) / t.reshape(shape), 0.0)
        x1 = np.where(live, X + (t1 - t).reshape(shape) * dx, X).astype(dtype).astype(np.float64)
        dp = (x1 - np.asarray(D(x1, t1), dtype=np.float64)) / t1.reshape(shape)
        y = np.where(live, X + (t1 - t).reshape(shape) * (0.5 * dx + 0.5 * dp), X).astype(dtype).astype(np.float64)
        evaluations += 2
        E = error_norm(X, x1, y, atol, rtol)
        accept = np.zeros(B, dtype=bool)
        for b in range(B):
            accept[b], rows[b] = control(rows[b], E[b], t_end, controller, dtype)
        trace.append((t, accept.copy(), E, x.copy() if keep_states else None))
        x = np.where(accept.reshape(shape), y, X).astype(dtype)
        iterations += 1
    return Result(x, np.array([r.accepted for r in rows]), np.array([r.rejected for r in rows]), iterations, evaluations,
                  np.array([r.status for r in rows]), np.array([r.t for r in rows], dtype=np.float64), trace)


def solve(D, x0, span, **kw) -> Result:
    """AdaptiveSolver.solve: span = (sigma_max, sigma_min, h0 < 0); the state starts at sigma_max * x0 and ends with the
    closing Euler step sigma_min -> 0, which returns D itself up to rounding"""
    t_start, t_end, h0 = span
    r = integrate(D, np.asarray(x0, dtype=np.float64) * t_start, t_start, t_end, h0, **kw)
    X = r.x.astype(np.float64)
    te = np.full(X.shape[0], t_end, dtype=np.float64)
    out = X + (0.0 - t_end) * ((X - np.asarray(D(X, te), dtype=np.float64)) / t_end)
    return r._replace(x=out.astype(r.x.dtype), evaluations=r.evaluations + 1)


def invert(D, image, span, **kw) -> Result:
    """AdaptiveSolver.invert: span = (sigma_min, sigma_max, h0 > 0); returns the unit-scale latent x / sigma_max"""
    t_start, t_end, h0 = span
    r = integrate(D, image, t_start, t_end, h0, **kw)
    return r._replace(x=(r.x.astype(np.float64) / t_end).astype(r.x.dtype))
