"""numpy fp64 restatement of the schedule search (tinyedm_amd/schedule.py, csrc/schedule.hip): the Heun trace of a
denoiser callable, the pair step errors written as their definition (no Gram identity), the step costs, the
dynamic-programming path and a brute-force enumerator of all paths for small grids.  Also the two analytic denoisers and
the setting of tests/test_adaptive_solver_cpu.py (d = 48, B = 8, torch.manual_seed(0)), restated for the tests here."""
import itertools

import numpy as np
import torch

D_, B_ = 48, 8
MIX_S, MIX_W = 0.1, (0.1, 0.2, 0.3, 0.4)


# ------------------------------------------------------------------ the analytic denoisers
def setting():
    """torch.manual_seed(0)'s stream: the mixture's means, then x0 ~ N(0, I), both fp64"""
    g = torch.Generator().manual_seed(0)
    means = 0.5 * torch.randn(4, D_, generator=g, dtype=torch.float64)
    x0 = torch.randn(B_, D_, generator=g, dtype=torch.float64)
    return means.numpy(), x0.numpy()


def gaussian(x, t):
    """the posterior mean for data ~ N(0, 0.25 I)"""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    return 0.25 / (0.25 + t * t) * x


def mixture(means):
    logw = np.log(np.array(MIX_W))

    def D(x, t):
        """the posterior mean E[y | y + t n = x] of the 4-component mixture"""
        v = MIX_S ** 2 + np.asarray(t, dtype=np.float64).reshape(-1, 1) ** 2
        d = x[:, None, :] - means[None]
        logp = logw[None] - 0.5 * (d * d).sum(-1) / v - 0.5 * means.shape[1] * np.log(v)
        p = np.exp(logp - logp.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        return (p[:, :, None] * (means[None] + (MIX_S ** 2 / v)[:, :, None] * d)).sum(axis=1)
    return D


# ------------------------------------------------------------------ tables and the Heun solve
def karras_table(num_steps, sigma_min=0.002, sigma_max=80.0, rho=7.0):
    """the N non-zero levels of the Karras table, fp64"""
    i = np.arange(num_steps, dtype=np.float64)
    return (sigma_max ** (1 / rho) + i / (num_steps - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho


def heun_trace(D, x0, sigmas):
    """Heun on the table ``sigmas`` (N non-zero levels; the closing 0 is appended) from sigmas[0] * x0: returns
    (x [N + 1, B, d], slope [N, B, d], tau [N + 1]), node i the state at t_i, slope i the Euler slope (x_i - D) / t_i"""
    tau = np.append(np.asarray(sigmas, dtype=np.float64), 0.0)
    N, B = len(tau) - 1, len(x0)
    xs, ss = [tau[0] * np.asarray(x0, dtype=np.float64)], []
    for i in range(N):
        x, t0, t1 = xs[-1], tau[i], tau[i + 1]
        dx = (x - D(x, np.full(B, t0))) / t0
        x1 = x + (t1 - t0) * dx
        if i < N - 1:
            dp = (x1 - D(x1, np.full(B, t1))) / t1
            x1 = x + (t1 - t0) * (0.5 * dx + 0.5 * dp)
        ss.append(dx)
        xs.append(x1)
    return np.stack(xs), np.stack(ss), tau


def heun_solve(D, x0, sigmas):
    return heun_trace(D, x0, sigmas)[0][-1]


# ------------------------------------------------------------------ the costs
def pair_step_errors(X, S, tau, order):
    """d2 [B, G, G + 1] by the definition: for i < j, h = tau[j] - tau[i],
    e = x_i + h s_i - x_j (order 1, and order 2 at j == G) or x_i + (h/2)(s_i + s_j) - x_j; d2 = sum_k e_k^2; 0 for j <= i"""
    X, S, tau = (np.asarray(a, dtype=np.float64) for a in (X, S, tau))
    G, B = S.shape[0], S.shape[1]
    X, S = X.reshape(G + 1, B, -1), S.reshape(G, B, -1)
    d2 = np.zeros((B, G, G + 1))
    for i in range(G):
        for j in range(i + 1, G + 1):
            h = tau[j] - tau[i]
            if order == 2 and j < G:
                e = X[i] + (h / 2) * (S[i] + S[j]) - X[j]
            else:
                e = X[i] + h * S[i] - X[j]
            d2[:, i, j] = (e * e).sum(axis=1)
    return d2


def pair_step_magnitudes(X, S, tau, order):
    """sum_k (|x_i| + |h||s_i| [+ |h/2||s_j|] + |x_j|)^2 per entry (with |h/2| on s_i too for the trapezoid): what the
    rounding error of d2 is measured against"""
    X, S = np.abs(np.asarray(X, dtype=np.float64)), np.abs(np.asarray(S, dtype=np.float64))
    tau = np.asarray(tau, dtype=np.float64)
    G, B = S.shape[0], S.shape[1]
    X, S = X.reshape(G + 1, B, -1), S.reshape(G, B, -1)
    m2 = np.zeros((B, G, G + 1))
    for i in range(G):
        for j in range(i + 1, G + 1):
            h = abs(tau[j] - tau[i])
            if order == 2 and j < G:
                m = X[i] + (h / 2) * (S[i] + S[j]) + X[j]
            else:
                m = X[i] + h * S[i] + X[j]
            m2[:, i, j] = (m * m).sum(axis=1)
    return m2


def step_costs(d2):
    """cost[i, j] = (1/B) sum_b sqrt(d2[b, i, j]), the samples added in index order; inf where j <= i"""
    d2 = np.asarray(d2, dtype=np.float64)
    B, G = d2.shape[0], d2.shape[1]
    acc = np.zeros((G, G + 1))
    for b in range(B):
        acc += np.sqrt(d2[b])
    cost = acc / B
    cost[np.tril_indices(G, 0, G + 1)] = np.inf
    return cost


# ------------------------------------------------------------------ the path
def best_path(cost, num_steps):
    """the path 0 -> G-1 of exactly N - 1 segments with the least summed cost (added along the path), ties to the smaller
    predecessor, plus the closing segment G-1 -> G: (indices of the N nodes, total)"""
    cost = np.asarray(cost, dtype=np.float64)
    G, N = cost.shape[0], int(num_steps)
    if cost.shape != (G, G + 1) or not 2 <= N <= G:
        raise ValueError(f"best_path: needs a [G, G + 1] cost and 2 <= num_steps <= G, got {cost.shape}, {num_steps}")
    f = np.full((N, G), np.inf)
    prev = np.zeros((N, G), dtype=np.int64)
    f[0, 0] = 0.0
    for m in range(1, N):
        for j in range(1, G):
            best, arg = np.inf, 0
            for i in range(j):
                c = f[m - 1, i] + cost[i, j]
                if c < best:
                    best, arg = c, i
            f[m, j], prev[m, j] = best, arg
    idx, j = [G - 1], G - 1
    for m in range(N - 1, 0, -1):
        j = int(prev[m, j])
        idx.append(j)
    return idx[::-1], float(f[N - 1, G - 1] + cost[G - 1, G])


def path_cost(cost, indices):
    """the cost of a path through ``indices`` (ending at G - 1) plus the closing segment, added along the path"""
    G = cost.shape[0]
    total = 0.0
    for a, b in zip(indices[:-1], indices[1:]):
        total = total + cost[a, b]
    return float(total + cost[G - 1, G])


def brute_force(cost, num_steps):
    """the least path_cost over every increasing path 0 -> G-1 with N nodes, and the paths that attain it"""
    G, N = cost.shape[0], int(num_steps)
    best, arg = np.inf, []
    for mid in itertools.combinations(range(1, G - 1), N - 2):
        idx = [0, *mid, G - 1]
        c = path_cost(cost, idx)
        if c < best:
            best, arg = c, [idx]
        elif c == best:
            arg.append(idx)
    return best, arg


def even_path(G, num_steps):
    """the evenly subsampled path, the N-step Karras table on a G-node Karras grid; None unless (G-1) % (N-1) == 0"""
    if (G - 1) % (num_steps - 1):
        return None
    s = (G - 1) // (num_steps - 1)
    return [k * s for k in range(num_steps)]
