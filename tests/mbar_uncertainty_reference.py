"""Float64 numpy yardstick of the MBAR Gram pass, the asymptotic covariance and the Newton step (upside_hip_mbar_gram of
include/upside_engine_c.h; mbar.gram, covariance, free_energy_uncertainty, expectation, profile and solver='newton'), written from
the definitions on top of tests/mbar_reference.py: the whole N x M weight matrix at once, G = W.T @ W, and the covariance by eq. D8 of
Shirts & Chodera 2008 with the N x N pseudo-inverse -- not the product's D9, which works on the M x M Gram matrix.  Nothing is
shared with csrc/.

    W[n, k]     = exp(f_k - u_k(n) - D_n),  k < K;     W[n, K + j] = exp(log_columns[j, n])
    Theta       = W^T (I_N - W N W^T)^+ W,             N = diag(n_k, 0, ..., 0)                       (D8)
    var(f_i - f_j) = Theta_ii + Theta_jj - 2 Theta_ij
    Newton:     g = N_k (1 - c_k),  H = diag(N_k c_k) - N G N  over the states with samples but the first;  f += solve(H, g)
"""
import numpy as np
import mbar_reference as M


def energies(case):
    v = case['values']
    if v is None:
        v = np.zeros((len(case['energy']), 0), 'f4')
    return M.reduced_energy(v, case['energy'], case['beta'], case['rows'], case['periods'])


def weights(u, n_k, f, log_columns=None):
    """(W (N, K + n_extra), D (N,))"""
    D = M.denominators(u, n_k, f)
    W = np.exp(np.asarray(f, 'f8')[None, :] - u - D[:, None])
    if log_columns is not None:
        with np.errstate(divide='ignore'):
            W = np.concatenate((W, np.exp(np.asarray(log_columns, 'f8').reshape(-1, len(u)).T)), axis=1)
    return W, D


def padded_counts(n_k, m):
    n = np.zeros(m)
    n[:len(n_k)] = np.asarray(n_k, 'f8')
    return n


def inner_pinv(W, n_k):
    """(I_N - W N W^T)^+ of eq. D8, N x N.  Only the columns with samples enter it, so one inverse serves every set of explicit
    columns.  The matrix is symmetric with eigenvalues in [0, 1]; the eigenvalue 0 belongs to the constant shift of every f.
    Eigenvalues below 1e-10 are taken as that null space (an eigenvalue of a 4000 x 4000 matrix carries about 1e-12; the smallest
    other eigenvalue of the cases here is above 1e-4)."""
    n = padded_counts(n_k, W.shape[1])
    A = np.eye(len(W)) - (W * n[None, :]) @ W.T
    return np.linalg.pinv(0.5 * (A + A.T), rcond=1e-10, hermitian=True)


def theta_d8(W, n_k, P=None):
    """eq. D8 with the N x N pseudo-inverse P = inner_pinv(W, n_k) (computed here if not given)"""
    if P is None:
        P = inner_pinv(W, n_k)
    return W.T @ P @ W


def pair_variance(theta):
    d = np.diag(theta)
    return d[:, None] + d[None, :] - 2. * theta


def newton_step(u, n_k, f):
    """(f after one Newton step, max |g| before it)"""
    n_k = np.asarray(n_k, 'f8')
    W, _ = weights(u, n_k, f)
    c = W.sum(axis=0); G = W.T @ W
    free = np.flatnonzero(n_k > 0)[1:]
    g = n_k * (1. - c)
    H = np.diag(n_k[free] * c[free]) - n_k[free, None] * G[np.ix_(free, free)] * n_k[None, free]
    out = np.array(f, 'f8')
    if len(free):
        out[free] += np.linalg.solve(H, g[free])
    return out, float(np.abs(g[n_k > 0]).max())


def solve(u, n_k, tol=1e-13, n_sc=3, max_step=50):
    """converged f by [n_sc iterations, then one iteration and one Newton step in turn]; ends on an iteration"""
    f = np.zeros(u.shape[1])
    for _ in range(n_sc):
        f, _ = M.iterate(u, n_k, f)
    for _ in range(max_step):
        fn, _ = M.iterate(u, n_k, f)
        delta = float(np.abs(fn - f).max())
        f = fn
        if delta < tol:
            return f
        f, _ = newton_step(u, n_k, f)
    raise RuntimeError('the yardstick solver did not converge')


def target_log_weights(case, u, n_k, f, target):
    """normalised log-weights of the samples in the target (beta_t, row_t or None)"""
    beta_t, row_t = target
    v = case['values']
    d = 0 if v is None else np.asarray(v).shape[1]
    if v is None:
        v = np.zeros((len(u), 0), 'f4')
    row = np.zeros((1, 3 * d)) if row_t is None else np.asarray(row_t, 'f8').reshape(1, 3 * d)
    ut = M.reduced_energy(v, case['energy'], [beta_t], row, case['periods'])[:, 0]
    x = -ut - M.denominators(u, n_k, f)
    return x - M.logsumexp(x, axis=0)


def expectation(u, n_k, f, log_w, A, P=None):
    """(mean (m,), variance (m,)) of the observables A (N, m) under the weights exp(log_w), by the augmented columns"""
    A = np.asarray(A, 'f8').reshape(len(u), -1)
    shift = A.min(axis=0) - 1.
    Ap = A - shift
    w = np.exp(log_w)
    mean_p = (w[:, None] * Ap).sum(axis=0)
    cols = np.concatenate((log_w[None, :], (log_w[:, None] + np.log(Ap / mean_p)).T))
    W, _ = weights(u, n_k, f, cols)
    th = theta_d8(W, n_k, P)
    K = u.shape[1]; t = K; a = K + 1 + np.arange(A.shape[1])
    return mean_p + shift, mean_p ** 2 * (th[a, a] + th[t, t] - 2. * th[a, t])


def bin_index(x, edges):
    e = np.asarray(edges, 'f8')
    b = np.full(len(x), -1)
    for i in range(len(e) - 1):
        last = i == len(e) - 2
        b[(x >= e[i]) & ((x <= e[i + 1]) if last else (x < e[i + 1]))] = i
    return b


def profile(u, n_k, f, log_w, x, edges, kT, P=None):
    """(F, variance of F_b - F_r relative to the lowest bin r) over the bins of edges (the last one closed); an empty bin: +inf, nan"""
    b = bin_index(np.asarray(x, 'f8'), edges)
    w = np.exp(log_w)
    nb = len(edges) - 1
    p = np.array([w[b == i].sum() for i in range(nb)])
    full = np.flatnonzero(p > 0)
    with np.errstate(divide='ignore'):
        F = -kT * np.log(p)
    cols = np.full((len(full), len(x)), -np.inf)
    for j, i in enumerate(full):
        cols[j, b == i] = log_w[b == i] - np.log(p[i])
    W, _ = weights(u, n_k, f, cols)
    th = theta_d8(W, n_k, P)
    K = u.shape[1]; idx = K + np.arange(len(full)); r = idx[np.argmin(F[full])]
    var = np.full(nb, np.nan)
    var[full] = kT ** 2 * (th[idx, idx] + th[r, r] - 2. * th[idx, r])
    return F, var


def emptied(case, windows=(2, 5)):
    """the case with the samples of the given windows taken out and their counts set to 0 (the windows stay as states)"""
    n_k = np.asarray(case['n_k']).copy()
    start = np.concatenate(([0], np.cumsum(n_k)))
    keep = np.ones(int(n_k.sum()), bool)
    for w in windows:
        keep[start[w]:start[w + 1]] = False
        n_k[w] = 0
    out = dict(case, n_k=n_k)
    out['values'] = None if case['values'] is None else case['values'][keep]
    out['energy'] = None if case['energy'] is None else case['energy'][keep]
    return out


def extra_columns(n, n_extra, seed, with_zero=True):
    """seeded log-columns (n_extra, n), each normalised to sum 1; with_zero puts -inf (weight 0) into a third of the first one"""
    rng = np.random.RandomState(seed)
    x = rng.normal(0., 1.5, (n_extra, n))
    if with_zero and n_extra and n > 2:
        x[0, rng.choice(n, n // 3, replace=False)] = -np.inf
    return x - M.logsumexp(x, axis=1)[:, None]
