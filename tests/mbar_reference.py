"""Float64 numpy yardstick of MBAR over umbrella and temperature ladders (the statement of upside_hip_mbar in
include/upside_engine_c.h), written from the definitions: the whole N x K matrix of reduced energies at once, every logsumexp as
max + log(sum(exp(x - max))) along an axis.  Nothing is tiled and nothing is shared with csrc/kernels_mbar.hip.  Pinned on cases
with known answers by tests/test_mbar_config.py.

    u_k(n) = beta_k (E_n + sum_c 1/2 k_kc max(0, |wrap_c(v_nc - center_kc)| - w_kc)^2),   wrap_c(x) = x - P_c rint(x / P_c) for P_c > 0
    D_n    = logsumexp_{l : N_l > 0} (ln N_l + f_l - u_l(n))
    f'_k   = -logsumexp_n (-u_k(n) - D_n),    f' = f' - f'_0
"""
import numpy as np


def logsumexp(x, axis):
    """ln sum exp(x) along axis, from the definition with the exact maximum taken out"""
    x = np.asarray(x, 'f8')
    m = x.max(axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.exp(x - m).sum(axis=axis))


def split_rows(rows, d):
    """(center, spring_const, flat_width), each (K, d), from rows (K, 3 d) laid out [center | spring_const | flat_width]"""
    r = np.asarray(rows, 'f8').reshape(-1, 3 * d)
    return r[:, :d], r[:, d:2 * d], r[:, 2 * d:]


def reduced_energy(values, energy, beta, rows, periods):
    """u (N, K) in float64.  values (N, d) (d may be 0), energy (N,) or None, beta (K,), rows (K, 3 d), periods (d,)"""
    beta = np.asarray(beta, 'f8').reshape(-1)
    v = np.asarray(values, 'f8')
    n = len(v) if v.ndim == 2 else len(energy)
    d = v.shape[1] if v.ndim == 2 else 0
    e = np.zeros(n) if energy is None else np.asarray(energy, 'f8').reshape(-1)
    total = np.repeat(e[:, None], len(beta), axis=1)
    if d:
        center, k, w = split_rows(rows, d)
        per = np.asarray(periods, 'f8').reshape(-1)
        for c in range(d):      # CVs in ascending order
            x = v[:, c, None] - center[None, :, c]
            if per[c] > 0:
                x = x - per[c] * np.rint(x / per[c])
            u = np.maximum(0., np.abs(x) - w[None, :, c])
            total = total + 0.5 * k[None, :, c] * u * u
    return beta[None, :] * total


def denominators(u, n_k, f):
    n_k = np.asarray(n_k, 'f8')
    has = n_k > 0
    return logsumexp(np.log(n_k[has])[None, :] + np.asarray(f, 'f8')[None, has] - u[:, has], axis=1)


def iterate(u, n_k, f):
    """one iteration: (f', D) with D the denominators of the f that went in"""
    D = denominators(u, n_k, f)
    fn = -logsumexp(-u - D[:, None], axis=0)
    return fn - fn[0], D


def mbar(values, energy, beta, rows, n_k, periods, tol, max_iter, f0=None, target=None):
    """dict(f, D, n_iter, last_delta[, log_w, f_target]).  D belongs to the returned f.  target: (beta_t, row_t or None)"""
    u = reduced_energy(values, energy, beta, rows, periods)
    f = np.zeros(u.shape[1]) if f0 is None else np.array(f0, 'f8')
    it, delta = 0, np.inf
    while it < max_iter:
        fn, _ = iterate(u, n_k, f)
        delta = float(np.abs(fn - f).max())
        f = fn; it += 1
        if delta < tol:
            break
    out = dict(f=f, D=denominators(u, n_k, f), n_iter=it, last_delta=delta)
    if target is not None:
        beta_t, row_t = target
        d = np.asarray(values).shape[1] if np.asarray(values).ndim == 2 else 0
        row = np.zeros((1, 3 * d)) if row_t is None else np.asarray(row_t, 'f8').reshape(1, 3 * d)
        ut = reduced_energy(values, energy, [beta_t], row, periods)[:, 0]
        x = -ut - out['D']
        lse = logsumexp(x, axis=0)
        out['log_w'] = x - lse
        out['f_target'] = -float(lse)
    return out


def naive_iterate(u, n_k, f):
    """the same iteration with plain sums of exponentials, no logarithms inside: only for tiny well-conditioned cases"""
    n_k = np.asarray(n_k, 'f8')
    den = (n_k[None, :] * np.exp(np.asarray(f, 'f8')[None, :] - u)).sum(axis=1)
    fn = -np.log((np.exp(-u) / den[:, None]).sum(axis=0))
    return fn - fn[0]


# ---- the two seeded cases of the convergence check ---------------------------------------------------------------------------------
# Both are rebuilt from the description of the prototype that set the bound (its shapes, kinds of CV and temperature), with seeds and
# parameters of their own: they are not that prototype's data, and converge in other iteration counts (500 and 270 to 1e-10).  The
# check made on them is a residual -- one more yardstick iteration moves f by less than 10 tol -- which holds for any seed.
def case_harmonic(seed=11):
    """K = 8 harmonic windows on a harmonic landscape, 500 float32 samples each, kT = 0.8: window k with centre c_k and spring k_k
    on U(x) = 1/2 k0 (x - x0)^2 samples a Gaussian exactly"""
    rng = np.random.RandomState(seed)
    kT, k0, x0 = 0.8, 1.5, 6.0
    centers = np.linspace(3.0, 10.0, 8); spring = np.full(8, 4.0)
    mean = (k0 * x0 + spring * centers) / (k0 + spring); sd = np.sqrt(kT / (k0 + spring))
    v = np.concatenate([rng.normal(mean[k], sd[k], 500) for k in range(8)]).astype('f4')[:, None]
    rows = np.column_stack((centers, spring, np.zeros(8))).astype('f4')
    energy = 0.5 * k0 * (v[:, 0].astype('f8') - x0) ** 2
    return dict(values=v, energy=energy, beta=np.full(8, 1. / kT), rows=rows, n_k=np.full(8, 500, 'i8'), periods=np.zeros(1))


def case_periodic(seed=12):
    """a 2-d case, CV 0 periodic (2 pi) with windows across the cut, CV 1 with flat bottoms; 5 windows x 257 samples"""
    rng = np.random.RandomState(seed)
    K, n = 5, 257
    c0 = np.array([-3.0, -1.5, 0.0, 1.5, 3.0]); c1 = np.linspace(8., 10., K)
    v0 = np.concatenate([rng.normal(c0[k], 0.45, n) for k in range(K)])
    v0 = v0 - 2 * np.pi * np.rint(v0 / (2 * np.pi))
    v1 = np.concatenate([rng.normal(c1[k], 0.6, n) for k in range(K)])
    v = np.column_stack((v0, v1)).astype('f4')
    rows = np.column_stack((c0, c1, np.full(K, 5.0), np.full(K, 3.0), np.zeros(K), np.full(K, 0.4))).astype('f4')
    return dict(values=v, energy=None, beta=np.full(K, 1.25), rows=rows, n_k=np.full(K, n, 'i8'), periods=np.array([2 * np.pi, 0.]))
