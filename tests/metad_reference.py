"""The float64 numpy yardstick of the metadynamics analysis (upside_hip_metad_bias, upside_hip_metad_grid, metad.py): it states the
definitions and nothing else.  Hills h = 0 .. n - 1 of a list in deposit order, centres s_h and weights w_h (float32, widened
exactly), widths sigma and periods (0 = not periodic) in double:

    wrap_c(x) = x - periods[c] rint(x / periods[c])   where periods[c] > 0, else x
    e_h(x)    = exp(-1/2 sum_c wrap_c(x_c - s_hc)^2 / sigma_c^2)
    V_m(x)    = sum_{h < m} w_h e_h(x)                the bias of the first m hills
    A_m(x)    = sum_{h < m} |w_h| e_h(x)              what the bounds of the device tests are made of
    hills_visible(r, pace, n_walker, n_initial, n_stored) = min(n_initial + n_walker floor((r - 1) / pace), n_stored)
    c(m)      = kT (ln sum_g exp(a V_m(g)) - ln sum_g exp(b V_m(g)))       b = 1 / kdT (0: plain), a = 1 / kT + b
    ln w_n    = (V_{m_n}(s_n) - c(m_n)) / kT - logsumexp_n(...)
    F_hills   = -(kT + kdT) / kdT V_n (well-tempered) or -V_n (plain)

Every log-sum-exp subtracts its exact maximum.  Pinned by tests/test_metad_config.py against a scalar double loop."""
import numpy as np

ROW_CHUNK = 512


def _arrays(centers, weights, sigma, periods):
    sg = np.asarray(sigma, 'f8').reshape(-1)
    d = len(sg)
    w = np.asarray(weights, 'f4').astype('f8').reshape(-1)
    c = np.asarray(centers, 'f4').astype('f8').reshape(len(w), d)
    per = np.zeros(d) if periods is None else np.asarray(periods, 'f8').reshape(-1)
    return c, w, sg, per, d


def hill_terms(x, c, sg, per):
    """e_h(x) for the points x (N, d) and the hills c (H, d): (N, H)"""
    q = np.zeros((len(x), len(c)))
    for k in range(len(sg)):
        dx = x[:, None, k] - c[None, :, k]
        if per[k] > 0:
            dx = dx - per[k] * np.rint(dx / per[k])
        q += dx * dx / (sg[k] * sg[k])
    return np.exp(-0.5 * q)


def bias(points, centers, weights, sigma, periods=None, n_visible=None):
    """(V, A), each (N,): V_{n_visible[i]}(points[i]) and A likewise; n_visible None: all hills"""
    c, w, sg, per, d = _arrays(centers, weights, sigma, periods)
    x = np.asarray(points, 'f8').reshape(-1, d)
    m = np.full(len(x), len(w), 'i8') if n_visible is None else np.asarray(n_visible, 'i8').reshape(-1)
    V = np.zeros(len(x)); A = np.zeros(len(x))
    for i0 in range(0, len(x), ROW_CHUNK):
        sl = slice(i0, i0 + ROW_CHUNK)
        top = int(m[sl].max()) if len(m[sl]) else 0
        e = hill_terms(x[sl], c[:top], sg, per) * (np.arange(top)[None, :] < m[sl, None])
        V[sl] = e @ w[:top]; A[sl] = e @ np.abs(w[:top])
    return V, A


def grid_points(axes):
    """the product grid in C order, (G, d)"""
    mesh = np.meshgrid(*[np.asarray(a, 'f8').reshape(-1) for a in axes], indexing='ij')
    return np.stack([m.reshape(-1) for m in mesh], axis=1)


def logsumexp(x):
    x = np.asarray(x, 'f8').reshape(-1)
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))


def bias_grid(axes, centers, weights, sigma, periods=None, checkpoints=None, scales=()):
    """dict(V (K, G), A (K, G), lse (K, Q)) at the checkpoints (hill counts; None: the whole list) of ONE list"""
    c, w, sg, per, d = _arrays(centers, weights, sigma, periods)
    g = grid_points(axes)
    ck = np.array([len(w)], 'i8') if checkpoints is None else np.asarray(checkpoints, 'i8').reshape(-1)
    V = np.zeros((len(ck), len(g))); A = np.zeros((len(ck), len(g)))
    for i0 in range(0, len(g), ROW_CHUNK):
        sl = slice(i0, i0 + ROW_CHUNK)
        e = hill_terms(g[sl], c[:int(ck.max())], sg, per)
        for j, m in enumerate(ck):
            V[j, sl] = e[:, :m] @ w[:m]; A[j, sl] = e[:, :m] @ np.abs(w[:m])
    sc = np.asarray(scales, 'f8').reshape(-1)
    lse = np.array([[logsumexp(s * V[j]) for s in sc] for j in range(len(ck))]).reshape(len(ck), len(sc))
    return dict(V=V, A=A, lse=lse)


def hills_visible(rounds, pace, n_walker=1, n_initial=0, n_stored=None):
    m = n_initial + n_walker * ((np.asarray(rounds, 'i8') - 1) // pace)
    return m if n_stored is None else np.minimum(m, n_stored)


def offset_scales(kT, kdT):
    b = 1. / kdT if kdT > 0 else 0.
    return 1. / kT + b, b


def frame_log_weights(centers, weights, sigma, frames, rounds, pace, kT, kdT, axes, n_walker=1, n_initial=0, periods=None):
    """dict(log_w, V, A, c, n_visible, n_eff, checkpoints, c_checkpoints, A_grid_max): the reweighting of the frames of one list,
    c evaluated at every distinct n_visible; A_grid_max[j] = max_g A_m(g) at checkpoint j"""
    c, w, sg, per, d = _arrays(centers, weights, sigma, periods)
    m = hills_visible(rounds, pace, n_walker, n_initial, len(w))
    V, A = bias(frames, centers, weights, sigma, periods, m)
    ck = np.unique(m)
    a, b = offset_scales(kT, kdT)
    gr = bias_grid(axes, centers, weights, sigma, periods, ck, (a, b))
    c_ck = kT * (gr['lse'][:, 0] - gr['lse'][:, 1])
    c_n = c_ck[np.searchsorted(ck, m)]
    lw = (V - c_n) / kT
    lw = lw - logsumexp(lw)
    return dict(log_w=lw, V=V, A=A, c=c_n, n_visible=m, n_eff=float(1. / np.exp(2. * lw).sum()), checkpoints=ck, c_checkpoints=c_ck,
                A_grid_max=gr['A'].max(axis=1))


def free_energy(V, kT=None, kdT=0.):
    return -(kT + kdT) / kdT * V if kdT > 0 else -V
