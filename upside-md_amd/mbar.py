"""MBAR on the device over the ladders the engine runs (upside_hip_mbar and upside_hip_mbar_gram of include/upside_engine_c.h;
csrc/kernels_mbar.hip, csrc/kernels_mbar_gram.hip): free energies of umbrella windows from the recorded CV series and of temperature
ladders from recorded energies, by self-consistent iteration or with Newton steps; their asymptotic uncertainties, and averages and
profiles in a target state with error bars, from the Gram matrix of the weight matrix (Shirts & Chodera 2008, eq. D8/D9).
Limits of the uncertainties: at most 8192 columns (states + target + observables or bins); the covariance from the Gram matrix is a
large-sample estimate -- where a window keeps few samples or neighbours overlap poorly, bootstrap(), bootstrap_sigma() and
profile_bootstrap() below give bootstrap error bars instead, all replicates solved in one device batch (upside_hip_mbar_bootstrap,
csrc/kernels_mbar_boot.hip); the samples are taken as uncorrelated by both, and bootstrapping correlated samples underestimates the
errors just as the asymptotic estimate does: timeseries.py finds the equilibration origin and the statistical inefficiency of a recorded
series on the device, and Ensemble.umbrella_mbar(decorrelate=True) applies them per window (own_state_reduced_bias is the observable).
bootstrap(draw='device') draws the counts on the device instead of the host (upside_hip_mbar_bootstrap_drawn; bootstrap_counts_device
is the draw alone), as a circular block bootstrap where block lengths are given: blocks of block_lengths(g) samples keep every sample
of a correlated series and its error bars honest."""
import ctypes as ct
import numpy as np

MAX_DIM = 8              # UPK_MBAR_MAX_DIM of include/upside_hip_kernels.h
STATE_TILE = 128         # UPK_MBAR_STATE_TILE: states staged in LDS per tile of the denominator pass
FE_TILE = 4              # UPK_MBAR_FE_TILE: states per workgroup of the free-energy pass
GRAM_TILE = 64           # UPK_MBAR_GRAM_TILE: the Gram pass computes G in tiles of 64 x 64
GRAM_MAX_COLUMNS = 8192  # UPK_MBAR_GRAM_MAX_COLUMNS
NULL_RCOND = 1e-10       # eigenvalues of I - Sigma V^T N V Sigma below this (relative) are its null space in covariance()
BOOT_MAX_COUNT = 65535   # a bootstrap count is an unsigned 16-bit number
BOOT_DRAW_TILE = 8192    # UPK_MBAR_BOOT_DRAW_TILE: a state of at most this many samples is counted in LDS by the device draw


def _bind(c):
    if getattr(c, '_mbar_bound', False):
        return
    vp, i32, i64, f64 = ct.c_void_p, ct.c_int, ct.c_longlong, ct.c_double
    c.upside_hip_mbar.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp, vp, f64, i32, vp, i32, f64, vp, vp, vp, vp, vp, vp, vp]
    c.upside_hip_mbar.restype = i32
    c.upside_hip_mbar_gram.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    c.upside_hip_mbar_gram.restype = i32
    c.upside_hip_mbar_bootstrap.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, f64, i32, vp, i32, vp, vp, vp, vp, vp]
    c.upside_hip_mbar_bootstrap.restype = i32
    c.upk_mbar_boot_solve.argtypes = [vp, ct.c_char_p, i32]
    c.upk_mbar_boot_solve.restype = i32
    u64 = ct.c_ulonglong
    c.upside_hip_mbar_bootstrap_drawn.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, u64, vp, vp, f64, i32, vp, i32, vp, vp, vp, vp, vp]
    c.upside_hip_mbar_bootstrap_drawn.restype = i32
    c.upside_hip_mbar_bootstrap_counts.argtypes = [i32, vp, i64, vp, i64, i64, u64, vp, vp]
    c.upside_hip_mbar_bootstrap_counts.restype = i32
    c.upk_mbar_boot_solve_drawn.argtypes = [vp, vp, ct.c_char_p, i32]
    c.upk_mbar_boot_solve_drawn.restype = i32
    c.upk_mbar_boot_chunk.argtypes = [i64, ct.c_size_t]
    c.upk_mbar_boot_chunk.restype = i64
    c.upside_hip_last_error.restype = ct.c_char_p
    c._mbar_bound = True


def _ptr(a):
    return None if a is None else a.ctypes.data


def _problem(values, energy, beta, rows, n_k, periods):
    """the arrays of a problem as the entry points take them: (v (N, d) f4, e (N,) f8 or None, b (K,), r (K, 3 d) f4, n_k i8, per (d,))"""
    n_k = np.ascontiguousarray(np.asarray(n_k).reshape(-1), 'i8')
    K = len(n_k)
    if values is None:
        if energy is None:
            raise ValueError('mbar: without values an energy is needed')
        values = np.zeros((len(np.asarray(energy).reshape(-1)), 0), 'f4')
    v = np.asarray(values)
    if v.ndim == 1:
        v = v[:, None]
    if v.ndim != 2:
        raise ValueError('mbar: values must be (N, d)')
    v = np.ascontiguousarray(v, 'f4')
    N, d = v.shape
    e = None
    if energy is not None:
        e = np.ascontiguousarray(np.asarray(energy, 'f8').reshape(-1))
        if len(e) != N:
            raise ValueError('mbar: energy holds %d entries for %d samples' % (len(e), N))
    b = np.ascontiguousarray(np.broadcast_to(np.asarray(beta, 'f8'), (K,)))
    r = np.zeros((K, 0), 'f4') if rows is None else np.ascontiguousarray(np.asarray(rows, 'f4'))
    if r.shape != (K, 3 * d):
        raise ValueError('mbar: rows must be (%d states, 3 x %d CVs), got %r' % (K, d, r.shape))
    per = np.zeros(d) if periods is None else np.ascontiguousarray(np.asarray(periods, 'f8').reshape(-1))
    if len(per) != d:
        raise ValueError('mbar: %d periods for %d CVs' % (len(per), d))
    return v, e, b, r, n_k, per


def own_state_reduced_bias(values, beta, rows, periods, state_of_sample):
    """(N,) float64 numpy: the reduced bias of every sample in the state it was drawn from,
        beta_k sum_c 1/2 spring_const_kc max(0, |wrap_c(values[n][c] - center_kc)| - flat_width_kc)^2,   k = state_of_sample[n],
    the u_k(n) of upside_hip_mbar without the energy term, CVs added in ascending order.  This is the observable whose correlation
    matters for a window: timeseries.detect_equilibration on it gives the window's t0 and g.  values (N, d) or (N,), beta (K,) or a
    scalar, rows (K, 3 d) = [center | spring_const | flat_width], periods (d,) or None (none periodic), state_of_sample (N,) ints."""
    v = np.asarray(values, 'f8')
    if v.ndim == 1:
        v = v[:, None]
    N, d = v.shape
    r = np.asarray(rows, 'f8').reshape(-1, 3 * d)
    K = len(r)
    k = np.asarray(state_of_sample).reshape(-1).astype('i8')
    if len(k) != N or (len(k) and (k.min() < 0 or k.max() >= K)):
        raise ValueError('mbar.own_state_reduced_bias: state_of_sample must hold %d entries in 0 .. %d' % (N, K - 1))
    b = np.broadcast_to(np.asarray(beta, 'f8'), (K,))
    per = np.zeros(d) if periods is None else np.asarray(periods, 'f8').reshape(-1)
    total = np.zeros(N)
    for c in range(d):
        x = v[:, c] - r[k, c]
        if per[c] > 0:
            x = x - per[c] * np.rint(x / per[c])
        u = np.maximum(0., np.abs(x) - r[k, 2 * d + c])
        total = total + 0.5 * r[k, d + c] * u * u
    return b[k] * total


def mbar(values, energy, beta, rows, n_k, periods=None, tol=1e-8, max_iter=10000, f0=None, target=None, want_denominators=True,
         library=None, solver='self-consistent', n_sc=10):
    """free energies f (K,) of K states from N samples, float64 on the device.
      values   (N, d) float32 CV values as recorded, d <= 8; None or (N, 0) for d = 0
      energy   (N,) unbiased potential, or None (= 0; it cancels when every beta is the same)
      beta     (K,) or a scalar for all states
      rows     (K, 3 d) = [center | spring_const | flat_width] per state: the cv_restraint per-system rows; None for d = 0
      n_k      (K,) samples drawn from each state, summing to N (the order of the samples does not matter)
      periods  (d,) period of each CV, 0 = not periodic (Ensemble.cv_periods, config.cv_periods); None: none is periodic
      tol, max_iter   stops when max |f' - f| < tol or after max_iter iterations (tol = 0: exactly max_iter); f0: the start, default 0
      target   None, or (beta_t, row_t) with row_t (3 d,) or None for no bias: the state to reweight to
      solver   'self-consistent' (the default, unchanged), or 'newton': n_sc self-consistent iterations, then one self-consistent
               iteration and one Newton step in turn (the step from gram() on the device, solved in numpy over the states with
               samples, the first of them pinned) until an iteration's delta is below tol.  A Newton step that does not lower the
               largest |gradient| is discarded and five self-consistent iterations run instead.  The result is always the output
               of a self-consistent iteration, so every entry keeps its meaning; n_iter counts self-consistent iterations (at most
               max_iter) and n_newton, the accepted Newton steps, is added.
    Returns dict(f, D (N,) the denominators of the returned f, n_iter, last_delta) and with a target also log_w (N,), the normalised
    log-weights of the samples in the target state, and f_target.  Every refusal of the entry point raises RuntimeError with its
    message."""
    from .engine import default_library
    lib = library if library is not None else default_library()
    c = lib.calc
    _bind(c)
    if solver == 'newton':
        return _newton(values, energy, beta, rows, n_k, periods, tol, max_iter, f0, target, want_denominators, lib, n_sc)
    if solver != 'self-consistent':
        raise ValueError("mbar: solver must be 'self-consistent' or 'newton'")
    v, e, b, r, n_k, per = _problem(values, energy, beta, rows, n_k, periods)
    (N, d), K = v.shape, len(n_k)
    start = None
    if f0 is not None:
        start = np.ascontiguousarray(np.asarray(f0, 'f8').reshape(-1))
        if len(start) != K:
            raise ValueError('mbar: f0 holds %d entries for %d states' % (len(start), K))
    f = np.zeros(K, 'f8')
    D = np.zeros(N, 'f8') if want_denominators else None
    n_iter = np.zeros(1, 'i4'); delta = np.zeros(1, 'f8')
    beta_t, row_t, log_w, f_t = 0., None, None, None
    if target is not None:
        beta_t, row_t = target
        if row_t is not None:
            row_t = np.ascontiguousarray(np.asarray(row_t, 'f4').reshape(-1))
            if len(row_t) != 3 * d:
                raise ValueError("mbar: the target's row must hold 3 x %d entries" % d)
        log_w = np.zeros(N, 'f8'); f_t = np.zeros(1, 'f8')
    rc = c.upside_hip_mbar(N, K, d, _ptr(v) if d else None, _ptr(e), _ptr(b), _ptr(r) if d else None, _ptr(n_k), _ptr(per) if d else None,
                           float(tol), int(max_iter), _ptr(start), int(target is not None), float(beta_t), _ptr(row_t), _ptr(f), _ptr(D),
                           _ptr(log_w), _ptr(f_t), _ptr(n_iter), _ptr(delta))
    if rc:
        raise RuntimeError('mbar failed: %s' % c.upside_hip_last_error().decode())
    out = dict(f=f, D=D, n_iter=int(n_iter[0]), last_delta=float(delta[0]))
    if target is not None:
        out['log_w'] = log_w; out['f_target'] = float(f_t[0])
    return out


def _newton(values, energy, beta, rows, n_k, periods, tol, max_iter, f0, target, want_denominators, lib, n_sc):
    """mbar(solver='newton'): every returned entry comes from the last self-consistent call; Newton steps only move its start"""
    n_k = np.asarray(n_k).reshape(-1)
    act = np.flatnonzero(n_k > 0)
    free = act[1:]
    cnt = n_k.astype('f8')

    def sc(start, n):
        return mbar(values, energy, beta, rows, n_k, periods, tol, n, f0=start, target=target, want_denominators=want_denominators, library=lib)

    def gradient(c):
        return cnt[act] * (1. - c[act])

    if int(n_sc) < 1:
        raise ValueError('mbar: n_sc must be at least 1')
    out = sc(f0, min(int(n_sc), int(max_iter)))
    n_iter, n_newton, n_next = out['n_iter'], 0, 1
    while not out['last_delta'] < tol and n_iter < max_iter:
        out = sc(out['f'], min(n_next, int(max_iter) - n_iter))
        n_iter += out['n_iter']; n_next = 1
        if out['last_delta'] < tol or n_iter >= max_iter:
            break
        if not len(free):      # one state with samples: nothing for a Newton step to move
            continue
        f = out['f']
        g = gram(values, energy, beta, rows, n_k, f, periods, library=lib)
        grad = gradient(g['colsum'])
        H = np.diag(cnt[free] * g['colsum'][free]) - cnt[free, None] * g['G'][np.ix_(free, free)] * cnt[None, free]
        trial = f.copy()
        try:
            trial[free] += np.linalg.solve(H, grad[1:])
        except np.linalg.LinAlgError:
            n_next = 5
            continue
        ok = np.isfinite(trial).all()
        if ok:
            c = gram(values, energy, beta, rows, n_k, trial, periods, want_gram=False, library=lib)['colsum']
            ok = np.isfinite(c).all() and np.abs(gradient(c)).max() < np.abs(grad).max()
        if ok:
            out = dict(out, f=trial); n_newton += 1
        else:
            n_next = 5
    out['n_iter'] = n_iter; out['n_newton'] = n_newton
    return out


def gram(values, energy, beta, rows, n_k, f, periods=None, log_columns=None, want_gram=True, library=None):
    """the Gram matrix G = W^T W (M, M) and the column sums (M,) of the MBAR weight matrix at the free energies f, float64 on the
    device (upside_hip_mbar_gram): M = K + n_extra columns, W[n, k] = exp(f_k - u_k(n) - D_n) for the K states of the problem (the
    arguments of mbar()) and W[n, K + j] = exp(log_columns[j, n]) for each explicit log-column (-inf = weight 0; NaN and +inf are
    refused).  want_gram=False computes the column sums only, a cheap pass.  Returns dict(G (or None), colsum, D (N,) the
    denominators of f).  G is bitwise symmetric and two calls return the same bits.  M <= 8192."""
    from .engine import default_library
    lib = library if library is not None else default_library()
    c = lib.calc
    _bind(c)
    v, e, b, r, n_k, per = _problem(values, energy, beta, rows, n_k, periods)
    (N, d), K = v.shape, len(n_k)
    fk = np.ascontiguousarray(np.asarray(f, 'f8').reshape(-1))
    if len(fk) != K:
        raise ValueError('mbar.gram: f holds %d entries for %d states' % (len(fk), K))
    lc, n_extra = None, 0
    if log_columns is not None:
        lc = np.ascontiguousarray(np.asarray(log_columns, 'f8'))
        if lc.ndim == 1:
            lc = lc[None, :]
        if lc.ndim != 2 or lc.shape[1] != N:
            raise ValueError('mbar.gram: log_columns must be (n_extra, %d samples), got %r' % (N, lc.shape))
        n_extra = lc.shape[0]
    M = K + n_extra
    if M > GRAM_MAX_COLUMNS:      # (before G is allocated; the entry point refuses it as well)
        raise ValueError('mbar.gram: n_state + n_extra = %d + %d columns, at most %d are supported' % (K, n_extra, GRAM_MAX_COLUMNS))
    G = np.zeros((M, M), 'f8') if want_gram else None
    colsum = np.zeros(M, 'f8'); D = np.zeros(N, 'f8')
    rc = c.upside_hip_mbar_gram(N, K, d, _ptr(v) if d else None, _ptr(e), _ptr(b), _ptr(r) if d else None, _ptr(n_k), _ptr(per) if d else None,
                                _ptr(fk), n_extra, _ptr(lc) if n_extra else None, _ptr(G), _ptr(colsum), _ptr(D))
    if rc:
        raise RuntimeError('mbar.gram failed: %s' % c.upside_hip_last_error().decode())
    return dict(G=G, colsum=colsum, D=D)


def covariance(G, n_k):
    """the asymptotic covariance Theta (M, M) of the log normalisation constants of the M columns of W from its Gram matrix
    (Shirts & Chodera 2008, eq. D9), pure numpy:
        s^2, V = eigh(G),  Sigma = sqrt(max(s^2, 0)),  Theta = V Sigma (I - Sigma V^T N V Sigma)^+ Sigma V^T,
    N = diag(n_k) padded with 0 for the columns past len(n_k).  var(f_i - f_j) = Theta_ii + Theta_jj - 2 Theta_ij.  The pseudo-inverse
    drops eigenvalues below NULL_RCOND of the largest (the constant shift of all f is an exact null direction)."""
    G = np.asarray(G, 'f8')
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise ValueError('mbar.covariance: G must be square')
    M = len(G)
    n = np.zeros(M)
    cnt = np.asarray(n_k, 'f8').reshape(-1)
    if len(cnt) > M:
        raise ValueError('mbar.covariance: %d counts for %d columns' % (len(cnt), M))
    n[:len(cnt)] = cnt
    s2, V = np.linalg.eigh(G)
    VS = V * np.sqrt(np.maximum(s2, 0.))[None, :]
    inner = np.eye(M) - VS.T @ (n[:, None] * VS)
    inner = 0.5 * (inner + inner.T)
    return VS @ np.linalg.pinv(inner, rcond=NULL_RCOND, hermitian=True) @ VS.T


def _pair_sigma(theta):
    dg = np.diag(theta)
    return np.sqrt(np.maximum(dg[:, None] + dg[None, :] - 2. * theta, 0.))


def free_energy_uncertainty(values, energy, beta, rows, n_k, f, periods=None, library=None):
    """sigma (K, K): the asymptotic standard deviation of f_i - f_j, sqrt(Theta_ii + Theta_jj - 2 Theta_ij), at the converged
    free energies f of the problem (the arguments of mbar())."""
    g = gram(values, energy, beta, rows, n_k, f, periods, library=library)
    return _pair_sigma(covariance(g['G'], n_k))


def _target_weights(values, energy, beta, rows, n_k, f, periods, target, library):
    """one self-consistent iteration from f with the target: (f', log_w) -- the weights belong to f', which equals f to within the
    tolerance f was converged to"""
    if target is None:
        raise ValueError('mbar: a target (beta_t, row_t or None) is needed')
    r = mbar(values, energy, beta, rows, n_k, periods, 0., 1, f0=f, target=target, want_denominators=False, library=library)
    return r['f'], r['log_w']


def expectation(values, energy, beta, rows, n_k, f, observables, target, periods=None, library=None):
    """(mean (m,), sigma (m,)): the averages of m observables (N, m) (or (N,)) in the target state (beta_t, row_t or None) with their
    asymptotic standard deviations, at the converged f.  Columns added to W: the target's weights w_t and, per observable,
    w_t A' / <A'> with A' = A - min A + 1 > 0; var <A> = <A'>^2 (Theta_AA + Theta_tt - 2 Theta_At)."""
    A = np.asarray(observables, 'f8')
    if A.ndim == 1:
        A = A[:, None]
    if A.ndim != 2 or not np.isfinite(A).all():
        raise ValueError('mbar.expectation: observables must be a finite (N, m) array')
    f1, log_w = _target_weights(values, energy, beta, rows, n_k, f, periods, target, library)
    if len(log_w) != len(A):
        raise ValueError('mbar.expectation: %d observables for %d samples' % (len(A), len(log_w)))
    shift = A.min(axis=0) - 1.
    Ap = A - shift[None, :]
    mean_p = (np.exp(log_w)[:, None] * Ap).sum(axis=0)
    cols = np.concatenate((log_w[None, :], (log_w[:, None] + np.log(Ap) - np.log(mean_p)[None, :]).T))
    K = len(np.asarray(n_k).reshape(-1))
    theta = covariance(gram(values, energy, beta, rows, n_k, f1, periods, log_columns=cols, library=library)['G'], n_k)
    t = K
    a = K + 1 + np.arange(A.shape[1])
    var = mean_p ** 2 * (theta[a, a] + theta[t, t] - 2. * theta[a, t])
    return mean_p + shift, np.sqrt(np.maximum(var, 0.))


def _bin_index(x, edges, period):
    """(N,) the bin of every x among edges, -1 outside: the bins of numpy.histogram (the last one is closed), x wrapped into
    [edges[0], edges[0] + period) first where period > 0"""
    e = np.asarray(edges, 'f8').reshape(-1)
    if period > 0:
        x = e[0] + np.mod(x - e[0], float(period))
    b = np.searchsorted(e, x, 'right') - 1
    b[x == e[-1]] = len(e) - 2
    b[(x < e[0]) | (x > e[-1])] = -1
    return b


def profile(values, energy, beta, rows, n_k, f, edges, kT, period=0, target=None, periods=None, cv=0, library=None):
    """(F (n_bin,), dF (n_bin,)): the free-energy profile of the target state along one CV with its asymptotic standard deviation.
    cv: the column of values to bin, or an (N,) array of its own.  F is config.mbar_profile of the target's weights.  One column is
    added to W per non-empty bin, w_t 1[bin] / p_b; dF_b = kT sqrt(Theta_bb + Theta_rr - 2 Theta_br) relative to the lowest bin r
    (dF_r = 0).  An empty bin has F = +inf and dF = nan."""
    from . import config
    f1, log_w = _target_weights(values, energy, beta, rows, n_k, f, periods, target, library)
    x = np.asarray(values)[:, cv] if np.ndim(cv) == 0 else np.asarray(cv)
    x = np.asarray(x, 'f8').reshape(-1)
    F = config.mbar_profile(x, log_w, edges, kT, period)
    b = _bin_index(x, edges, period)
    full = np.flatnonzero(np.isfinite(F))
    dF = np.full(len(F), np.nan)
    if not len(full):
        return F, dF
    cols = np.full((len(full), len(x)), -np.inf)
    for i, bin_ in enumerate(full):
        inside = b == bin_
        cols[i, inside] = log_w[inside] + F[bin_] / float(kT)      # ln (w_n / p_b), p_b = exp(-F_b / kT)
    K = len(np.asarray(n_k).reshape(-1))
    theta = covariance(gram(values, energy, beta, rows, n_k, f1, periods, log_columns=cols, library=library)['G'], n_k)
    idx = K + np.arange(len(full))
    r = idx[np.argmin(F[full])]
    dF[full] = float(kT) * np.sqrt(np.maximum(theta[idx, idx] + theta[r, r] - 2. * theta[idx, r], 0.))
    return F, dF


# ---- the bootstrap: replicates of the problem with integer sample weights, solved in one device batch ---------------------------------
class _BootProblem(ct.Structure):
    """upk_mbar_boot_problem_t of include/upside_hip_kernels.h"""
    _fields_ = [('n_sample', ct.c_longlong), ('n_state', ct.c_int), ('d', ct.c_int), ('values', ct.c_void_p), ('energy', ct.c_void_p),
                ('beta', ct.c_void_p), ('rows', ct.c_void_p), ('n_k', ct.c_void_p), ('periods', ct.c_void_p), ('state_of_sample', ct.c_void_p),
                ('n_replicate', ct.c_int), ('counts', ct.c_void_p), ('tol', ct.c_double), ('max_iter', ct.c_int), ('f0', ct.c_void_p),
                ('n_column', ct.c_int), ('log_numerator', ct.c_void_p), ('workspace_bytes', ct.c_size_t), ('f_boot', ct.c_void_p),
                ('column_boot', ct.c_void_p), ('n_iter', ct.c_void_p), ('last_delta', ct.c_void_p)]


class _BootDraw(ct.Structure):
    """upk_mbar_boot_draw_t of include/upside_hip_kernels.h"""
    _fields_ = [('seed', ct.c_ulonglong), ('block', ct.c_void_p), ('first_replicate', ct.c_longlong), ('counts_out', ct.c_void_p)]


def _origins(n_k, state_of_sample):
    """(state_of_sample (N,) i4, grouped): the default is the samples grouped by state, np.repeat(arange(K), n_k)"""
    n_k = np.asarray(n_k).reshape(-1).astype('i8')
    if state_of_sample is None:
        return np.repeat(np.arange(len(n_k), dtype='i4'), n_k), True
    sos = np.asarray(state_of_sample).reshape(-1)
    if sos.dtype.kind not in 'iu':
        raise ValueError('mbar: state_of_sample must hold integers')
    return np.ascontiguousarray(sos, 'i4'), False


def bootstrap_counts(n_k, n_bootstrap, seed=0, state_of_sample=None):
    """(B, N) uint16: the sample counts of B = n_bootstrap stratified bootstrap replicates -- per state k, in ascending order of k,
    numpy.random.default_rng(seed).multinomial(n_k[k], uniform over the state's n_k[k] samples, size=B), so every replicate keeps
    every state's sample count.  state_of_sample (N,): the state each sample was drawn from, default np.repeat(arange(K), n_k)
    (the samples grouped by state); the draw of a state goes to its samples in their order.  Raises ValueError where a count would
    exceed 65535 or state_of_sample does not name n_k[k] samples for state k."""
    n_k = np.asarray(n_k).reshape(-1).astype('i8')
    B = int(n_bootstrap)
    if B < 1:
        raise ValueError('mbar.bootstrap_counts: n_bootstrap = %d, at least one replicate is needed' % B)
    if (n_k < 0).any():
        raise ValueError('mbar.bootstrap_counts: a negative n_k')
    sos, grouped = _origins(n_k, state_of_sample)
    N, K = int(n_k.sum()), len(n_k)
    if len(sos) != N or (N and (sos.min() < 0 or sos.max() >= K)) or not np.array_equal(np.bincount(sos, minlength=K), n_k):
        raise ValueError('mbar.bootstrap_counts: state_of_sample must name n_k[k] samples for every state k')
    order = None if grouped else np.argsort(sos, kind='stable')
    start = np.concatenate(([0], np.cumsum(n_k)))
    rng = np.random.default_rng(seed)
    counts = np.zeros((B, N), 'u2')
    for k in range(K):
        m = int(n_k[k])
        if not m:
            continue
        draw = rng.multinomial(m, np.full(m, 1. / m), size=B)
        if draw.max() > BOOT_MAX_COUNT:
            raise ValueError('mbar.bootstrap_counts: a count of %d in state %d exceeds %d' % (draw.max(), k, BOOT_MAX_COUNT))
        if grouped:
            counts[:, start[k]:start[k + 1]] = draw
        else:
            counts[:, order[start[k]:start[k + 1]]] = draw
    return counts


def _seed64(seed, who):
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError('%s: the seed must be an unsigned 64-bit number' % who)
    return seed


def _block_array(block, K, who):
    """None, or (K,) i8 block lengths from an int or a (K,) array (their range is the entry point's to refuse)"""
    if block is None:
        return None
    b = np.asarray(block)
    if b.dtype.kind not in 'iu':
        raise ValueError('%s: block must hold integers' % who)
    if b.ndim == 0:
        b = np.full(K, int(b))
    if b.shape != (K,):
        raise ValueError('%s: block must be one integer or (%d states,), got %r' % (who, K, b.shape))
    return np.ascontiguousarray(b, 'i8')


def block_lengths(g, factor=5):
    """(K,) i8 block lengths for the circular block bootstrap of series with statistical inefficiencies g: ceil(factor g), and at
    least 1 where g < 1 (no estimate).  Why a factor, and why 5: a block bootstrap with blocks of L samples sees the correlations
    inside a block and none across block borders.  For exponentially decaying correlations rho_t = phi^t, g = (1 + phi) / (1 - phi),
    the variance of a mean it reports is the Bartlett-weighted sum var / n (1 + 2 sum_{t<L} (1 - t / L) phi^t) =
    var / n (g - 2 phi / ((1 - phi)^2 L) + O(phi^L / L)), and 2 phi / (1 - phi)^2 = (g^2 - 1) / 2: it is low by (g^2 - 1) / (2 g L)
    relative, about g / (2 L).  At L = ceil(g) the variance is about half of what it should be (sigma 30 % low); at L = factor g it
    is low by 1 / (2 factor), so factor 5 leaves the variance 10 % and the standard deviation about 5 % low -- the sampling noise of
    the standard deviation over 200 replicates, 1 / sqrt(2 x 200).  (AR(1) with phi = 0.8, n = 4096, g = 9: L = 9 gives 0.057, L = 40
    gives 0.076, L = 1 gives 0.026 against the analytic 0.077.)  A larger factor buys little and leaves fewer blocks, n / L, to draw."""
    g = np.atleast_1d(np.asarray(g, 'f8'))
    if not (float(factor) > 0):
        raise ValueError('mbar.block_lengths: the factor must be positive')
    with np.errstate(invalid='ignore'):
        L = np.ceil(float(factor) * np.where(np.isfinite(g) & (g >= 1.), g, 0.))
    return np.maximum(L, 1.).astype('i8')


def bootstrap_counts_device(n_k, n_bootstrap, seed=0, state_of_sample=None, block=None, first=0, library=None):
    """(B, N) uint16: the counts of replicates first .. first + n_bootstrap - 1 of the DEVICE draw (upside_hip_mbar_bootstrap_counts;
    include/upside_engine_c.h states it and tests/mbar_boot_draw_reference.py restates it in numpy): per state the circular block
    bootstrap with block length min(max(block[k], 1), n_k[k]) -- block None or 1 is the plain stratified bootstrap -- from the
    counter-based Threefry4x32-20, so a replicate's counts depend on (seed, its index, k, n_k[k], block[k]) alone.  seed: an
    unsigned 64-bit number.  block: None, one integer or (K,).  state_of_sample as bootstrap_counts takes it; block > 1 needs each
    state's samples in time order.  These are the counts bootstrap(draw='device') solves with and returns with want_counts=True.
    Every refusal of the entry point raises RuntimeError with its message."""
    from .engine import default_library
    c = (library if library is not None else default_library()).calc
    _bind(c)
    who = 'mbar.bootstrap_counts_device'
    n_k = np.ascontiguousarray(np.asarray(n_k).reshape(-1), 'i8')
    K, N, B = len(n_k), int(n_k.sum()), int(n_bootstrap)
    sos = None
    if state_of_sample is not None:
        sos, _ = _origins(n_k, state_of_sample)
        if len(sos) != N:
            raise ValueError('%s: state_of_sample holds %d entries for %d samples' % (who, len(sos), N))
    blk = _block_array(block, K, who)
    counts = np.zeros((max(B, 0), N), 'u2')
    if c.upside_hip_mbar_bootstrap_counts(K, _ptr(n_k), N, _ptr(sos), B, int(first), _seed64(seed, who), _ptr(blk), _ptr(counts)):
        raise RuntimeError('%s failed: %s' % (who, c.upside_hip_last_error().decode()))
    return counts


def bootstrap(values, energy, beta, rows, n_k, f, state_of_sample=None, n_bootstrap=200, seed=0, counts=None, periods=None, tol=1e-8,
              max_iter=10000, log_numerators=None, library=None, workspace_bytes=None, draw='host', block=None, want_counts=None):
    """bootstrap replicates of the problem (the arguments of mbar()), all solved in ONE batch on the device (upside_hip_mbar_bootstrap):
    replicate b weights sample n by counts[b, n] and iterates from f (the full-sample solution; None = 0) until its max |f' - f| < tol
    or max_iter; a replicate that has converged leaves the grid, the host synchronises once per iteration for all, the samples are
    copied once.
      state_of_sample  (N,) the state every sample was drawn from; None: the samples are grouped by state, np.repeat(arange(K), n_k)
      counts           (B, N) uint16, per replicate and state adding up to n_k; None: bootstrap_counts(n_k, n_bootstrap, seed, ...)
      log_numerators   None or (J, N): columns carrying a target state, an observable or a profile bin WITHOUT the denominators (they
                       differ per replicate), -inf = weight 0; columns[b, j] = -logsumexp_n (ln c_b(n) + log_numerators[j, n] - D_b(n))
                       at the returned f_b, +inf where no sample of the replicate contributes
      workspace_bytes  None, or the bytes the denominators of the replicates solved together may fill (at most the default, 512 MB):
                       the results do not depend on it, bit for bit
      draw             'host' (the default): the counts are given or come from bootstrap_counts.  'device': they are drawn on the
                       device, chunk by chunk, into the buffer the solve reads (upside_hip_mbar_bootstrap_drawn; the draw is
                       bootstrap_counts_device's, replicates 0 .. n_bootstrap - 1 of `seed`, an unsigned 64-bit number): no host
                       array of counts, no host pass over them, no copy.  Another stream of random numbers than 'host'.
      block            with draw='device': None, one integer or (K,) block lengths of the circular block bootstrap, for correlated
                       series kept whole (block_lengths(g)); each state's samples must be in time order
      want_counts      with draw='device': True copies the drawn counts back; given the same counts, draw='host' returns the same bits
    Returns dict(f_boot (B, K), n_iter (B,), last_delta (B,), converged (B,) = last_delta < tol, counts (B, N)) and columns (B, J)
    when columns were asked for; with draw='device', counts only with want_counts=True, and seed and block (K,) i8 (None: 1) are
    added.  The samples are taken as uncorrelated unless blocks are drawn: bootstrapping correlated samples sample by sample
    underestimates the errors, so subsample first (Ensemble.umbrella_mbar(decorrelate=True), timeseries.py) or draw blocks.  block
    with draw='host', counts with draw='device', or a draw that is neither raise ValueError.  Every refusal of the entry point
    raises RuntimeError with its message."""
    if draw not in ('host', 'device'):
        raise ValueError("mbar.bootstrap: draw must be 'host' or 'device', got %r" % (draw,))
    if draw == 'host' and block is not None:
        raise ValueError("mbar.bootstrap: block lengths are drawn on the device only, pass draw='device'")
    if draw == 'device' and counts is not None:
        raise ValueError("mbar.bootstrap: with draw='device' the counts are drawn, none may be given")
    from .engine import default_library
    lib = library if library is not None else default_library()
    c = lib.calc
    _bind(c)
    v, e, b, r, n_k, per = _problem(values, energy, beta, rows, n_k, periods)
    (N, d), K = v.shape, len(n_k)
    sos, _ = _origins(n_k, state_of_sample)
    if len(sos) != N:
        raise ValueError('mbar.bootstrap: state_of_sample holds %d entries for %d samples' % (len(sos), N))
    device = draw == 'device'
    if device:
        B = int(n_bootstrap)
        seed = _seed64(seed, 'mbar.bootstrap')
        blk = _block_array(block, K, 'mbar.bootstrap')
        cnt = np.zeros((max(B, 0), N), 'u2') if want_counts else None
    else:
        if counts is None:
            counts = bootstrap_counts(n_k, n_bootstrap, seed, state_of_sample)
        cnt = np.asarray(counts)
        if cnt.ndim == 1:
            cnt = cnt[None, :]
        if cnt.ndim != 2 or cnt.shape[1] != N:
            raise ValueError('mbar.bootstrap: counts must be (B, %d samples), got %r' % (N, cnt.shape))
        if cnt.dtype != np.uint16:
            if cnt.dtype.kind not in 'iu' or (cnt.size and (cnt.min() < 0 or cnt.max() > BOOT_MAX_COUNT)):
                raise ValueError('mbar.bootstrap: counts must be integers in 0 .. %d' % BOOT_MAX_COUNT)
        cnt = np.ascontiguousarray(cnt, 'u2')
        B = cnt.shape[0]
    start = None
    if f is not None:
        start = np.ascontiguousarray(np.asarray(f, 'f8').reshape(-1))
        if len(start) != K:
            raise ValueError('mbar.bootstrap: f holds %d entries for %d states' % (len(start), K))
    ln, J = None, 0
    if log_numerators is not None:
        ln = np.ascontiguousarray(np.asarray(log_numerators, 'f8'))
        if ln.ndim == 1:
            ln = ln[None, :]
        if ln.ndim != 2 or ln.shape[1] != N:
            raise ValueError('mbar.bootstrap: log_numerators must be (J, %d samples), got %r' % (N, ln.shape))
        J = ln.shape[0]
    f_boot = np.zeros((max(B, 0), K), 'f8'); cols = np.zeros((max(B, 0), J), 'f8')
    n_iter = np.zeros(max(B, 0), 'i4'); delta = np.zeros(max(B, 0), 'f8')
    if device:
        cnt_out = _ptr(cnt) if cnt is not None and cnt.size else None
        if workspace_bytes is None:
            rc = c.upside_hip_mbar_bootstrap_drawn(N, K, d, _ptr(v) if d else None, _ptr(e), _ptr(b), _ptr(r) if d else None, _ptr(n_k),
                                                   _ptr(per) if d else None, _ptr(sos), B, seed, _ptr(blk), cnt_out, float(tol), int(max_iter), _ptr(start),
                                                   J, _ptr(ln) if J else None, _ptr(f_boot), _ptr(cols) if J else None, _ptr(n_iter), _ptr(delta))
            msg = c.upside_hip_last_error().decode() if rc else ''
        else:      # the same host side with a workspace of the caller's size (upk_mbar_boot_solve_drawn)
            p = _BootProblem(N, K, d, _ptr(v) if d else None, _ptr(e), _ptr(b), _ptr(r) if d else None, _ptr(n_k), _ptr(per) if d else None, _ptr(sos), B,
                             None, float(tol), int(max_iter), _ptr(start), J, _ptr(ln) if J else None, int(workspace_bytes),
                             _ptr(f_boot), _ptr(cols) if J else None, _ptr(n_iter), _ptr(delta))
            dr = _BootDraw(seed, _ptr(blk), 0, cnt_out)
            buf = ct.create_string_buffer(256)
            rc = c.upk_mbar_boot_solve_drawn(ct.byref(p), ct.byref(dr), buf, 256)
            msg = buf.value.decode()
        if rc:
            raise RuntimeError('mbar.bootstrap failed: %s' % msg)
        out = dict(f_boot=f_boot, n_iter=n_iter, last_delta=delta, converged=delta < tol, seed=seed, block=blk)
        if want_counts:
            out['counts'] = cnt
        if log_numerators is not None:
            out['columns'] = cols
        return out
    if workspace_bytes is None:
        rc = c.upside_hip_mbar_bootstrap(N, K, d, _ptr(v) if d else None, _ptr(e), _ptr(b), _ptr(r) if d else None, _ptr(n_k), _ptr(per) if d else None,
                                         _ptr(sos), B, _ptr(cnt) if B else None, float(tol), int(max_iter), _ptr(start), J, _ptr(ln) if J else None,
                                         _ptr(f_boot), _ptr(cols) if J else None, _ptr(n_iter), _ptr(delta))
        msg = c.upside_hip_last_error().decode() if rc else ''
    else:      # the same host side with a workspace of the caller's size (upk_mbar_boot_solve): the chunking is all that differs
        p = _BootProblem(N, K, d, _ptr(v) if d else None, _ptr(e), _ptr(b), _ptr(r) if d else None, _ptr(n_k), _ptr(per) if d else None, _ptr(sos), B,
                         _ptr(cnt) if B else None, float(tol), int(max_iter), _ptr(start), J, _ptr(ln) if J else None, int(workspace_bytes),
                         _ptr(f_boot), _ptr(cols) if J else None, _ptr(n_iter), _ptr(delta))
        buf = ct.create_string_buffer(256)
        rc = c.upk_mbar_boot_solve(ct.byref(p), buf, 256)
        msg = buf.value.decode()
    if rc:
        raise RuntimeError('mbar.bootstrap failed: %s' % msg)
    out = dict(f_boot=f_boot, n_iter=n_iter, last_delta=delta, converged=delta < tol, counts=cnt)
    if log_numerators is not None:
        out['columns'] = cols
    return out


def boot_chunk(n_sample, workspace_bytes, library=None):
    """the replicates solved together with a workspace of that many bytes (upk_mbar_boot_chunk); 0: not even one fits"""
    from .engine import default_library
    c = (library if library is not None else default_library()).calc
    _bind(c)
    return int(c.upk_mbar_boot_chunk(int(n_sample), int(workspace_bytes)))


def bootstrap_sigma(f_boot, converged=None):
    """sigma (K, K): the standard deviation (ddof = 1) over the converged replicates of f_i - f_j.  f_boot: (B, K), or the dict
    bootstrap() returned (its 'converged' is then used); converged: (B,) bools, None = all.  Unconverged replicates are left out and
    their number is reported by a RuntimeWarning; with fewer than two converged replicates every entry is nan."""
    if isinstance(f_boot, dict):
        if converged is None:
            converged = f_boot['converged']
        f_boot = f_boot['f_boot']
    fb = np.asarray(f_boot, 'f8')
    if fb.ndim != 2:
        raise ValueError('mbar.bootstrap_sigma: f_boot must be (B, K)')
    if converged is not None:
        ok = np.asarray(converged, bool).reshape(-1)
        if len(ok) != len(fb):
            raise ValueError('mbar.bootstrap_sigma: %d flags for %d replicates' % (len(ok), len(fb)))
        if not ok.all():
            import warnings
            warnings.warn('mbar.bootstrap_sigma: %d of %d replicates did not converge and are left out' % (int((~ok).sum()), len(ok)), RuntimeWarning)
        fb = fb[ok]
    K = fb.shape[1]
    if len(fb) < 2:
        return np.full((K, K), np.nan)
    sigma = (fb[:, :, None] - fb[:, None, :]).std(axis=0, ddof=1)
    sigma[np.arange(K), np.arange(K)] = 0.
    return 0.5 * (sigma + sigma.T)


def _target_reduced_energy(values, energy, target, periods):
    """(N,) u_t(n) of the target (beta_t, row_t or None) in float64 on the host"""
    beta_t, row_t = target
    v = np.asarray(values, 'f8')
    if v.ndim == 1:
        v = v[:, None]
    u = np.zeros(len(v))
    if row_t is not None and v.shape[1]:
        u = own_state_reduced_bias(v, float(beta_t), np.asarray(row_t, 'f8').reshape(1, -1), periods, np.zeros(len(v), 'i8'))
    if energy is not None:
        u = u + float(beta_t) * np.asarray(energy, 'f8').reshape(-1)
    return u


def profile_bootstrap(values, energy, beta, rows, n_k, f, edges, kT, period=0, target=None, periods=None, cv=0, state_of_sample=None,
                      n_bootstrap=200, seed=0, counts=None, tol=1e-8, max_iter=10000, library=None, draw='host', block=None):
    """(F (n_bin,), dF_boot (n_bin,)): the free-energy profile of the target state along one CV, as profile() gives it from the full
    sample, with the BOOTSTRAP standard deviation (ddof = 1) over the converged replicates of kT (F_bin - F_r) relative to the full
    sample's lowest bin r (dF_boot[r] = 0).  One column per bin that holds samples, -u_target(n) inside the bin and -inf outside, goes
    through bootstrap() (whose arguments state_of_sample, n_bootstrap, seed, counts, tol, max_iter, draw, block are); F_bin / kT of a replicate is
    its column up to a constant that cancels in the difference.  dF_boot is nan for a bin that is empty in the full sample; replicates
    in which the bin or r received no sample (+inf) are left out of that bin's deviation."""
    from . import config
    if target is None:
        raise ValueError('mbar: a target (beta_t, row_t or None) is needed')
    f1, log_w = _target_weights(values, energy, beta, rows, n_k, f, periods, target, library)
    x = np.asarray(values)[:, cv] if np.ndim(cv) == 0 else np.asarray(cv)
    x = np.asarray(x, 'f8').reshape(-1)
    F = config.mbar_profile(x, log_w, edges, kT, period)
    b = _bin_index(x, edges, period)
    full = np.flatnonzero(np.isfinite(F))
    dF = np.full(len(F), np.nan)
    if not len(full):
        return F, dF
    ut = _target_reduced_energy(values, energy, target, periods)
    cols = np.full((len(full), len(x)), -np.inf)
    for i, bin_ in enumerate(full):
        inside = b == bin_
        cols[i, inside] = -ut[inside]
    r = bootstrap(values, energy, beta, rows, n_k, f1, state_of_sample, n_bootstrap, seed, counts, periods, tol, max_iter, cols, library,
                  draw=draw, block=block)
    g = float(kT) * r['columns'][r['converged']]
    ref = int(np.argmin(F[full]))
    for i, bin_ in enumerate(full):
        both = np.isfinite(g[:, i]) & np.isfinite(g[:, ref])
        diff = g[both, i] - g[both, ref]
        dF[bin_] = diff.std(ddof=1) if len(diff) > 1 else np.nan
    return F, dF
