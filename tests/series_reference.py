"""Float64 numpy yardstick of the statistical inefficiency of a series at a set of origins (the statement of
upside_hip_series_inefficiency in include/upside_engine_c.h; pymbar's statistical_inefficiency(fast=False)), written from the
definition: a plain loop over the lags of every (series, origin) with direct sums over the tail.  Nothing is tiled, nothing is shared
between origins and nothing is shared with csrc/kernels_series.hip.  Pinned by tests/test_series_config.py.

    A_n = a[t0 + n], n < Tt = length - t0;  mu = mean(A),  s2 = mean((A - mu)^2)
    C(t) = sum_{n=0}^{Tt-1-t} (A_n - mu)(A_{n+t} - mu) / ((Tt - t) s2)
    g = max(1, 1 + 2 sum_{t=1}^{t_stop-1} C(t) (1 - t / Tt))
    t_stop = the first t with (C(t) <= 0 and t > mintime), or max_lag + 1, or Tt - 1, whichever comes first
"""
import numpy as np

MIN_TAIL = 16


def tail_inefficiency(A, mintime=3, max_lag=None):
    """(g, stop_lag, mean, variance, c_margin) of one tail A.  c_margin: the smallest |C(t)| over the lags t > mintime that were
    evaluated (inf where there was none): how far the stop decision was from going the other way."""
    A = np.asarray(A, 'f8')
    Tt = len(A)
    if Tt == 0:
        return 0., -1, 0., 0., np.inf
    mu = A.mean()
    dA = A - mu
    s2 = float((dA * dA).mean())
    if Tt < MIN_TAIL:
        return 0., -1, float(mu), s2, np.inf
    if s2 == 0.:
        return 1., 0, float(mu), 0., np.inf
    g, t, margin = 1., 1, np.inf
    stop = None
    while t < Tt - 1 and (max_lag is None or t <= max_lag):
        C = float((dA[:Tt - t] * dA[t:]).sum()) / ((Tt - t) * s2)
        if t > mintime:
            margin = min(margin, abs(C))
        if C <= 0. and t > mintime:
            stop = t
            break
        g += 2. * C * (1. - t / float(Tt))
        t += 1
    if stop is None:
        stop = t      # max_lag + 1 or Tt - 1
    return max(g, 1.), stop, float(mu), s2, margin


def statistical_inefficiency(series, origins=(0,), mintime=3, max_lag=None, lengths=None):
    """dict(g, stop_lag, mean, variance, n_eff, c_margin), each (K, J), for series (K, T) (or (T,), which is taken as K = 1)"""
    a = np.asarray(series, 'f8')
    if a.ndim == 1:
        a = a[None, :]
    K, T = a.shape
    n = np.full(K, T, 'i8') if lengths is None else np.asarray(lengths, 'i8').reshape(-1)
    o = np.asarray(origins, 'i8').reshape(-1)
    J = len(o)
    out = dict(g=np.zeros((K, J)), stop_lag=np.zeros((K, J), 'i8'), mean=np.zeros((K, J)), variance=np.zeros((K, J)),
               n_eff=np.zeros((K, J)), c_margin=np.zeros((K, J)))
    for k in range(K):
        for j in range(J):
            g, stop, mu, s2, margin = tail_inefficiency(a[k, min(int(o[j]), int(n[k])):n[k]], mintime, max_lag)
            out['g'][k, j] = g; out['stop_lag'][k, j] = stop; out['mean'][k, j] = mu; out['variance'][k, j] = s2
            out['c_margin'][k, j] = margin
            out['n_eff'][k, j] = (n[k] - o[j]) / g if g > 0. else 0.
    return out


def equilibration_origins(T, n_origin=64):
    step = max(1, int(T) // int(n_origin))
    o = step * np.arange(int(n_origin), dtype='i8')
    return o[o < max(int(T), 1)]


def detect_equilibration(series, n_origin=64, mintime=3, max_lag=None, lengths=None):
    """dict(t0, g, n_eff, gap (each (K,)), c_margin (K,), all): per series the origin with the largest n_eff (the earliest on a tie);
    gap = (best - second best) / best n_eff over the origins (inf with one origin): how far the choice was from another origin;
    c_margin = the smallest over the origins; all = the whole statistical_inefficiency result"""
    a = np.asarray(series, 'f8')
    if a.ndim == 1:
        a = a[None, :]
    o = equilibration_origins(a.shape[1], n_origin)
    r = statistical_inefficiency(a, o, mintime, max_lag, lengths)
    K = len(a)
    best = np.zeros(K, 'i8'); gap = np.full(K, np.inf)
    for k in range(K):
        ne = r['n_eff'][k]
        b = 0
        for j in range(1, len(o)):
            if ne[j] > ne[b]:
                b = j
        best[k] = b
        if len(o) > 1:
            second = max(ne[j] for j in range(len(o)) if j != b)
            gap[k] = (ne[b] - second) / ne[b] if ne[b] > 0 else 0.
    idx = np.arange(K)
    return dict(t0=o[best], g=r['g'][idx, best], n_eff=r['n_eff'][idx, best], gap=gap, c_margin=r['c_margin'].min(axis=1), all=r)


def subsample_indices(length, t0, g):
    if not g >= 1.:
        return np.zeros(0, 'i8')
    return np.arange(int(t0), int(length), int(np.ceil(g)), dtype='i8')


def ar1(rng, T, phi, K=1):
    """K stationary AR(1) series of T samples with unit variance: x_n = phi x_{n-1} + sqrt(1 - phi^2) e_n"""
    e = rng.normal(size=(K, T))
    x = np.empty((K, T))
    x[:, 0] = e[:, 0]
    s = np.sqrt(1. - phi * phi)
    for n in range(1, T):
        x[:, n] = phi * x[:, n - 1] + s * e[:, n]
    return x
