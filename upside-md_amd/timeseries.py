"""Time-series analysis of recorded series on the device (upside_hip_series_inefficiency of include/upside_engine_c.h;
csrc/kernels_series.hip): the statistical inefficiency g of a series at a set of origins (Chodera et al. 2007; pymbar's
statistical_inefficiency(fast=False)), automated equilibration detection (Chodera 2016: the origin t0 at which the number of
effectively uncorrelated samples (T - t0) / g(t0) is largest) and the indices of a decorrelated subsample.  This is what the
uncertainties of mbar.py need of their samples: Ensemble.umbrella_mbar(decorrelate=True) applies it per window."""
import ctypes as ct
import numpy as np

MIN_TAIL = 16        # UPK_SERIES_MIN_TAIL of include/upside_hip_kernels.h: a shorter tail has no estimate (g = 0, stop_lag = -1)
LAG_BLOCK = 128      # UPK_SERIES_LAG_BLOCK: lags are produced in blocks of 128
PIECE = 2048         # UPK_SERIES_PIECE: the time axis is cut at the origins and then every 2048 samples


def _bind(c):
    if getattr(c, '_series_bound', False):
        return
    vp, i32, i64 = ct.c_void_p, ct.c_int, ct.c_longlong
    c.upside_hip_series_inefficiency.argtypes = [i32, i64, vp, vp, i32, vp, i32, i64, vp, vp, vp, vp]
    c.upside_hip_series_inefficiency.restype = i32
    c.upside_hip_last_error.restype = ct.c_char_p
    c._series_bound = True


def _series(series, lengths):
    a = np.asarray(series, 'f8')
    single = a.ndim == 1
    if single:
        a = a[None, :]
    if a.ndim != 2:
        raise ValueError('timeseries: series must be (K, T) or (T,)')
    a = np.ascontiguousarray(a)
    K, T = a.shape
    if lengths is None:
        n = np.full(K, T, 'i8')
    else:
        n = np.ascontiguousarray(np.asarray(lengths).reshape(-1), 'i8')
        if len(n) != K:
            raise ValueError('timeseries: %d lengths for %d series' % (len(n), K))
    return a, n, single


def statistical_inefficiency(series, origins=(0,), mintime=3, max_lag=None, lengths=None, library=None):
    """the statistical inefficiency of K series at J origins, float64 on the device.
      series   (K, T) or (T,), float64; lengths (K,): the samples of each series that count, default T for all
      origins  (J,) ascending sample indices t0: the estimate is that of the tail series[k, t0:length]
      mintime  the sum over lags stops at the first lag t > mintime whose correlation C(t) <= 0
      max_lag  the largest lag that is summed; None: no cap (every lag up to the tail's length - 2)
    Returns dict(g, stop_lag, mean, variance, n_eff), each (K, J) ((J,) for a (T,) series): g >= 1; stop_lag the lag at which the sum
    stopped; mean and variance of the tail; n_eff = (length - origin) / g.  A tail shorter than 16 samples has no estimate: g = 0,
    stop_lag = -1, n_eff = 0.  A constant tail has g = 1, stop_lag = 0.  Every refusal of the entry point raises RuntimeError with
    its message."""
    from .engine import default_library
    lib = library if library is not None else default_library()
    c = lib.calc
    _bind(c)
    a, n, single = _series(series, lengths)
    K, T = a.shape
    o = np.ascontiguousarray(np.asarray(origins).reshape(-1), 'i8')
    J = len(o)
    cap = (1 << 62) if max_lag is None else int(max_lag)
    g = np.zeros((K, J), 'f8'); stop = np.zeros((K, J), 'i8'); mean = np.zeros((K, J), 'f8'); var = np.zeros((K, J), 'f8')
    rc = c.upside_hip_series_inefficiency(K, T, n.ctypes.data, a.ctypes.data, J, o.ctypes.data, int(mintime), cap, g.ctypes.data,
                                          stop.ctypes.data, mean.ctypes.data, var.ctypes.data)
    if rc:
        raise RuntimeError('statistical_inefficiency failed: %s' % c.upside_hip_last_error().decode())
    tail = (n[:, None] - o[None, :]).astype('f8')
    n_eff = np.where(g > 0., tail / np.where(g > 0., g, 1.), 0.)
    out = dict(g=g, stop_lag=stop, mean=mean, variance=var, n_eff=n_eff)
    return dict((k, v[0]) for k, v in out.items()) if single else out


def equilibration_origins(T, n_origin=64):
    """the origins detect_equilibration tries on series of T samples: j * max(1, T // n_origin), j = 0 .. n_origin - 1, below T"""
    step = max(1, int(T) // int(n_origin))
    o = step * np.arange(int(n_origin), dtype='i8')
    return o[o < max(int(T), 1)]


def detect_equilibration(series, n_origin=64, mintime=3, max_lag=None, lengths=None, library=None):
    """(t0, g, n_eff), each (K,) (scalars for a (T,) series): per series the origin among equilibration_origins(T, n_origin) with the
    largest number of effectively uncorrelated samples n_eff = (length - t0) / g(t0), its g and that n_eff (Chodera 2016).  On a tie
    the earliest origin wins.  A series too short for any estimate returns t0 = 0, g = 0, n_eff = 0."""
    a, n, single = _series(series, lengths)
    o = equilibration_origins(a.shape[1], n_origin)
    r = statistical_inefficiency(a, o, mintime, max_lag, n, library)
    best = np.argmax(r['n_eff'], axis=1)      # (the first of equal maxima)
    k = np.arange(len(a))
    t0, g, n_eff = o[best], r['g'][k, best], r['n_eff'][k, best]
    return (int(t0[0]), float(g[0]), float(n_eff[0])) if single else (t0, g, n_eff)


def subsample_indices(length, t0, g):
    """t0 + ceil(g) * arange(...) below length: the indices of a decorrelated subsample of series[t0:length], the conservative rule of
    pymbar's subsampleCorrelatedData(conservative=True).  g < 1 (no estimate) keeps nothing."""
    if not g >= 1.:
        return np.zeros(0, 'i8')
    return np.arange(int(t0), int(length), int(np.ceil(g)), dtype='i8')
