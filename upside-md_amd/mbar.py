"""MBAR on the device over the ladders the engine runs (upside_hip_mbar of include/upside_engine_c.h; csrc/kernels_mbar.hip): free
energies of umbrella windows from the recorded CV series and of temperature ladders from recorded energies.  The profile along a CV
from the returned log-weights is config.mbar_profile."""
import ctypes as ct
import numpy as np

MAX_DIM = 8              # UPK_MBAR_MAX_DIM of include/upside_hip_kernels.h
STATE_TILE = 128         # UPK_MBAR_STATE_TILE: states staged in LDS per tile of the denominator pass
FE_TILE = 4              # UPK_MBAR_FE_TILE: states per workgroup of the free-energy pass


def _bind(c):
    if getattr(c, '_mbar_bound', False):
        return
    vp, i32, i64, f64 = ct.c_void_p, ct.c_int, ct.c_longlong, ct.c_double
    c.upside_hip_mbar.argtypes = [i64, i32, i32, vp, vp, vp, vp, vp, vp, f64, i32, vp, i32, f64, vp, vp, vp, vp, vp, vp, vp]
    c.upside_hip_mbar.restype = i32
    c.upside_hip_last_error.restype = ct.c_char_p
    c._mbar_bound = True


def _ptr(a):
    return None if a is None else a.ctypes.data


def mbar(values, energy, beta, rows, n_k, periods=None, tol=1e-8, max_iter=10000, f0=None, target=None, want_denominators=True,
         library=None):
    """free energies f (K,) of K states from N samples, float64 on the device.
      values   (N, d) float32 CV values as recorded, d <= 8; None or (N, 0) for d = 0
      energy   (N,) unbiased potential, or None (= 0; it cancels when every beta is the same)
      beta     (K,) or a scalar for all states
      rows     (K, 3 d) = [center | spring_const | flat_width] per state: the cv_restraint per-system rows; None for d = 0
      n_k      (K,) samples drawn from each state, summing to N (the order of the samples does not matter)
      periods  (d,) period of each CV, 0 = not periodic (Ensemble.cv_periods, config.cv_periods); None: none is periodic
      tol, max_iter   stops when max |f' - f| < tol or after max_iter iterations (tol = 0: exactly max_iter); f0: the start, default 0
      target   None, or (beta_t, row_t) with row_t (3 d,) or None for no bias: the state to reweight to
    Returns dict(f, D (N,) the denominators of the returned f, n_iter, last_delta) and with a target also log_w (N,), the normalised
    log-weights of the samples in the target state, and f_target.  Every refusal of the entry point raises RuntimeError with its
    message."""
    from .engine import default_library
    lib = library if library is not None else default_library()
    c = lib.calc
    _bind(c)
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
