"""Analysis of metadynamics runs on the device (upside_hip_metad_bias and upside_hip_metad_grid of include/upside_engine_c.h;
csrc/kernels_metad.hip): the bias a list of hills puts on points and on product grids, the reweighting offset c(t) and the frame
weights of Tiwary & Parrinello 2015, and the sum-of-hills free energy.  With the hills h = 0 .. n - 1 of a list in deposit order,
    e_h(x) = exp(-1/2 sum_c wrap_c(x_c - s_hc)^2 / sigma_c^2)      (the nearest image of a hill in a periodic dimension, no others)
    V_m(x) = sum_{h < m} w_h e_h(x)                                the bias of the first m hills
    c(m)   = kT (ln sum_g exp(a V_m(g)) - ln sum_g exp(b V_m(g)))  over a grid g, b = 1 / kdT (0: plain), a = 1 / kT + b
    ln w_n = (V_{m_n}(s_n) - c(m_n)) / kT - logsumexp_n(...)       m_n = hills_visible(round of frame n, ...)
A frame recorded at completed round r was produced under the deposits of the rounds before r: the engine records the collective
variables of a completed round first and deposits afterwards.  Limits: d <= 4; a grid of at most 2^22 points; 2^24 hills per
list; c(t) is interpolated between max_checkpoints hill counts where a run has more distinct ones; the weights of plain
metadynamics (kdT = 0) are defined but do not converge in the long-time limit -- use well-tempered runs for reweighting.
The node computes with (double)(float)sigma and (double)(float)height: pass those rounded values (config.metad_node_parameters
returns them) when comparing with what a node applied."""
import ctypes as ct
import numpy as np

MAX_DIM = 4            # UPK_METAD_MAX_DIM
MAX_GRID = 1 << 22     # UPK_METAD_MAX_GRID
MAX_SCALES = 8         # UPK_METAD_MAX_SCALES


def _bind(c):
    if getattr(c, '_metad_bound', False):
        return
    vp, i32 = ct.c_void_p, ct.c_int
    c.upside_hip_metad_bias.argtypes = [i32, i32] + [vp] * 9
    c.upside_hip_metad_bias.restype = i32
    c.upside_hip_metad_grid.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp]
    c.upside_hip_metad_grid.restype = i32
    c.upside_hip_last_error.restype = ct.c_char_p
    c._metad_bound = True


def _starts(start, n, what):
    """a *_start array (n_list + 1,), or None for one list of n"""
    if start is None:
        return np.array([0, n], 'i8'), True
    s = np.ascontiguousarray(np.asarray(start).reshape(-1), 'i8')
    if len(s) < 2 or s[0] != 0 or s[-1] != n or (np.diff(s) < 0).any():
        raise ValueError('metad: %s must ascend from 0 to %d over n_list + 1 entries' % (what, n))
    return s, False


def _hills(centers, weights, sigma, periods, hill_start):
    sg = np.ascontiguousarray(np.asarray(sigma, 'f8').reshape(-1))
    d = len(sg)
    if not 1 <= d <= MAX_DIM:
        raise ValueError('metad: sigma holds %d entries, 1 to %d collective variables are supported' % (d, MAX_DIM))
    if not (np.isfinite(sg).all() and (sg > 0).all()):
        raise ValueError('metad: sigma must be finite and positive')
    per = np.zeros(d) if periods is None else np.ascontiguousarray(np.asarray(periods, 'f8').reshape(-1))
    if len(per) != d or not (np.isfinite(per).all() and (per >= 0).all()):
        raise ValueError('metad: periods must be %d finite numbers, not negative (0 = not periodic)' % d)
    w = np.ascontiguousarray(np.asarray(weights).reshape(-1), 'f4')
    c = np.asarray(centers)
    if c.ndim == 1 and d == 1:
        c = c[:, None]
    if c.shape != (len(w), d):
        raise ValueError('metad: centers must be (%d hills, %d CVs), got %r' % (len(w), d, c.shape))
    c = np.ascontiguousarray(c, 'f4')
    if not (np.isfinite(c).all() and np.isfinite(w).all()):
        raise ValueError('metad: centers and weights must be finite')
    hs, single = _starts(hill_start, len(w), 'hill_start')
    return c, w, sg, per, hs, single, d


_EMPTY = np.zeros(2, 'f8')


def _ptr(a):
    """the data pointer; an empty array still passes one (the entry points refuse NULL and read nothing through it)"""
    return a.ctypes.data if a.size else _EMPTY.ctypes.data


def _library(library):
    from .engine import default_library
    lib = library if library is not None else default_library()
    _bind(lib.calc)
    return lib.calc


def bias(centers, weights, sigma, points, n_visible=None, periods=None, hill_start=None, point_start=None, library=None):
    """V (N,) float64: V[i] = V_{n_visible[i]}(points[i]) over the hills of the point's own list, on the device.
      centers (H, d) (or (H,) for d = 1) and weights (H,): float32 hills in deposit order; sigma (d,), periods (d,) or None
      points (N, d) (or (N,) for d = 1) float64; n_visible (N,) or None: all hills of the list
      hill_start, point_start (n_list + 1,): where the hills and the points of each list begin; both None: one list
    A point without hills receives exactly 0.  Shape and value errors raise ValueError before the library is touched; a refusal
    of the entry point raises RuntimeError with its message."""
    c, w, sg, per, hs, single, d = _hills(centers, weights, sigma, periods, hill_start)
    x = np.asarray(points, 'f8')
    if x.ndim == 1 and d == 1:
        x = x[:, None]
    if x.ndim != 2 or x.shape[1] != d:
        raise ValueError('metad.bias: points must be (N, %d), got %r' % (d, x.shape))
    x = np.ascontiguousarray(x)
    if not np.isfinite(x).all():
        raise ValueError('metad.bias: points must be finite')
    ps, psingle = _starts(point_start, len(x), 'point_start')
    if len(ps) != len(hs):
        raise ValueError('metad.bias: hill_start names %d lists, point_start %d' % (len(hs) - 1, len(ps) - 1))
    nv = None
    if n_visible is not None:
        nv = np.ascontiguousarray(np.asarray(n_visible).reshape(-1), 'i8')
        if len(nv) != len(x):
            raise ValueError('metad.bias: %d n_visible for %d points' % (len(nv), len(x)))
        if len(nv) and (nv.min() < 0 or (nv > np.repeat(np.diff(hs), np.diff(ps))).any()):
            raise ValueError('metad.bias: n_visible must lie between 0 and the hills of the point\'s list')
    lib = _library(library)
    V = np.zeros(len(x), 'f8')
    rc = lib.upside_hip_metad_bias(len(hs) - 1, d, hs.ctypes.data, _ptr(c), _ptr(w), sg.ctypes.data, per.ctypes.data, ps.ctypes.data, _ptr(x),
                                   None if nv is None else _ptr(nv), _ptr(V))
    if rc:
        raise RuntimeError('metad.bias failed: %s' % lib.upside_hip_last_error().decode())
    return V


def _axes(axes, d):
    if d == 1 and len(axes) and np.ndim(axes[0]) == 0:
        axes = [axes]
    ax = [np.ascontiguousarray(np.asarray(a, 'f8').reshape(-1)) for a in axes]
    if len(ax) != d:
        raise ValueError('metad: %d axes for %d collective variables' % (len(ax), d))
    n_axis = np.array([len(a) for a in ax], 'i4')
    if (n_axis < 1).any():
        raise ValueError('metad: an axis holds at least one value')
    if int(np.prod(n_axis.astype('i8'))) > MAX_GRID:
        raise ValueError('metad: the grid holds %d points, at most 2^22 are supported' % int(np.prod(n_axis.astype('i8'))))
    flat = np.concatenate(ax)
    if not np.isfinite(flat).all():
        raise ValueError('metad: axis values must be finite')
    return ax, n_axis, flat


def bias_grid(centers, weights, sigma, axes, checkpoints=None, scales=(), periods=None, hill_start=None, want_V=True, library=None):
    """the bias on the product grid of `axes` (d arrays; the grid is shared by all lists), on the device.
      checkpoints  (K,) for one list or (n_list, K): ascending hill counts (repeats allowed); None: the whole list
      scales       (Q,), Q <= 8: lse[.., j, q] = ln sum_g exp(scales[q] V_{checkpoints[j]}(g)), the exact maximum taken off
    Returns dict(V: V_m(g) at the LAST checkpoint, shape n_axis (one list) or (n_list,) + n_axis, None without want_V; lse: (K, Q) or
    (n_list, K, Q), None without scales).  Errors as bias."""
    c, w, sg, per, hs, single, d = _hills(centers, weights, sigma, periods, hill_start)
    ax, n_axis, flat = _axes(axes, d)
    L = len(hs) - 1
    if checkpoints is None:
        ck = np.diff(hs)[:, None].copy()
    else:
        ck = np.asarray(checkpoints)
        ck = np.ascontiguousarray(ck[None, :] if ck.ndim == 1 else ck, 'i8')
    if ck.ndim != 2 or ck.shape[0] != L or ck.shape[1] < 1:
        raise ValueError('metad.bias_grid: checkpoints must be (%d lists, K >= 1), got %r' % (L, ck.shape))
    if ck.min() < 0 or (ck > np.diff(hs)[:, None]).any() or (np.diff(ck, axis=1) < 0).any():
        raise ValueError('metad.bias_grid: checkpoints must ascend within 0 .. the hills of their list')
    sc = np.ascontiguousarray(np.asarray(scales, 'f8').reshape(-1))
    if len(sc) > MAX_SCALES or not np.isfinite(sc).all():
        raise ValueError('metad.bias_grid: at most %d finite scales' % MAX_SCALES)
    if not want_V and not len(sc):
        raise ValueError('metad.bias_grid: nothing is asked for (no V, no scales)')
    lib = _library(library)
    G = int(np.prod(n_axis.astype('i8')))
    V = np.zeros((L, G), 'f8') if want_V else None
    lse = np.zeros((L, ck.shape[1], len(sc)), 'f8') if len(sc) else None
    rc = lib.upside_hip_metad_grid(L, d, hs.ctypes.data, _ptr(c), _ptr(w), sg.ctypes.data, per.ctypes.data, n_axis.ctypes.data, flat.ctypes.data,
                                   ck.shape[1], ck.ctypes.data, len(sc), sc.ctypes.data if len(sc) else None, None if V is None else V.ctypes.data,
                                   None if lse is None else lse.ctypes.data)
    if rc:
        raise RuntimeError('metad.bias_grid failed: %s' % lib.upside_hip_last_error().decode())
    if V is not None:
        V = V.reshape((L,) + tuple(int(n) for n in n_axis))
    return dict(V=V[0] if (single and V is not None) else V, lse=lse[0] if (single and lse is not None) else lse)


def hills_visible(rounds, pace, n_walker=1, n_initial=0, n_stored=None):
    """the hills a frame recorded at completed round `rounds` (>= 1; scalar or array) was produced under:
        min(n_initial + n_walker * floor((rounds - 1) / pace), n_stored)
    n_walker: the systems that deposit into a shared list (slot order k * n_system + s); n_initial: hills loaded before the run;
    n_stored (None: no clip): the hills the list holds, which clips where a list ran full."""
    r = np.asarray(rounds)
    if r.size and (r < 1).any():
        raise ValueError('hills_visible: a frame is recorded at a completed round, 1 or later')
    if int(pace) != pace or pace < 1:
        raise ValueError('hills_visible: pace must be a whole number of rounds, at least 1')
    if n_walker < 1 or n_initial < 0:
        raise ValueError('hills_visible: n_walker >= 1 and n_initial >= 0')
    m = int(n_initial) + int(n_walker) * ((r.astype('i8') - 1) // int(pace))
    if n_stored is not None:
        m = np.minimum(m, int(n_stored))
    return m if r.ndim else int(m)


def _offset_scales(kT, kdT):
    if not (np.ndim(kT) == 0 and np.isfinite(kT) and kT > 0):
        raise ValueError('metad: kT must be one finite positive number')
    if not (np.ndim(kdT) == 0 and np.isfinite(kdT) and kdT >= 0):
        raise ValueError('metad: kdT must be finite and not negative (0 = plain metadynamics)')
    b = 1. / float(kdT) if kdT > 0 else 0.
    return 1. / float(kT) + b, b


def reweighting_offset(centers, weights, sigma, axes, checkpoints, kT, kdT, periods=None, hill_start=None, library=None):
    """c at the checkpoints, (K,) or (n_list, K): c(m) = kT (ln sum_g exp(a V_m(g)) - ln sum_g exp(b V_m(g))) over the grid of `axes`,
    b = 1 / kdT (0 for plain metadynamics, kdT = 0), a = 1 / kT + b; arguments as bias_grid"""
    a, b = _offset_scales(kT, kdT)
    lse = bias_grid(centers, weights, sigma, axes, checkpoints, (a, b), periods, hill_start, want_V=False, library=library)['lse']
    return float(kT) * (lse[..., 0] - lse[..., 1])


def _logsumexp(x):
    m = x.max()
    return m + np.log(np.exp(x - m).sum())


def frame_log_weights_lists(centers, weights, sigma, frames, rounds, pace, kT, kdT, axes, hill_start=None, point_start=None, n_walker=1, n_initial=0,
                            periods=None, max_checkpoints=4096, library=None):
    """frame_log_weights for several lists in one bias call and one grid call: list l has the hills hill_start[l] .. and the frames
    point_start[l] .. (rounds per frame).  Returns one dict per list."""
    c, w, sg, per, hs, single, d = _hills(centers, weights, sigma, periods, hill_start)
    a, b = _offset_scales(kT, kdT)
    if int(max_checkpoints) < 2:
        raise ValueError('frame_log_weights: max_checkpoints must be at least 2')
    x = np.asarray(frames, 'f8')
    if x.ndim == 1 and d == 1:
        x = x[:, None]
    if x.ndim != 2 or x.shape[1] != d:
        raise ValueError('frame_log_weights: frames must be (N, %d), got %r' % (d, x.shape))
    r = np.asarray(rounds).reshape(-1)
    if len(r) != len(x):
        raise ValueError('frame_log_weights: %d rounds for %d frames' % (len(r), len(x)))
    ps, _ = _starts(point_start, len(x), 'point_start')
    if len(ps) != len(hs):
        raise ValueError('frame_log_weights: hill_start names %d lists, point_start %d' % (len(hs) - 1, len(ps) - 1))
    L = len(hs) - 1
    n_hill = np.diff(hs)
    if (np.diff(ps) < 1).any():
        raise ValueError('frame_log_weights: every list needs at least one frame')
    nv = np.concatenate([np.atleast_1d(hills_visible(r[ps[l]:ps[l + 1]], pace, n_walker, n_initial, n_hill[l])) for l in range(L)]).astype('i8')
    V = bias(c, w, sg, x, nv, per, hs, ps, library)
    # the checkpoints of a list: its distinct prefixes, thinned to max_checkpoints; one width for all lists (the last one repeated)
    cks = []
    for l in range(L):
        u = np.unique(nv[ps[l]:ps[l + 1]])
        if len(u) > int(max_checkpoints):
            u = u[np.unique(np.rint(np.linspace(0, len(u) - 1, int(max_checkpoints))).astype('i8'))]
        cks.append(u)
    K = max(len(u) for u in cks)
    ck = np.stack([np.concatenate((u, np.full(K - len(u), u[-1], 'i8'))) for u in cks])
    c_ck = np.atleast_2d(reweighting_offset(c, w, sg, axes, ck, kT, kdT, per, hs, library))
    out = []
    for l in range(L):
        m = nv[ps[l]:ps[l + 1]]
        c_n = np.interp(m, cks[l], c_ck[l, :len(cks[l])])      # (exact at a checkpoint; linear in the hill count between two)
        lw = (V[ps[l]:ps[l + 1]] - c_n) / float(kT)
        lw = lw - _logsumexp(lw)
        out.append(dict(log_w=lw, V=V[ps[l]:ps[l + 1]].copy(), c=c_n, n_visible=m.copy(), n_eff=float(1. / np.exp(2. * lw).sum()),
                        checkpoints=cks[l], c_checkpoints=c_ck[l, :len(cks[l])].copy()))
    return out


def frame_log_weights(centers, weights, sigma, frames, rounds, pace, kT, kdT, axes, n_walker=1, n_initial=0, periods=None, max_checkpoints=4096,
                      library=None):
    """the reweighting of recorded frames (Tiwary & Parrinello 2015) for one list of hills, on the device.
      frames (N, d): the biased CVs of the recorded frames; rounds (N,): the completed round each was recorded at
      pace, n_walker, n_initial: as hills_visible (the list's length clips); kT: the run's temperature; kdT: the node's (0 = plain)
      axes: the d grid axes c(t) is integrated over (default_axes gives a set that covers the hills)
    Returns dict(log_w (N,): normalised, logsumexp = 0; V (N,): the bias each frame felt; c (N,): the offset at each frame;
    n_visible (N,); n_eff: the Kish effective sample size 1 / sum w^2; checkpoints, c_checkpoints: the hill counts c was evaluated
    at).  The checkpoints are the distinct n_visible; where there are more than max_checkpoints they are thinned to that many,
    evenly, and c is interpolated linearly in the hill count between them: an APPROXIMATION, whose error falls with the hill
    weights and is absent when max_checkpoints covers the run."""
    return frame_log_weights_lists(centers, weights, sigma, frames, rounds, pace, kT, kdT, axes, None, None, n_walker, n_initial, periods,
                                   max_checkpoints, library)[0]


def free_energy_grid(centers, weights, sigma, axes, kT=None, kdT=0., periods=None, hill_start=None, library=None):
    """the sum-of-hills free energy on the grid of `axes`, on the device, up to a constant: -V (plain, kdT = 0) or
    -(kT + kdT) / kdT V (well-tempered); what config.metadynamics_free_energy gives on the host for small inputs"""
    if kdT < 0.:
        raise ValueError('free_energy_grid: kdT must not be negative')
    if kdT > 0. and (kT is None or not kT > 0.):
        raise ValueError('free_energy_grid: well-tempered (kdT > 0) needs kT > 0')
    V = bias_grid(centers, weights, sigma, axes, None, (), periods, hill_start, library=library)['V']
    return -(float(kT) + float(kdT)) / float(kdT) * V if kdT > 0. else -V


def default_axes(centers, sigma, periods=None, n=64):
    """d axes of n points each that cover the hills: in a dimension that is not periodic, n points over [min - 3 sigma, max + 3 sigma]
    of the centres; in a periodic one, n points over one period from -period / 2, the duplicated end left out"""
    sg = np.asarray(sigma, 'f8').reshape(-1)
    d = len(sg)
    c = np.asarray(centers, 'f8')
    c = c[:, None] if (c.ndim == 1 and d == 1) else c
    if c.ndim != 2 or c.shape[1] != d or not len(c):
        raise ValueError('default_axes: centers must be (at least one hill, %d)' % d)
    per = np.zeros(d) if periods is None else np.asarray(periods, 'f8').reshape(-1)
    if len(per) != d or int(n) < 1:
        raise ValueError('default_axes: periods must hold %d entries and n >= 1' % d)
    return [(-0.5 * per[k] + per[k] * np.arange(int(n)) / int(n)) if per[k] > 0 else
            np.linspace(c[:, k].min() - 3. * sg[k], c[:, k].max() + 3. * sg[k], int(n)) for k in range(d)]


def reweighted_profile(log_w, values, bins, kT):
    """(F (n_bin,), edges (n_bin + 1,)): F = -kT ln of the weighted histogram of `values` (any observable of the frames, one per
    frame) with weights exp(log_w), on the host; bins: as numpy.histogram takes them.  An empty bin is +inf."""
    lw = np.asarray(log_w, 'f8').reshape(-1)
    v = np.asarray(values, 'f8').reshape(-1)
    if len(lw) != len(v) or not len(v):
        raise ValueError('reweighted_profile: %d weights for %d values' % (len(lw), len(v)))
    if not (np.ndim(kT) == 0 and kT > 0):
        raise ValueError('reweighted_profile: kT must be positive')
    h, edges = np.histogram(v, bins=bins, weights=np.exp(lw - lw.max()))
    with np.errstate(divide='ignore'):
        return -float(kT) * np.log(h / h.sum()), edges
