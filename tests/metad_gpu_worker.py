"""Child process of tests/test_gpu_metad.py: one check of the metadynamics analysis on the device (upside_hip_metad_bias,
upside_hip_metad_grid, csrc/kernels_metad.hip; metad.py; Ensemble.metad_reweight) per invocation,

    python tests/metad_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is tests/metad_reference.py
(float64 numpy, pinned by tests/test_metad_config.py); the inputs are tests/metad_cases.py.  Bounds, with A = sum |w_h| e_h:
    |V - V_ref| <= 1e-11 A          |lse - lse_ref| <= 1e-11 + 1e-11 |scale| max_g A(g)
Both sides are fp64: sums of at most about 10^3 terms carry about 1e-13 and an exponent of up to 128 carries 4e-14, which leaves two
orders of margin.  Points lie within 8 sigma of some hill."""
import ctypes as ct
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                  # noqa: E402
import metad_cases as C                  # noqa: E402
import metad_reference as R              # noqa: E402

pkg = P.pkg
E = pkg.engine
metad = pkg.metad
BOUND = 1e-11


class Hills(ct.Structure):
    _fields_ = [('n_list', ct.c_int), ('d', ct.c_int)] + [(k, ct.c_void_p) for k in ('hill_start', 'centers', 'weights', 'sigma', 'periods')]


class GridProblem(ct.Structure):
    _fields_ = [('H', Hills), ('n_axis', ct.c_void_p), ('axes', ct.c_void_p), ('n_checkpoint', ct.c_int), ('checkpoints', ct.c_void_p),
                ('n_scale', ct.c_int), ('scales', ct.c_void_p), ('V_last', ct.c_void_p), ('lse', ct.c_void_p), ('workspace_limit', ct.c_size_t),
                ('path', ct.c_int), ('stats', ct.c_void_p)]


def raw_grid(c, w, hs, sigma, per, axes, ck, scales, workspace_limit=0, path=0):
    """upk_metad_grid_solve with the two arguments the public entry point does not pass on: (V (L, G), lse (L, K, Q), stats)"""
    lib = pkg.default_library().calc
    lib.upk_metad_grid_solve.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int]
    c = np.ascontiguousarray(c, 'f4'); w = np.ascontiguousarray(w, 'f4'); hs = np.ascontiguousarray(hs, 'i8')
    sg = np.ascontiguousarray(sigma, 'f8'); per = np.ascontiguousarray(per, 'f8')
    n_axis = np.array([len(a) for a in axes], 'i4'); flat = np.ascontiguousarray(np.concatenate(axes), 'f8')
    ck = np.ascontiguousarray(ck, 'i8'); sc = np.ascontiguousarray(scales, 'f8')
    L, K, G = len(hs) - 1, ck.shape[1], int(np.prod(n_axis))
    V = np.zeros((L, G)); lse = np.zeros((L, K, len(sc))); stats = np.zeros(6)
    keep = np.zeros(2, 'f4')
    Pm = GridProblem()
    Pm.H = Hills(L, len(sg), hs.ctypes.data, c.ctypes.data if c.size else keep.ctypes.data, w.ctypes.data if w.size else keep.ctypes.data, sg.ctypes.data, per.ctypes.data)
    Pm.n_axis = n_axis.ctypes.data; Pm.axes = flat.ctypes.data; Pm.n_checkpoint = K; Pm.checkpoints = ck.ctypes.data
    Pm.n_scale = len(sc); Pm.scales = sc.ctypes.data; Pm.V_last = V.ctypes.data; Pm.lse = lse.ctypes.data
    Pm.workspace_limit = workspace_limit; Pm.path = path; Pm.stats = stats.ctypes.data
    msg = ct.create_string_buffer(256)
    rc = lib.upk_metad_grid_solve(ct.byref(Pm), msg, 256)
    assert rc == 0, msg.value
    return V, lse, stats


def ratio_V(got, ref, A):
    """largest |got - ref| / (1e-11 A); where A = 0 the value must be exactly 0"""
    got = np.asarray(got).reshape(-1); ref = np.asarray(ref).reshape(-1); A = np.asarray(A).reshape(-1)
    zero = A == 0.
    assert not got[zero].any(), 'a point without hills is not exactly 0'
    return float((np.abs(got - ref)[~zero] / (BOUND * A[~zero])).max()) if (~zero).any() else 0.


def ratio_lse(got, ref, scales, A_max):
    """largest |got - ref| / (1e-11 + 1e-11 |scale| max_g A); got, ref (K, Q), A_max (K,)"""
    bound = BOUND + BOUND * np.abs(np.asarray(scales))[None, :] * np.asarray(A_max)[:, None]
    return float((np.abs(got - ref) / bound).max())


def lists_case(d, n_list, seed, periodic):
    """unequal lists with their points: (c, w, hs, x, ps)"""
    c, w, hs = C.unequal_lists(d, n_list, seed, periodic)
    if n_list == 1:
        c, w = C.hills(d, 1000, seed, periodic); hs = np.array([0, 1000], 'i8')
    xs = [C.points_near(c[hs[l]:hs[l + 1]], C.POINT_COUNTS[(2 * l + seed) % len(C.POINT_COUNTS)], 7 * seed + l, d, periodic) for l in range(n_list)]
    return c, w, hs, np.concatenate(xs), np.concatenate(([0], np.cumsum([len(x) for x in xs]))).astype('i8')


def reference_bias(c, w, hs, x, ps, sg, per, nv):
    V = np.zeros(len(x)); A = np.zeros(len(x))
    for l in range(len(hs) - 1):
        sl = slice(ps[l], ps[l + 1])
        V[sl], A[sl] = R.bias(x[sl], c[hs[l]:hs[l + 1]], w[hs[l]:hs[l + 1]], sg, per, None if nv is None else nv[sl])
    return V, A


def visible_modes(hs, ps, seed):
    """n_visible: None, all 0, ascending within each list, shuffled"""
    rng = np.random.RandomState(seed)
    n_h = np.repeat(np.diff(hs), np.diff(ps))
    asc = np.concatenate([np.sort(rng.randint(0, hs[l + 1] - hs[l] + 1, size=ps[l + 1] - ps[l])) for l in range(len(hs) - 1)]).astype('i8')
    return (('all hills', None), ('no hills', np.zeros(len(n_h), 'i8')), ('ascending', asc), ('shuffled', rng.randint(0, n_h + 1).astype('i8')))


def bias(work):
    worst = 0.; n_call = 0; seen_h = set(); seen_p = set()
    for d in (1, 2, 3, 4):
        for n_list in C.LIST_COUNTS:
            for periodic in ((False, True) if n_list == 3 else (d == 2,)):
                c, w, hs, x, ps = lists_case(d, n_list, 10 * d + n_list, periodic)
                sg, per = C.SIGMA[:d], C.periods_of(d, periodic)
                seen_h.update(np.diff(hs).tolist()); seen_p.update(np.diff(ps).tolist())
                for what, nv in visible_modes(hs, ps, d + n_list):
                    ref, A = reference_bias(c, w, hs, x, ps, sg, per, nv)
                    got = metad.bias(c, w, sg, x, nv, per, hs, ps)
                    n_call += 1
                    r = ratio_V(got, ref, A)
                    worst = max(worst, r)
                    print('d = %d, %2d lists (%5d hills, %5d points)%s, n_visible %-9s: largest |V - f64| / (1e-11 A) = %.3e' %
                          (d, n_list, len(w), len(x), ', periodic' if periodic else '', what, r))
                    assert r <= 1. and np.isfinite(got).all()
                    if what == 'no hills':
                        assert not got.any()
    # one list passed without the *_start arrays; a list of no hills at all
    c, w = C.hills(2, 257, 5)
    x = C.points_near(c, 300, 6, 2)
    ref, A = R.bias(x, c, w, C.SIGMA[:2])
    got = metad.bias(c, w, C.SIGMA[:2], x)
    none = metad.bias(c[:0], w[:0], C.SIGMA[:2], x)
    print('one list without *_start: ratio %.3e; no hills: largest |V| %r; negative weights among the hills: %d; negative V: %d' %
          (ratio_V(got, ref, A), float(np.abs(none).max()), int((w < 0).sum()), int((got < 0).sum())))
    assert ratio_V(got, ref, A) <= 1. and not none.any() and (w < 0).any() and (got < 0).any()
    print('%d calls, worst ratio %.3e (bound 1); hill counts seen %s; point counts seen %s' % (n_call, worst, sorted(seen_h), sorted(seen_p)))
    assert seen_h >= set(C.HILL_COUNTS) and seen_p >= set(C.POINT_COUNTS)


def checkpoints_of(n):
    """0, a count that is no multiple of 4, the same again, two thirds (odd), and one below the list's length"""
    return np.sort(np.minimum([0, 3, 3, (2 * n // 3) | 1, max(n - 1, 0)], n)).astype('i8')


GRID_SHAPES = ([(n,) for n in C.AXIS_SIZES] +
               [(1, 100), (100, 1), (15, 17), (16, 64), (17, 63), (63, 65), (64, 16), (65, 15), (100, 100), (8, 8), (7, 100)] +
               [(5, 13, 17), (1, 16, 15), (3, 5, 7, 9), (4, 4, 4, 4), (2, 3, 5, 1)])


def grid_case(shape, i, periodic, counts=None):
    d = len(shape)
    counts = counts if counts is not None else [C.HILL_COUNTS[(3 * i + k * 5) % len(C.HILL_COUNTS)] for k in range(3)]
    parts = [C.hills(d, n, 50 * i + k, periodic) for k, n in enumerate(counts)]
    c = np.concatenate([p[0] for p in parts]).reshape(-1, d); w = np.concatenate([p[1] for p in parts])
    hs = np.concatenate(([0], np.cumsum(counts))).astype('i8')
    ck = np.stack([checkpoints_of(n) for n in counts])
    return c, w, hs, ck, C.axes_over(d, shape, periodic)


def check_grid(shape, c, w, hs, ck, axes, per, label, path=0, with_bias=True):
    """the public entry point (path 0) or the internal solve with a forced path against the yardstick; returns the worst ratios"""
    d = len(shape)
    sg = C.SIGMA[:d]
    if path == 0:
        got = metad.bias_grid(c, w, sg, axes, ck, C.SCALES, per, hs)
        V, lse = got['V'].reshape(len(hs) - 1, -1), got['lse']
        only = metad.bias_grid(c, w, sg, axes, ck, C.SCALES, per, hs, want_V=False)
        assert only['V'] is None and only['lse'].tobytes() == lse.tobytes(), 'V_last NULL changes lse'
        taken = raw_grid(c, w, hs, sg, per, axes, ck, C.SCALES)[2][4]
    else:
        V, lse, stats = raw_grid(c, w, hs, sg, per, axes, ck, C.SCALES, path=path)
        taken = stats[4]
    rv = rl = rb = 0.
    g = R.grid_points(axes)
    for l in range(len(hs) - 1):
        ref = R.bias_grid(axes, c[hs[l]:hs[l + 1]], w[hs[l]:hs[l + 1]], sg, per, ck[l], C.SCALES)
        rv = max(rv, ratio_V(V[l], ref['V'][-1], ref['A'][-1]))
        rl = max(rl, ratio_lse(lse[l], ref['lse'], C.SCALES, ref['A'].max(axis=1)))
        assert abs(lse[l, 0, 0] - np.log(len(g))) <= 1e-14 and np.abs(lse[l, :, 0] - np.log(len(g))).max() <= BOUND      # checkpoint 0, scale 0
        if with_bias:
            direct = metad.bias(c[hs[l]:hs[l + 1]], w[hs[l]:hs[l + 1]], sg, g, np.full(len(g), ck[l, -1]), per)
            rb = max(rb, ratio_V(V[l], direct, ref['A'][-1]))
    print('%-22s %s, hills %s, path %d: V ratio %.3e, lse ratio %.3e, V against upside_hip_metad_bias %.3e (bound 1)' %
          (label, 'x'.join(str(n) for n in shape), np.diff(hs).tolist(), int(taken), rv, rl, rb))
    assert rv <= 1. and rl <= 1. and rb <= 1. and np.isfinite(V).all() and np.isfinite(lse).all()
    return int(taken)


def grid(work):
    seen = set(); paths = set()
    for i, shape in enumerate(GRID_SHAPES):
        periodic = i % 3 == 1
        c, w, hs, ck, axes = grid_case(shape, i, periodic)
        seen.update(np.diff(hs).tolist())
        paths.add(check_grid(shape, c, w, hs, ck, axes, C.periods_of(len(shape), periodic), 'periodic' if periodic else ''))
    assert seen >= set(C.HILL_COUNTS) and paths == {1, 2}, (sorted(seen), paths)
    # the other path at shapes that the routing sends elsewhere: the direct sum for d >= 2, the factorised sum on thin grids
    for shape, path in (((17, 63), 1), ((5, 13, 17), 1), ((3, 5, 7, 9), 1), ((1, 100), 2), ((7, 100), 2), ((2, 3, 5, 1), 2)):
        c, w, hs, ck, axes = grid_case(shape, 40 + len(shape), False, [257, 0, 1000])
        assert check_grid(shape, c, w, hs, ck, axes, np.zeros(len(shape)), 'forced', path, with_bias=False) == path
    # more hills in a segment than a slab holds (512 for 4000 x 8: 63 tiles, 8 partial ranges), and a grid of 272 tiles (no partials)
    for shape, counts in (((4000, 8), [600]), ((1030, 1000), [17])):
        c, w, hs, ck, axes = grid_case(shape, 60, False, counts)
        assert check_grid(shape, c, w, hs, ck, axes, np.zeros(2), 'large', with_bias=False) == 2


def reproducible(work):
    for shape, few in (((33, 20), 9000000), ((50,), 2000), ((5, 13, 17), 9000000)):      # few: a workspace that holds a few lists
        d = len(shape)
        sg, per = C.SIGMA[:d], C.periods_of(d, d == 2)
        c, w, hs = C.unequal_lists(d, 65, 3, d == 2)
        # list 0 gets 1000 hills, so that it is worth comparing
        c0, w0 = C.hills(d, 1000, 99, d == 2)
        c = np.concatenate((c0, c[hs[1]:])); w = np.concatenate((w0, w[hs[1]:])); hs = np.concatenate(([0], hs[1:] - hs[1] + 1000)).astype('i8')
        ck = np.stack([checkpoints_of(n) for n in np.diff(hs)])
        axes = C.axes_over(d, shape, d == 2)
        one = raw_grid(c, w, hs, sg, per, axes, ck, C.SCALES); two = raw_grid(c, w, hs, sg, per, axes, ck, C.SCALES)
        small = raw_grid(c, w, hs, sg, per, axes, ck, C.SCALES, workspace_limit=1)
        three = raw_grid(c, w, hs, sg, per, axes, ck, C.SCALES, workspace_limit=few)
        alone = raw_grid(c[:1000], w[:1000], hs[:2], sg, per, axes, ck[:1], C.SCALES)
        order = [1, 2, 0]
        cl = np.concatenate([c[hs[l]:hs[l + 1]] for l in order]); wl = np.concatenate([w[hs[l]:hs[l + 1]] for l in order])
        hl = np.concatenate(([0], np.cumsum([hs[l + 1] - hs[l] for l in order]))).astype('i8')
        last = raw_grid(cl, wl, hl, sg, per, axes, ck[order], C.SCALES)
        s = dict(two_calls=one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes(),
                 chunks_of_one=small[0].tobytes() == one[0].tobytes() and small[1].tobytes() == one[1].tobytes(),
                 chunks_of_few=three[0].tobytes() == one[0].tobytes() and three[1].tobytes() == one[1].tobytes(),
                 alone=alone[0][0].tobytes() == one[0][0].tobytes() and alone[1][0].tobytes() == one[1][0].tobytes(),
                 last_of_3=last[0][2].tobytes() == one[0][0].tobytes() and last[1][2].tobytes() == one[1][0].tobytes())
        print('grid %s, 65 lists, path %d: chunks %d / %d / %d; %s' % ('x'.join(map(str, shape)), int(one[2][4]), int(one[2][5]), int(small[2][5]), int(three[2][5]), s))
        assert all(s.values()) and one[2][5] == 1 and small[2][5] == 65 and 1 < three[2][5] < 65 and one[0].any()
        # the bias at points
        xs = [C.points_near(c[hs[l]:hs[l + 1]], 257 if l else 1000, l, d, d == 2) for l in range(65)]
        ps = np.concatenate(([0], np.cumsum([len(x) for x in xs]))).astype('i8')
        x = np.concatenate(xs)
        nv = visible_modes(hs, ps, 4)[3][1]
        b1 = metad.bias(c, w, sg, x, nv, per, hs, ps); b2 = metad.bias(c, w, sg, x, nv, per, hs, ps)
        ba = metad.bias(c[:1000], w[:1000], sg, xs[0], nv[:1000], per)
        pl = np.concatenate(([0], np.cumsum([len(xs[l]) for l in order]))).astype('i8')
        bl = metad.bias(cl, wl, sg, np.concatenate([xs[l] for l in order]), np.concatenate([nv[ps[l]:ps[l + 1]] for l in order]), per, hl, pl)
        s = dict(two_calls=b1.tobytes() == b2.tobytes(), alone=ba.tobytes() == b1[:1000].tobytes(), last_of_3=bl[pl[2]:].tobytes() == b1[:1000].tobytes())
        print('bias at %d points of 65 lists, d = %d: %s' % (len(x), d, s))
        assert all(s.values()) and b1.any()


def end_to_end(work):
    import cv_restraint_cases as K
    from cv_metad_gpu_worker import make, NODE, NAME
    cfg = pkg.config
    native = K.coords(NAME)
    ca = np.arange(1, len(native), 3, dtype='i4')
    dist = {'name': 'd_ee', 'kind': 'distance', 'pair': (int(ca[0]), int(ca[-1]))}
    rg = {'name': 'rg_ca', 'kind': 'rg', 'atoms': ca}
    extra = {'name': 'rg_all', 'kind': 'rg', 'atoms': np.arange(len(native), dtype='i4')}
    sigma, height, kdT, kT, pace, S, n_round = (0.5, 0.2), 0.3, 2.0, 0.8, 2, 4, 60
    for shared in (False, True):
        path = make(work, 'rew%d' % shared, [dist, rg], sigma, False, height=height, pace=pace, capacity=(n_round // pace) * (S if shared else 1), kdT=kdT, shared=shared)
        p = cfg.metad_node_parameters(path, NODE)
        assert p['names'] == ['d_ee', 'rg_ca'] and p['pace'] == pace and p['shared'] == shared and p['kdT'] == kdT
        assert p['sigma'].tolist() == np.asarray(sigma, 'f4').astype('f8').tolist() and p['height'] == float(np.float32(height))
        ens = E.Ensemble(path, S)
        ens.set_pos(native.astype('f4'))
        ens.init_md(kT, 21)
        ens.define_cvs([rg, extra, dist])      # (another order than the node's: the columns are found by name)
        ens.record_cvs(1, n_round)
        ens.run_rounds(n_round)
        series = ens.read_cvs(reset=False)
        assert series.shape == (n_round, S, 3)
        got = ens.metad_reweight(NODE, kT)
        frames = series[:, :, [2, 0]].astype('f8')
        rounds = np.arange(1, n_round + 1)
        n_dep = n_round // pace
        worst = dict(V=0., c=0., lw=0., w=0.)
        lists = [ens.metad_hills(NODE, 0)] if shared else [ens.metad_hills(NODE, s) for s in range(S)]
        outs = [got] if shared else got
        assert len(outs) == len(lists)
        for l, (o, (c, w, na)) in enumerate(zip(outs, lists)):
            assert len(w) == n_dep * (S if shared else 1) and na == n_dep
            x = frames.reshape(-1, 2) if shared else frames[:, l]
            r = np.repeat(rounds, S) if shared else rounds
            ref = R.frame_log_weights(c, w, p['sigma'], x, r, pace, kT, kdT, o['axes'], n_walker=S if shared else 1, periods=p['periods'])
            a, b = R.offset_scales(kT, kdT)
            c_bound = kT * ((BOUND + BOUND * a * ref['A_grid_max']) + (BOUND + BOUND * b * ref['A_grid_max']))      # at the checkpoints
            c_bound_n = c_bound[np.searchsorted(ref['checkpoints'], ref['n_visible'])]
            lw_bound = 2. * ((BOUND * ref['A'] + c_bound_n) / kT).max() + 1e-13
            assert np.array_equal(o['n_visible'], ref['n_visible']) and np.array_equal(o['checkpoints'], ref['checkpoints'])
            worst['V'] = max(worst['V'], ratio_V(o['V'], ref['V'], ref['A']))
            worst['c'] = max(worst['c'], float((np.abs(o['c_checkpoints'] - ref['c_checkpoints']) / c_bound).max()))
            worst['lw'] = max(worst['lw'], float(np.abs(o['log_w'] - ref['log_w']).max() / lw_bound))
            assert abs(R.logsumexp(o['log_w'])) <= 1e-12 and abs(o['n_eff'] - ref['n_eff']) <= 1e-9 * ref['n_eff'] and np.array_equal(o['c'], o['c_checkpoints'][np.searchsorted(o['checkpoints'], o['n_visible'])])
            # at a deposit round the frame is the hill's centre, and the bias it felt is what the engine made the hill's weight of
            for k in range(n_dep):
                for s in (range(S) if shared else (l,)):
                    f = (pace * (k + 1) - 1) * S + s if shared else pace * (k + 1) - 1      # the frame of round pace (k + 1)
                    h = k * S + s if shared else k
                    fx = series[pace * (k + 1) - 1, s, [2, 0]]
                    assert fx.tobytes() == c[h].tobytes(), 'frame %d of system %d is not the centre of hill %d' % (f, s, h)
                    assert o['n_visible'][f] == (k * S if shared else k)
                    miss = abs(o['V'][f] + kdT * np.log(float(w[h]) / p['height'])) / (2e-7 * kdT + BOUND * ref['A'][f])
                    worst['w'] = max(worst['w'], float(miss))
            print('%s list %d: %d hills, %d frames, n_eff %.2f of %d; c from %.4f to %.4f' % ('shared' if shared else 'own', l, len(w), len(x), o['n_eff'], len(x),
                                                                                              o['c_checkpoints'][0], o['c_checkpoints'][-1]))
        print('shared = %s: largest ratios to the bounds: V %.3e, c %.3e, log_w %.3e, V + kdT ln(w / height) at the deposit rounds %.3e (bound 1)' %
              (shared, worst['V'], worst['c'], worst['lw'], worst['w']))
        assert max(worst.values()) <= 1.
        # a CV of the node that is not recorded
        ens.define_cvs([rg, extra])
        try:
            ens.metad_reweight(NODE, kT, series=series[:, :, :2])
        except ValueError as err:
            print('not recorded: %s' % err)
            assert 'd_ee' in str(err)
        else:
            raise AssertionError('a CV that is not recorded was accepted')
        ens.close()


def refusals(work):
    lib = pkg.default_library().calc
    metad._bind(lib)
    d = 2
    c, w, hs = C.unequal_lists(d, 3, 1)
    sg = np.ascontiguousarray(C.SIGMA[:d]); per = np.array([0., 6.25])
    x = C.points_near(c, 10, 2, d); ps = np.array([0, 4, 4, 10], 'i8'); nv = np.zeros(10, 'i8'); V = np.zeros(10)
    axes = C.axes_over(d, (9, 12)); n_axis = np.array([9, 12], 'i4'); flat = np.concatenate(axes)
    ck = np.zeros((3, 2), 'i8'); sc = np.array([1., -2.5]); Vg = np.zeros((3, 108)); lse = np.zeros((3, 2, 2))
    before_b = metad.bias(c, w, sg, x, None, per, hs, ps)
    before_g = metad.bias_grid(c, w, sg, axes, None, sc, per, hs)

    def good_bias():
        return [3, d, hs, c, w, sg, per, ps, x, nv, V]

    def good_grid():
        return [3, d, hs, c, w, sg, per, n_axis, flat, 2, ck, 2, sc, Vg, lse]

    def call(fn, args):
        keep = [np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a for a in args]
        rc = fn(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in keep])
        return rc, lib.upside_hip_last_error().decode()

    def changed(a, at, value):
        b = np.array(a, copy=True); b.reshape(-1)[at] = value
        return b
    big = np.arange(130, dtype='i8') << 24
    hills_cases = [('d = 0', 1, 0, 'd = 0'), ('d = 5', 1, 5, 'd = 5'), ('n_list = 0', 0, 0, 'n_list = 0'), ('hill_start NULL', 2, None, 'must be given'),
                   ('centers NULL', 3, None, 'must be given'), ('weights NULL', 4, None, 'must be given'), ('sigma NULL', 5, None, 'must be given'),
                   ('periods NULL', 6, None, 'must be given'), ('hill_start from 1', 2, changed(hs, 0, 1), 'hill_start[0] = 1'),
                   ('hill_start descending', 2, changed(hs, 1, hs[2] + 1), 'descends'), ('a list above 2^24', 2, np.array([0, (1 << 24) + 1, (1 << 24) + 1, (1 << 24) + 1], 'i8'), 'at most 2^24'),
                   ('sigma NaN', 5, changed(sg, 1, np.nan), 'sigma[1] is not finite'), ('sigma 0', 5, changed(sg, 0, 0.), 'sigma[0] = 0 is not positive'),
                   ('period inf', 6, changed(per, 0, np.inf), 'periods[0] is not finite'), ('period negative', 6, changed(per, 1, -1.), 'periods[1] is negative'),
                   ('a centre NaN', 3, changed(c, 5, np.nan), 'hill 2, CV 1 is not finite'), ('a weight inf', 4, changed(w, 3, np.inf), 'weights[3] is not finite')]
    bias_cases = hills_cases + [('point_start NULL', 7, None, 'must be given'), ('points NULL', 8, None, 'must be given'), ('V NULL', 10, None, 'must be given'),
                                ('point_start from 2', 7, changed(ps, 0, 2), 'point_start[0] = 2'), ('point_start descending', 7, changed(ps, 2, 3), 'descends'),
                                ('2^31 points', 7, np.array([0, 1 << 31, 1 << 31, 1 << 31], 'i8'), 'fewer than 2^31'), ('a point NaN', 8, changed(x, 19, np.nan), 'point 9, CV 1 is not finite'),
                                ('n_visible -1', 9, changed(nv, 2, -1), 'n_visible[2] = -1'), ('n_visible above its list', 9, changed(nv, 9, hs[3] - hs[2] + 1), 'n_visible[9]')]
    grid_cases = hills_cases + [('n_axis NULL', 7, None, 'must be given'), ('axes NULL', 8, None, 'must be given'), ('checkpoints NULL', 10, None, 'must be given'),
                                ('scales NULL', 12, None, 'scales must be given'), ('lse NULL', 14, None, 'lse must be given exactly'), ('n_checkpoint 0', 9, 0, 'n_checkpoint = 0'),
                                ('n_scale -1', 11, -1, 'n_scale = -1'), ('n_scale 9', 11, 9, 'n_scale = 9'), ('n_axis 0', 7, np.array([9, 0], 'i4'), 'n_axis[1] = 0'),
                                ('G above 2^22', 7, np.array([2048, 2049], 'i4'), 'more than 2^22'), ('an axis value NaN', 8, changed(flat, 20, np.nan), 'axes[20] is not finite'),
                                ('a scale inf', 12, changed(sc, 1, np.inf), 'scales[1] is not finite'), ('a checkpoint -1', 10, changed(ck, 0, -1), 'checkpoint 0 of list 0 = -1'),
                                ('a checkpoint above its list', 10, changed(ck, 3, 1), 'checkpoint 1 of list 1 = 1, the list holds 0 hills'),
                                ('checkpoints descending', 10, changed(ck, 4, 1), 'descends')]
    n = 0
    for name, fn, good, cases in (('metad_bias', lib.upside_hip_metad_bias, good_bias, bias_cases), ('metad_grid', lib.upside_hip_metad_grid, good_grid, grid_cases)):
        for label, at, value, fragment in cases:
            args = good(); args[at] = value
            rc, msg = call(fn, args)
            print('%-11s %-28s refused: %s' % (name, label, msg))
            assert rc == 1 and fragment in msg and msg.startswith(name + ': '), (label, msg)
            n += 1
        # 2^31 hills in total: 129 lists of 2^24, refused before an array of hills is read
        args = good(); args[0] = 129; args[2] = big
        rc, msg = call(fn, args)
        print('%-11s %-28s refused: %s' % (name, '2^31 hills in total', msg))
        assert rc == 1 and 'fewer than 2^31' in msg
        n += 1
    after_b = metad.bias(c, w, sg, x, None, per, hs, ps)
    after_g = metad.bias_grid(c, w, sg, axes, None, sc, per, hs)
    assert after_b.tobytes() == before_b.tobytes() and after_g['V'].tobytes() == before_g['V'].tobytes() and after_g['lse'].tobytes() == before_g['lse'].tobytes()
    assert before_b.any() and before_g['V'].any()
    print('%d refusals; good calls after them return the bits of the ones before' % n)


def cli(work):
    """tools/metad_reweight.py on the output of an `upside_hip` run: F_hills and the reweighted profile along a CV that was not biased"""
    import subprocess
    import cv_restraint_cases as K
    from cv_metad_gpu_worker import make, NODE, NAME, run_cli
    cfg = pkg.config
    native = K.coords(NAME)
    ca = np.arange(1, len(native), 3, dtype='i4')
    dist = {'name': 'd_ee', 'kind': 'distance', 'pair': (int(ca[0]), int(ca[-1]))}
    rg = {'name': 'rg_ca', 'kind': 'rg', 'atoms': ca}
    extra = {'name': 'rg_all', 'kind': 'rg', 'atoms': np.arange(len(native), dtype='i4')}
    sigma, height, kdT, kT, pace = (0.5, 0.2), 0.3, 2.0, 0.8, 2
    path = make(work, 'tool', [dist, rg], sigma, False, height=height, pace=pace, capacity=40, kdT=kdT)
    cfg.add_collective_variables(path, [rg, extra, dist])
    run_cli(['--duration', '0.648', '--frame-interval', '0.054', '--seed', '3', '--temperature', str(kT), path])      # 24 rounds of 3 x 0.009, a frame every 2
    with pkg.h5lite.open_file(path) as t:
        out = t.group('output')
        series = out.read('cv', 'f4').reshape(-1, 3)
        m = out.group('metadynamics/' + NODE)
        w = m.read('hill_weight', 'f4').ravel(); c = m.read('hill_center', 'f4').reshape(len(w), 2)
        del m, out
    print('%d frames, %d hills' % (len(series), len(w)))
    assert len(series) == 12 and len(w) == 12      # (a frame is taken at the start of rounds 0, 2, .. 22)
    for f in range(1, 12):      # frame f is completed round 2 f, where hill f - 1 was deposited
        assert series[f, [2, 0]].tobytes() == c[f - 1].tobytes(), 'frame %d is not the centre of hill %d' % (f, f - 1)
    tool = os.path.join(P.ROOT, 'tools', 'metad_reweight.py')
    r = subprocess.run([sys.executable, tool, path, '--node', NODE, '--temperature', str(kT), '--every', '2', '--along', 'rg_all', '--bins', '4', '--grid', '12'],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    text = r.stdout.decode()
    print(text[-1500:])
    assert r.returncode == 0
    lines = text.splitlines()
    at_f = next(i for i, ln in enumerate(lines) if ln.startswith('# F_hills'))
    at_p = next(i for i, ln in enumerate(lines) if ln.startswith('# reweighted profile'))
    F = np.array([[float(x) for x in ln.split()] for ln in lines[at_f + 1:at_p]])
    prof = np.array([[float(x) for x in ln.split()] for ln in lines[at_p + 1:] if ln and not ln.startswith('#')])
    p = cfg.metad_node_parameters(path, NODE)
    axes = metad.default_axes(c, p['sigma'], p['periods'], n=12)
    ref_V = R.bias_grid(axes, c, w, p['sigma'], p['periods'])['V'][0]
    ref_F = R.free_energy(ref_V, kT, kdT); ref_F = ref_F - ref_F.min()
    assert F.shape == (144, 3) and np.abs(F[:, 2] - ref_F).max() <= 2e-5 * max(1., np.abs(ref_F).max())      # (printed with 6 digits)
    assert np.abs(F[:, :2] - R.grid_points(axes)).max() <= 1e-5 * np.abs(R.grid_points(axes)).max()
    ref = R.frame_log_weights(c, w, p['sigma'], series[1:, [2, 0]].astype('f8'), 2 * np.arange(1, 12), pace, kT, kdT, axes)
    hst, edges = np.histogram(series[1:, 1].astype('f8'), bins=4, weights=np.exp(ref['log_w']))
    with np.errstate(divide='ignore'):
        want = -kT * np.log(hst / hst.sum())
    want = want - want[np.isfinite(want)].min()
    print('profile along rg_all: tool %s, yardstick %s; n_visible %s' % (prof[:, 1].tolist(), want.tolist(), ref['n_visible'].tolist()))
    assert ref['n_visible'].tolist() == list(range(11)) and prof.shape == (4, 2)
    both = np.isfinite(want)
    assert np.array_equal(np.isfinite(prof[:, 1]), both) and np.abs(prof[both, 1] - want[both]).max() <= 2e-5 * max(1., want[both].max())
    assert np.abs(prof[:, 0] - 0.5 * (edges[1:] + edges[:-1])).max() <= 1e-5 * edges[-1]


CHECKS = dict(bias=bias, grid=grid, reproducible=reproducible, end_to_end=end_to_end, refusals=refusals, cli=cli)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
