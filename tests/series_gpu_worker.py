"""Child process of tests/test_gpu_series.py: one check of the time-series analysis on the device (upside_hip_series_inefficiency,
csrc/kernels_series.hip; timeseries.py; Ensemble.umbrella_mbar(decorrelate=True)) per invocation,

    python tests/series_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is tests/series_reference.py
(float64 numpy, direct sums per (series, origin), pinned by tests/test_series_config.py); the inputs are tests/series_cases.py.
Bound: |g - g_ref| <= 1e-9 max(1, g_ref) -- both sides are fp64 and a sum of up to 4099 products carries about N eps ~ 1e-12, which
leaves three orders of margin.  stop_lag and the chosen origin are compared exactly; that rests on two conditions asserted on the
yardstick alone before the device is asked: no |C(t)| below 1e-6 where a stop is decided, and the best n_eff 1e-3 ahead of the next."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                  # noqa: E402
import series_cases as C                 # noqa: E402
import series_reference as R             # noqa: E402
import mbar_reference as M               # noqa: E402
from mbar_gpu_worker import ladder, NODE                     # noqa: E402

pkg = P.pkg
E = pkg.engine
ts = pkg.timeseries
BOUND = 1e-9


def ratio(got, want, bound=BOUND):
    """largest |got - want| / (bound max(1, want))"""
    got = np.asarray(got, 'f8'); want = np.asarray(want, 'f8')
    return float((np.abs(got - want) / (bound * np.maximum(1., np.abs(want)))).max()) if got.size else 0.


def same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ('g', 'stop_lag', 'mean', 'variance', 'n_eff'))


def margins(ref, with_argmax):
    """the two conditions of the exact comparisons, on the yardstick alone"""
    assert ref['c_margin'].min() >= C.C_MARGIN, ('c_margin', ref['c_margin'].min())
    if with_argmax and ref['n_eff'].shape[1] > 1:
        s = np.sort(ref['n_eff'], axis=1)
        assert ((s[:, -1] - s[:, -2]) >= C.GAP * s[:, -1]).all(), 'n_eff gap'


def compare(got, ref, rows, label, worst, with_argmax=True):
    """got against the rows `rows` of the yardstick; worst: running maxima"""
    rg = ratio(got['g'], ref['g'][rows]); rm = ratio(got['mean'], ref['mean'][rows]); rv = ratio(got['variance'], ref['variance'][rows])
    worst['g'] = max(worst['g'], rg); worst['mean'] = max(worst['mean'], rm); worst['variance'] = max(worst['variance'], rv)
    worst['stop'] = max(worst['stop'], int(got['stop_lag'].max()))
    ok = (rg <= 1. and rm <= 1. and rv <= 1. and np.array_equal(got['stop_lag'], ref['stop_lag'][rows]) and
          (not with_argmax or np.array_equal(np.argmax(got['n_eff'], axis=1), np.argmax(ref['n_eff'][rows], axis=1))) and
          all(np.isfinite(got[k]).all() for k in ('g', 'mean', 'variance', 'n_eff')) and ratio(got['n_eff'], ref['n_eff'][rows]) <= 1.)
    if not ok:
        print('%s: g ratio %.3e, mean ratio %.3e, variance ratio %.3e (bound 1)\n stop_lag %s\n yardstick %s' %
              (label, rg, rm, rv, got['stop_lag'].tolist(), ref['stop_lag'][rows].tolist()))
    return ok


def parity(work):
    lib = pkg.default_library().calc
    assert lib.upk_series_lag_block() == ts.LAG_BLOCK and lib.upk_series_piece() == ts.PIECE
    worst = dict(g=0., mean=0., variance=0., stop=0); n_call = 0; bad = []
    for T in C.PARITY_T:
        a = C.parity_batch(T)
        for n_origin in (1, 8):
            o = C.parity_origins(T, n_origin)
            ref = R.statistical_inefficiency(a, o)
            margins(ref, True)
            batches = [(np.arange(k, k + 1), 'phi %g alone' % C.PHIS[k]) for k in range(4)] + [(np.arange(3), '3 series'), (np.arange(65), '65 series')]
            assert sorted(set(len(b[0]) for b in batches)) == list(C.PARITY_N_SERIES)
            for rows, what in batches:
                got = ts.statistical_inefficiency(a[rows], o)
                n_call += 1
                if not compare(got, ref, rows, 'T = %d, %d origins, %s' % (T, n_origin, what), worst):
                    bad.append((T, n_origin, what))
            print('T = %4d, %d origins %s: stop lags of the 65 series from %d to %d, smallest |C| at a stop %.2e; running worst g ratio %.3e' %
                  (T, n_origin, o.tolist(), ref['stop_lag'][ref['stop_lag'] > 0].min(), ref['stop_lag'].max(), ref['c_margin'].min(), worst['g']))
    a, n = C.unequal_batch()
    o = C.parity_origins(1000, 8)
    ref = R.statistical_inefficiency(a, o, lengths=n)
    margins(ref, False)
    got = ts.statistical_inefficiency(a, o, lengths=n)
    n_call += 1
    if not compare(got, ref, np.arange(5), 'unequal lengths %s' % n.tolist(), worst, False):
        bad.append('unequal')
    print('unequal lengths %s of stride 1000 (NaN behind each): g[:, 0] = %s' % (n.tolist(), np.round(got['g'][:, 0], 6).tolist()))
    # the origin detect_equilibration picks, 64 origins
    for T in (257, 1000, 4099):
        a = C.parity_batch(T, 8)
        ref = R.detect_equilibration(a)
        assert ref['c_margin'].min() >= C.C_MARGIN and ref['gap'].min() >= C.GAP, (T, ref['c_margin'].min(), ref['gap'].min())
        t0, g, n_eff = ts.detect_equilibration(a)
        print('detect_equilibration, T = %d, 8 series: t0 %s (yardstick %s), g ratio %.3e' % (T, t0.tolist(), ref['t0'].tolist(), ratio(g, ref['g'])))
        if not (np.array_equal(t0, ref['t0']) and ratio(g, ref['g']) <= 1. and ratio(n_eff, ref['n_eff']) <= 1.):
            bad.append(('detect', T))
    print('%d calls; largest |gpu - f64| / (1e-9 max(1, |f64|)): g %.3e, mean %.3e, variance %.3e; largest stop lag %d; failed: %s' %
          (n_call, worst['g'], worst['mean'], worst['variance'], worst['stop'], bad))
    assert not bad


def stress(work):
    rng = np.random.RandomState(77)
    o8 = C.parity_origins(1000, 8)
    # a large mean: products formed before centring would miss 1e-7 by three orders
    a = 1e6 + R.ar1(rng, 1000, 0.9, K=3)
    ref = R.statistical_inefficiency(a, o8)
    margins(ref, False)
    got = ts.statistical_inefficiency(a, o8)
    r = ratio(got['g'], ref['g'], 1e-7)
    print('mean 1e6, unit scatter: largest |g - f64| / (1e-7 max(1, g)) = %.3e (bound 1); g[:, 0] = %s; mean ratio (1e-9 |mean|) %.3e' %
          (r, got['g'][:, 0].tolist(), float((np.abs(got['mean'] - ref['mean']) / (1e-9 * np.abs(ref['mean']))).max())))
    assert r <= 1. and np.array_equal(got['stop_lag'], ref['stop_lag']) and ratio(got['variance'], ref['variance'], 1e-7) <= 1.
    assert (np.abs(got['mean'] - ref['mean']) <= 1e-9 * np.abs(ref['mean'])).all()
    # constant series, also one whose sums are not exact and one at 1e6
    a = np.stack([np.full(300, 2.5), np.full(300, 0.1), np.full(300, 1e6 + 0.3)])
    got = ts.statistical_inefficiency(a, [0, 100, 290])
    print('constant series: g %s stop_lag %s variance %s' % (got['g'].tolist(), got['stop_lag'].tolist(), got['variance'].tolist()))
    assert got['g'].tolist() == [[1., 1., 0.]] * 3 and got['stop_lag'].tolist() == [[0, 0, -1]] * 3 and not got['variance'].any()
    assert np.array_equal(got['mean'], a[:, :3])
    # a start-up drift
    x = C.drift_series()
    ref = R.detect_equilibration(x)
    assert ref['c_margin'].min() >= C.C_MARGIN and ref['gap'].min() >= C.GAP and ref['t0'][0] > 0
    t0, g, n_eff = ts.detect_equilibration(x)
    print('drift of five sigma over T / 8 = 256: t0 = %d (yardstick %d), g = %.6f (%.6f), n_eff = %.3f' % (t0, ref['t0'][0], g, ref['g'][0], n_eff))
    assert t0 == ref['t0'][0] and t0 > 0 and abs(g - ref['g'][0]) <= BOUND * max(1., ref['g'][0])
    w = ts.detect_equilibration(C.white_series())
    print('white noise: t0 = %d, g = %r' % (w[0], w[1]))
    assert w[0] == 0 and w[1] == 1.
    # a lag cap below the natural stop; other mintimes
    a = C.parity_batch(1000, 8)
    free = R.statistical_inefficiency(a, o8)
    for cap in (1, 5, 127, 128, 129):
        ref = R.statistical_inefficiency(a, o8, max_lag=cap)
        margins(ref, False)
        got = ts.statistical_inefficiency(a, o8, max_lag=cap)
        capped = free['stop_lag'] > cap + 1
        print('max_lag = %3d: %d of %d tails capped, g ratio %.3e' % (cap, capped.sum(), capped.size, ratio(got['g'], ref['g'])))
        assert (got['stop_lag'][capped] == cap + 1).all() and np.array_equal(got['stop_lag'], ref['stop_lag']) and ratio(got['g'], ref['g']) <= 1.
        assert capped.any() or cap > 5
    for mintime in (1, 10):
        ref = R.statistical_inefficiency(a, o8, mintime=mintime)
        margins(ref, False)
        got = ts.statistical_inefficiency(a, o8, mintime=mintime)
        print('mintime = %2d: stop lags at origin 0 %s, g ratio %.3e' % (mintime, got['stop_lag'][:, 0].tolist(), ratio(got['g'], ref['g'])))
        assert np.array_equal(got['stop_lag'], ref['stop_lag']) and ratio(got['g'], ref['g']) <= 1.
    # short tails: origins whose tails hold 17, 16, 15, 1 and no samples
    got = ts.statistical_inefficiency(a[:2], [983, 984, 985, 999, 1000, 5000])
    ref = R.statistical_inefficiency(a[:2], [983, 984, 985, 999, 1000, 5000])
    print('tails of 17, 16, 15, 1, 0, 0 samples: g %s stop_lag %s' % (got['g'].tolist(), got['stop_lag'].tolist()))
    assert (got['g'][:, 2:] == 0.).all() and (got['stop_lag'][:, 2:] == -1).all() and (got['n_eff'][:, 2:] == 0.).all() and (got['g'][:, :2] >= 1.).all()
    assert ratio(got['g'], ref['g']) <= 1. and all(np.isfinite(got[k]).all() for k in ('g', 'mean', 'variance', 'n_eff'))


def reproducible(work):
    for T, n_origin in ((4099, 8), (1000, 1), (65, 8)):
        a = C.parity_batch(T)
        o = C.parity_origins(T, n_origin)
        one = ts.statistical_inefficiency(a, o); two = ts.statistical_inefficiency(a, o)
        alone = ts.statistical_inefficiency(a[:1], o)
        last = ts.statistical_inefficiency(a[[1, 2, 0]], o)
        s = dict(two_calls=same_bits(one, two),
                 alone=all(alone[k][0].tobytes() == one[k][0].tobytes() for k in alone),
                 last_of_3=all(last[k][2].tobytes() == one[k][0].tobytes() for k in last))
        print('T = %d, %d origins: two calls on 65 series bit-identical, series 0 alone and as the last of 3 as in the 65: %s' % (T, n_origin, s))
        assert all(s.values())


def end_to_end(work):
    fs, spec, centers, pos0 = ladder(work)
    kT = 0.8
    ens = E.Ensemble.from_files(fs)
    ens.set_pos(pos0.astype('f4'))
    ens.init_md(kT, 21)
    bare = dict((k, v) for k, v in spec.items() if k not in pkg.config.CV_RESTRAINT_VALUES)
    rg = {'name': 'rg_all', 'kind': 'rg', 'atoms': np.arange(len(pos0), dtype='i4')}
    ens.define_cvs([rg, bare])
    ens.record_cvs(1, 200)
    ens.run_rounds(200)
    series = ens.read_cvs(reset=False)
    assert series.shape == (200, 8, 2)
    rows = np.column_stack((centers, np.full(8, 2.0), np.full(8, 0.25))).astype('f4')
    # the yardstick on the own-state bias series of every window
    bias = np.stack([M.reduced_energy(series[:, s, 1:2], None, [1. / kT], rows[s:s + 1], np.zeros(1))[:, 0] for s in range(8)])
    ref = R.detect_equilibration(bias)
    print('own-state bias series, 8 windows x 200 rounds: yardstick t0 %s g %s; smallest |C| at a stop %.2e, smallest n_eff gap %.2e' %
          (ref['t0'].tolist(), np.round(ref['g'], 4).tolist(), ref['c_margin'].min(), ref['gap'].min()))
    assert ref['c_margin'].min() >= C.C_MARGIN and ref['gap'].min() >= C.GAP
    want_kept = [R.subsample_indices(200, ref['t0'][s], ref['g'][s]) for s in range(8)]
    got = ens.umbrella_mbar(NODE, kT, tol=0., max_iter=20, uncertainty=True, decorrelate=True)
    print('decorrelate=True: t0 %s, g ratio %.3e (bound 1), kept %s samples, f = %s, sigma(f_k - f_0) = %s' %
          (got['t0'].tolist(), ratio(got['g'], ref['g']), [len(k) for k in got['kept']], np.round(got['f'], 4).tolist(), np.round(got['sigma'][:, 0], 4).tolist()))
    assert np.array_equal(got['t0'], ref['t0']) and ratio(got['g'], ref['g']) <= 1. and ratio(got['n_eff'], ref['n_eff']) <= 1.
    assert len(got['kept']) == 8 and all(np.array_equal(a, b) for a, b in zip(got['kept'], want_kept))
    assert got['n_k'].tolist() == [len(k) for k in got['kept']] and got['n_k'].sum() == len(got['values']) and (got['n_k'] > 0).all()
    values = np.concatenate([series[want_kept[s], s, 1:2] for s in range(8)])
    assert got['values'].tobytes() == np.ascontiguousarray(values, 'f4').tobytes()
    direct = pkg.mbar.mbar(values, None, 1. / kT, rows, got['n_k'], np.zeros(1), 0., 20)
    assert got['f'].tobytes() == direct['f'].tobytes() and np.isfinite(got['f']).all() and np.isfinite(got['sigma']).all()
    sig = pkg.mbar.free_energy_uncertainty(values, None, 1. / kT, rows, got['n_k'], direct['f'], np.zeros(1))
    assert got['sigma'].tobytes() == sig.tobytes()
    # decorrelate=False: as before, the bits of a direct call on the full series
    plain = ens.umbrella_mbar(NODE, kT, tol=0., max_iter=20, uncertainty=True)
    full = series[:, :, 1].reshape(-1, 1)
    direct = pkg.mbar.mbar(full, None, 1. / kT, rows, np.full(8, 200, 'i8'), np.zeros(1), 0., 20)
    print('decorrelate=False: f = %s, sigma(f_k - f_0) = %s' % (np.round(plain['f'], 4).tolist(), np.round(plain['sigma'][:, 0], 4).tolist()))
    assert plain['f'].tobytes() == direct['f'].tobytes() and plain['D'].tobytes() == direct['D'].tobytes() and plain['n_k'].tolist() == [200] * 8
    assert plain['values'].tobytes() == full.tobytes() and not any(k in plain for k in ('t0', 'g', 'n_eff', 'kept'))
    ens.close()


def refusals(work):
    a = C.parity_batch(64, 3)
    ok = ts.statistical_inefficiency(a, [0, 8])
    for label, kw, fragment in C.refusal_cases(a):
        try:
            ts.statistical_inefficiency(**kw)
        except RuntimeError as err:
            print('%-34s refused: %s' % (label, err))
            assert fragment in str(err), (label, str(err))
        else:
            raise AssertionError('%s was accepted' % label)
    # those that only the raw entry point can be told: NULL arrays and n_series x stride at 2^40, refused before an array is read
    lib = pkg.default_library().calc
    n = np.full(3, 64, 'i8'); o = np.zeros(1, 'i8'); g = np.zeros(3); stop = np.zeros(3, 'i8')
    good = [3, 64, n.ctypes.data, a.ctypes.data, 1, o.ctypes.data, 3, 100, g.ctypes.data, stop.ctypes.data, None, None]
    for label, at, value, fragment in (('a NULL', 3, None, 'must be given'), ('length NULL', 2, None, 'must be given'), ('origin NULL', 5, None, 'must be given'),
                                       ('g NULL', 8, None, 'must be given'), ('stop_lag NULL', 9, None, 'must be given'),
                                       ('n_series x stride at 2^40', 1, 1 << 39, '2^40')):
        args = list(good); args[at] = value
        rc = lib.upside_hip_series_inefficiency(*args)
        msg = lib.upside_hip_last_error().decode()
        print('%-34s refused: %s' % (label, msg))
        assert rc == 1 and fragment in msg
    assert lib.upside_hip_series_inefficiency(*good) == 0 and g.tobytes() == ts.statistical_inefficiency(a)['g'][:, 0].tobytes()      # mean and variance may be NULL
    again = ts.statistical_inefficiency(a, [0, 8])
    assert same_bits(ok, again) and np.isfinite(again['g']).all()
    print('a good call after the refusals returns the bits of the one before them')


CHECKS = dict(parity=parity, stress=stress, reproducible=reproducible, end_to_end=end_to_end, refusals=refusals)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
