"""Child process of tests/test_gpu_mbar.py: one check of MBAR on the device (upside_hip_mbar, csrc/kernels_mbar.hip) per invocation,

    python tests/mbar_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is tests/mbar_reference.py
(float64 numpy, pinned by tests/test_mbar_config.py); the inputs are tests/mbar_cases.py.  Bound: f and D within
1e-9 x max(1, |value|) of the yardstick after the same number of iterations -- both sides are fp64, a sum of N <= 1e4 terms carries
about N eps ~ 1e-12 and the iteration contracts, which leaves three orders of margin; equalities between two calls are bitwise."""
import ctypes as ct
import os
import shutil
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                  # noqa: E402
import mbar_cases as C                   # noqa: E402
import mbar_reference as M               # noqa: E402

pkg = P.pkg
cfg = pkg.config
E = pkg.engine
mbar = pkg.mbar.mbar
BOUND = 1e-9
NAME = 'trpcage20_7A'
NODE = 'cv_restraint'


def reference(case, tol, max_iter, **kw):
    c = dict(case)
    if c['values'] is None:
        c['values'] = np.zeros((len(c['energy']), 0), 'f4')
    return M.mbar(tol=tol, max_iter=max_iter, **dict(c, **kw))


def ratio(got, want):
    """largest |got - want| / (BOUND max(1, |want|))"""
    got = np.asarray(got, 'f8'); want = np.asarray(want, 'f8')
    return float((np.abs(got - want) / (BOUND * np.maximum(1., np.abs(want)))).max())


def fixed(work):
    lib = pkg.default_library().calc
    assert lib.upk_mbar_state_tile() == C.STATE_TILE and lib.upk_mbar_fe_tile() == C.FE_TILE
    worst = dict(f=0., D=0.); worst_abs = dict(f=0., D=0.); at = {}; n_case = 0; u_max = 0.
    for d in C.FIXED_D:
        for N in C.FIXED_N:
            for K in C.FIXED_K:
                case = C.stressed_case(N, K, d, 1000 * d + N + K)
                got = mbar(tol=0., max_iter=20, **case)
                want = reference(case, 0., 20)
                assert got['n_iter'] == 20 and want['n_iter'] == 20
                assert np.isfinite(got['f']).all() and np.isfinite(got['D']).all(), ('not finite', N, K, d)
                u_max = max(u_max, float(np.abs(want['f']).max()))
                for key in ('f', 'D'):
                    r = ratio(got[key], want[key])
                    worst_abs[key] = max(worst_abs[key], float(np.abs(got[key] - want[key]).max()))
                    if r >= worst[key]:
                        worst[key] = r; at[key] = (N, K, d)
                n_case += 1
    print('%d cases, N in %s, K in %s, d in %s, 20 iterations from f = 0; largest |f| of the yardstick %.3e' % (n_case, C.FIXED_N, C.FIXED_K, C.FIXED_D, u_max))
    for key in ('f', 'D'):
        print('%s: largest |gpu - f64| / (1e-9 max(1, |f64|)) = %.3e at (N, K, d) = %s; largest |gpu - f64| = %.3e' % (key, worst[key], at[key], worst_abs[key]))
    assert worst['f'] <= 1. and worst['D'] <= 1.


def convergence(work):
    tol = 1e-10
    for name, case in (('harmonic', M.case_harmonic()), ('periodic', M.case_periodic())):
        got = mbar(tol=tol, max_iter=5000, **case)
        u = M.reduced_energy(case['values'], case['energy'], case['beta'], case['rows'], case['periods'])
        nxt, _ = M.iterate(u, case['n_k'], got['f'])
        moved = float(np.abs(nxt - got['f']).max())
        want = reference(case, tol, 5000)
        print('%s: %d iterations (yardstick %d), last_delta %.3e (tol %.0e), one yardstick iteration moves f by %.3e (bound %.0e), |f - yardstick| %.3e' %
              (name, got['n_iter'], want['n_iter'], got['last_delta'], tol, moved, 10 * tol, np.abs(got['f'] - want['f']).max()))
        assert got['last_delta'] < tol and got['n_iter'] < 5000
        assert moved < 10 * tol


def temperature(work):
    case = C.temperature_case()
    beta_t = 1. / 0.80
    got = mbar(tol=0., max_iter=20, target=(beta_t, None), **case)
    want = reference(case, 0., 20, target=(beta_t, None))
    rf, rD = ratio(got['f'], want['f']), ratio(got['D'], want['D'])
    dw = float(np.abs(got['log_w'] - want['log_w']).max())
    norm = abs(float(np.exp(got['log_w']).sum()) - 1.)
    print('six temperatures, %d samples: f ratio %.3e, D ratio %.3e (bound 1); log-weights at T = 0.80: largest |gpu - f64| %.3e (bound 1e-9), '
          '|sum w - 1| %.3e (bound 1e-12), f_target %.12g (f64 %.12g)' % (len(case['energy']), rf, rD, dw, norm, got['f_target'], want['f_target']))
    assert rf <= 1. and rD <= 1. and dw <= 1e-9 and norm <= 1e-12
    assert abs(got['f_target'] - want['f_target']) <= BOUND * max(1., abs(want['f_target']))
    # a target with a bias of its own (d = 2)
    case = C.stressed_case(257, 5, 2, 77)
    row = case['rows'][1].copy(); row[0] = -3.0
    got = mbar(tol=0., max_iter=20, target=(1.3, row), **case)
    want = reference(case, 0., 20, target=(1.3, row))
    dw = float(np.abs(got['log_w'] - want['log_w']) .max() / max(1., np.abs(want['log_w']).max()))
    norm = abs(float(np.exp(got['log_w']).sum()) - 1.)
    print('biased target, d = 2: log-weights |gpu - f64| / max(1, |f64|) %.3e (bound 1e-9), |sum w - 1| %.3e' % (dw, norm))
    assert dw <= 1e-9 and norm <= 1e-12


def reproducible(work):
    for N, K, d in ((1000, C.STATE_TILE + 1, 2), (257, 5, 8), (1000, 6, 0)):
        case = C.stressed_case(N, K, d, 5)
        tgt = (1.1, None if d != 2 else case['rows'][0])
        a = mbar(tol=0., max_iter=10, target=tgt, **case); b = mbar(tol=0., max_iter=10, target=tgt, **case)
        same = dict((k, a[k].tobytes() == b[k].tobytes()) for k in ('f', 'D', 'log_w'))
        print('(N, K, d) = (%d, %d, %d): two calls bit-identical: %s' % (N, K, d, same))
        assert all(same.values()) and a['f_target'] == b['f_target'] and a['last_delta'] == b['last_delta']


def ladder(work, n=8):
    pos0 = P.golden(NAME)['pos'].astype('f8').reshape(-1, 3)
    n_atom = len(pos0)
    pair = (1, n_atom - 2)      # the first and the last CA
    r0 = float(np.linalg.norm(pos0[pair[0]] - pos0[pair[1]]))
    spec = {'name': 'end_to_end', 'kind': 'distance', 'pair': pair, 'center': r0, 'spring_const': 2.0, 'flat_width': 0.25}
    base = os.path.join(work, 'base.up')
    shutil.copyfile(P.fixture(NAME), base)
    cfg.add_cv_restraint(base, [spec])
    centers = r0 + np.linspace(-2.0, 2.0, n)
    fs = cfg.write_umbrella_windows(base, [os.path.join(work, 'w%d.up' % i) for i in range(n)], NODE, centers)
    return fs, spec, centers, pos0


def end_to_end(work):
    fs, spec, centers, pos0 = ladder(work)
    ens = E.Ensemble.from_files(fs)
    ens.set_pos(pos0.astype('f4'))
    ens.init_md(0.8, 21)
    bare = dict((k, v) for k, v in spec.items() if k not in cfg.CV_RESTRAINT_VALUES)
    rg = {'name': 'rg_all', 'kind': 'rg', 'atoms': np.arange(len(pos0), dtype='i4')}
    ens.define_cvs([rg, bare])      # the node's CV is the second recorded column: found by name
    ens.record_cvs(1, 200)
    ens.run_rounds(200)
    got = ens.umbrella_mbar(NODE, 0.8, tol=0., max_iter=20, target='unbiased')
    series = ens.read_cvs()
    assert series.shape == (200, 8, 2)
    want_rows = np.column_stack((centers, np.full(8, 2.0), np.full(8, 0.25))).astype('f4')
    assert got['rows'].tobytes() == want_rows.tobytes(), 'the rows are not the configuration\'s'
    values = series[:, :, 1].reshape(-1, 1)
    assert got['values'].tobytes() == values.tobytes() and got['names'] == ['end_to_end'] and got['periods'].tolist() == [0.]
    want = M.mbar(values, None, np.full(8, 1. / 0.8), want_rows, np.full(8, 200, 'i8'), np.zeros(1), 0., 20, target=(1. / 0.8, None))
    rf, rD = ratio(got['f'], want['f']), ratio(got['D'], want['D'])
    dw = float(np.abs(got['log_w'] - want['log_w']).max())
    print('trpcage20, 8 windows on the end-to-end distance (centres %s), T = 0.8, 200 rounds: f = %s' % (np.round(centers, 3).tolist(), np.round(got['f'], 4).tolist()))
    print('f ratio %.3e, D ratio %.3e (bound 1), log-weights |gpu - f64| %.3e' % (rf, rD, dw))
    assert np.isfinite(series).all() and rf <= 1. and rD <= 1. and dw <= 1e-9
    edges = np.linspace(values.min(), values.max() + 1e-3, 9)
    prof = cfg.mbar_profile(values[:, 0], got['log_w'], edges, 0.8)
    print('unbiased profile over 8 bins (kT = 0.8): %s' % np.round(prof - prof[np.isfinite(prof)].min(), 3).tolist())
    ens.close()


def expect_refusal(what, fragment, call):
    try:
        call()
    except (RuntimeError, ValueError) as err:
        print('%-34s refused: %s' % (what, err))
        assert fragment in str(err), (what, str(err))
    else:
        raise AssertionError('%s was accepted' % what)


def refusals(work):
    good, cases = C.refusal_cases()
    ok = mbar(tol=0., max_iter=3, **good)
    for label, change, fragment in cases:
        kw = dict(good, tol=0., max_iter=3); kw.update(change)
        expect_refusal(label, fragment, lambda: mbar(**kw))
    expect_refusal('no state', 'at least one state', lambda: mbar(np.zeros((4, 1), 'f4'), None, np.zeros(0), np.zeros((0, 3), 'f4'), np.zeros(0, 'i8')))
    expect_refusal('no sample', 'at least one sample', lambda: mbar(np.zeros((0, 1), 'f4'), None, 1., np.zeros((2, 3), 'f4'), np.zeros(2, 'i8')))
    # N x K at 2^62: only the raw entry point can be told of so many samples; it refuses before it reads an array
    lib = pkg.default_library().calc
    one = np.zeros(8, 'f8'); cnt = np.ones(4, 'i8')
    rc = lib.upside_hip_mbar(ct.c_longlong(1 << 60), 4, 0, None, one.ctypes.data, one.ctypes.data, None, cnt.ctypes.data, None, 0., 1, None, 0, 0., None,
                             one.ctypes.data, None, None, None, None, None)
    msg = lib.upside_hip_last_error().decode()
    print('%-34s refused: %s' % ('N x K = 2^62', msg))
    assert rc == 1 and '2^62' in msg
    # a CV of the node that is not recorded
    fs, spec, centers, pos0 = ladder(work, 2)
    ens = E.Ensemble.from_files(fs)
    ens.set_pos(pos0.astype('f4'))
    ens.define_cvs([{'name': 'rg_all', 'kind': 'rg', 'atoms': np.arange(len(pos0), dtype='i4')}])
    expect_refusal('a node CV that is not recorded', "'end_to_end'", lambda: ens.umbrella_mbar(NODE, 0.8))
    ens.close()
    again = mbar(tol=0., max_iter=3, **good)
    assert again['f'].tobytes() == ok['f'].tobytes() and np.isfinite(again['f']).all()
    print('a good call after the refusals returns the bits of the one before them')


CHECKS = dict(fixed=fixed, convergence=convergence, temperature=temperature, end_to_end=end_to_end, reproducible=reproducible, refusals=refusals)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
