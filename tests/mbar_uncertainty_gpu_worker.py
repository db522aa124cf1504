"""Child process of tests/test_gpu_mbar_uncertainty.py: one check of the MBAR Gram pass, the uncertainties built on it and the Newton
solver (upside_hip_mbar_gram, csrc/kernels_mbar_gram.hip; mbar.gram, free_energy_uncertainty, expectation, profile,
mbar(solver='newton')) per invocation,

    python tests/mbar_uncertainty_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is
tests/mbar_uncertainty_reference.py (float64 numpy on the whole weight matrix, the covariance by eq. D8 with the N x N
pseudo-inverse); the inputs are tests/mbar_uncertainty_cases.py and the seeded cases of tests/mbar_reference.py.  Bounds:
|dG_kl| <= 1e-9 sqrt(G_kk G_ll) with the yardstick's diagonal and colsum within 1e-9 relative (both sides fp64; a sum of at most 1e4
positive terms carries about 1e-12, the exponent about 1e-10 where reduced energies of 3e5 cancel -- mbar_uncertainty_cases.gram_case);
every variance within 1e-6 relative (a relative perturbation eps of G moves the variances by about 14 eps); equalities between two
calls are bitwise."""
import ctypes as ct
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                          # noqa: E402
import mbar_reference as M                       # noqa: E402
import mbar_uncertainty_reference as U           # noqa: E402
import mbar_uncertainty_cases as C               # noqa: E402

pkg = P.pkg
mb = pkg.mbar
G_BOUND = 1e-9
VAR_BOUND = 1e-6


def arrays(case):
    return dict((k, case[k]) for k in ('values', 'energy', 'beta', 'rows', 'n_k', 'periods'))


def g_ratio(got, want):
    """largest |got - want| / (1e-9 sqrt(want_kk want_ll)); a zero diagonal of the yardstick asks for an exact zero"""
    dg = np.sqrt(np.diag(want))
    scale = G_BOUND * dg[:, None] * dg[None, :]
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0., 0., err / scale)
    return float(r.max())


def c_ratio(got, want):
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.where(err == 0., 0., err / (G_BOUND * np.abs(want))).max())


def yardstick(case, n_extra, seed):
    """(f after 20 iterations from 0, log-columns, G, colsum, D) of the yardstick"""
    u = U.energies(case)
    f = np.zeros(u.shape[1])
    for _ in range(20):
        f, _ = M.iterate(u, case['n_k'], f)
    cols = U.extra_columns(len(u), n_extra, seed) if n_extra else None
    W, D = U.weights(u, case['n_k'], f, cols)
    return f, cols, W.T @ W, W.sum(axis=0), D


def check_gram(got, G, c, D, what):
    assert np.isfinite(got['G']).all() and np.isfinite(got['colsum']).all() and np.isfinite(got['D']).all(), ('not finite', what)
    assert got['G'].tobytes() == got['G'].T.copy().tobytes(), ('G is not bitwise symmetric', what)
    rg, rc = g_ratio(got['G'], G), c_ratio(got['colsum'], c)
    rd = float((np.abs(got['D'] - D) / (G_BOUND * np.maximum(1., np.abs(D)))).max())
    return rg, rc, rd


def gram_shapes(d):
    lib = pkg.default_library().calc
    T = lib.upk_mbar_gram_tile()
    assert T == C.GRAM_TILE == mb.GRAM_TILE
    worst = dict(G=0., colsum=0., D=0.); at = {}; n_case = 0; u_max = 0.
    for N in C.GRAM_N:
        for m in C.gram_columns(T):
            for n_extra in C.GRAM_EXTRA:
                K = m - n_extra
                if K < 1:
                    continue
                seed = 1000 * d + 10 * N + m + n_extra
                case = C.gram_case(N, K, d, seed)
                f, cols, G, c, D = yardstick(case, n_extra, seed)
                u_max = max(u_max, float(np.abs(U.energies(case)).max()))
                got = mb.gram(f=f, log_columns=cols, **arrays(case))
                only = mb.gram(f=f, log_columns=cols, want_gram=False, **arrays(case))
                assert only['G'] is None and only['colsum'].tobytes() == got['colsum'].tobytes(), ('colsum-only differs', N, m, n_extra, d)
                for key, r in zip(('G', 'colsum', 'D'), check_gram(got, G, c, D, (N, m, n_extra, d))):
                    if r >= worst[key]:
                        worst[key] = r; at[key] = (N, m, n_extra)
                n_case += 1
    print('d = %d: %d cases, N in %s, M in %s, n_extra in %s; largest reduced energy %.3e' % (d, n_case, C.GRAM_N, C.gram_columns(T), C.GRAM_EXTRA, u_max))
    print('G: largest |gpu - f64| / (1e-9 sqrt(G_kk G_ll)) = %.3e at (N, M, n_extra) = %s' % (worst['G'], at['G']))
    print('colsum: largest |gpu - f64| / (1e-9 |f64|) = %.3e at %s;  D: largest ratio to 1e-9 max(1, |D|) = %.3e' % (worst['colsum'], at['colsum'], worst['D']))
    assert worst['G'] <= 1. and worst['colsum'] <= 1. and worst['D'] <= 1.
    assert d == 0 or u_max > 1e5, 'no state with reduced energies above 1e5 among the inputs'      # (d = 0, a temperature ladder, has no stiff state)


class States(ct.Structure):
    _fields_ = [('d', ct.c_int), ('n_state', ct.c_int), ('beta', ct.c_void_p), ('rows', ct.c_void_p), ('period', ct.c_double * 8)]


class Samples(ct.Structure):
    _fields_ = [('n', ct.c_longlong), ('values', ct.c_void_p), ('energy', ct.c_void_p)]


def launcher():
    lib = pkg.default_library().calc
    lib.upk_mbar_gram_rows.restype = ct.c_longlong
    lib.upk_mbar_gram_rows.argtypes = [ct.c_int, ct.c_size_t]
    lib.upk_mbar_gram_partial_bytes.restype = ct.c_size_t
    lib.upk_mbar_denominator.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p]
    lib.upk_mbar_gram.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_void_p, ct.c_int, ct.c_void_p, ct.c_void_p, ct.c_void_p,
                                  ct.c_void_p, ct.c_size_t]
    return lib


def one_granule(lib, m):
    """the bytes of the smallest workspace upk_mbar_gram accepts for m columns: the partial sums and one granule of rows"""
    T = lib.upk_mbar_gram_tile()
    nbytes = lib.upk_mbar_gram_partial_bytes(m) + (m + T - 1) // T * T * 8 * C.GRAM_GRANULE
    assert lib.upk_mbar_gram_rows(m, nbytes) == C.GRAM_GRANULE and lib.upk_mbar_gram_rows(m, nbytes - 1) == 0
    return nbytes


def launch_gram(lib, case, f, cols, nbytes):
    """upk_mbar_denominator and upk_mbar_gram on device arrays (torch) with a workspace of nbytes: (return code, dict(G, colsum, D))"""
    import torch
    n_extra, K = len(cols), len(case['n_k'])
    m, N, d = K + n_extra, len(case['values']), case['values'].shape[1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    t = dict(values=dev(case['values']), energy=dev(case['energy']), beta=dev(case['beta']), rows=dev(case['rows']), f=dev(f), cols=dev(cols),
             a=dev(np.where(case['n_k'] > 0, np.log(np.maximum(case['n_k'], 1)) + f, -np.inf)))
    out = dict(D=torch.zeros(N, dtype=torch.float64, device='cuda'), G=torch.full((m, m), np.nan, dtype=torch.float64, device='cuda'),
               c=torch.zeros(m, dtype=torch.float64, device='cuda'), w=torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device='cuda'))
    S = States(d, K, t['beta'].data_ptr(), t['rows'].data_ptr(), (ct.c_double * 8)(*case['periods']))
    X = Samples(N, t['values'].data_ptr(), t['energy'].data_ptr())
    torch.cuda.synchronize()
    assert lib.upk_mbar_denominator(None, ct.byref(S), ct.byref(X), t['a'].data_ptr(), out['D'].data_ptr()) == 0
    rc = lib.upk_mbar_gram(None, ct.byref(S), ct.byref(X), out['D'].data_ptr(), t['f'].data_ptr(), n_extra, t['cols'].data_ptr(),
                           out['G'].data_ptr(), out['c'].data_ptr(), out['w'].data_ptr(), nbytes)
    torch.cuda.synchronize()
    return rc, dict(G=out['G'].cpu().numpy(), colsum=out['c'].cpu().numpy(), D=out['D'].cpu().numpy())


def gram_slabs(work):
    """upk_mbar_gram itself with the smallest workspace: N on both sides of one slab and over several; and a converged f"""
    lib = launcher()
    T = lib.upk_mbar_gram_tile()
    n_extra, d = 3, 2
    m = 2 * T + 1
    nbytes = one_granule(lib, m)
    R = lib.upk_mbar_gram_rows(m, nbytes)
    print('M = %d: a workspace of %d bytes holds R = %d rows, one byte less %d' % (m, nbytes, R, lib.upk_mbar_gram_rows(m, nbytes - 1)))
    worst = 0.
    for N in (R - 1, R, R + 1, 3 * R + 1):
        case = C.gram_case(N, m - n_extra, d, 4000 + N)
        f, cols, G, c, D = yardstick(case, n_extra, N)
        small, _ = launch_gram(lib, case, f, cols, nbytes - 1)
        rc, got = launch_gram(lib, case, f, cols, nbytes)
        rg, rcs, rd = check_gram(got, G, c, D, N)
        print('N = %d (R = %d): return %d (a workspace one byte short: %d); G ratio %.3e, colsum ratio %.3e, D ratio %.3e (bound 1)' % (N, R, rc, small, rg, rcs, rd))
        assert rc == 0 and small == 9405
        worst = max(worst, rg, rcs, rd)
    assert worst <= 1.
    tol = 1e-10
    for name, case in (('harmonic', M.case_harmonic()), ('periodic', M.case_periodic())):
        r = mb.mbar(tol=tol, max_iter=5000, **case)
        c = mb.gram(f=r['f'], want_gram=False, **arrays(case))['colsum']
        print('%s, f converged to %.0e: largest |colsum - 1| = %.3e (bound %.0e)' % (name, tol, np.abs(c - 1.).max(), 10 * tol))
        assert np.abs(c[case['n_k'] > 0] - 1.).max() <= 10 * tol


SWITCH = 1985      # from this M on (512 tiles or more in the upper triangle) a slab is not cut into ranges: the tiles accumulate in G itself


def gram_switch(work):
    """both sides of the switch between the two accumulation paths, through upk_mbar_gram with one granule of rows so that four slabs
    accumulate: M = 1984 (2 ranges, partial matrices of stride Mp, then the reduction) and M = 1985, 2049 (straight into G with the
    stride M, no multiple of 64: the bounds of the last tile row and column, and the read-back of G on the later slabs)"""
    lib = launcher()
    n_extra, d, N = 3, 2, 3 * C.GRAM_GRANULE + 4
    worst = 0.
    for m in (SWITCH - 1, SWITCH, 2049):
        parts = lib.upk_mbar_gram_partial_bytes(m)
        assert (parts > 0) == (m < SWITCH), (m, parts)
        case = C.gram_case(N, m - n_extra, d, 7000 + m)
        f, cols, G, c, D = yardstick(case, n_extra, m)
        nbytes = one_granule(lib, m)
        rc, got = launch_gram(lib, case, f, cols, nbytes)
        rc2, again = launch_gram(lib, case, f, cols, nbytes)
        rg, rcs, rd = check_gram(got, G, c, D, m)
        same = all(got[k].tobytes() == again[k].tobytes() for k in ('G', 'colsum', 'D'))
        print('M = %d, N = %d in slabs of %d rows (%s): return %d; G ratio %.3e, colsum ratio %.3e, D ratio %.3e (bound 1); two calls bit-identical: %s' %
              (m, N, C.GRAM_GRANULE, '%d bytes of partial sums' % parts if parts else 'accumulated in G', rc, rg, rcs, rd, same))
        assert rc == 0 and rc2 == 0 and same
        worst = max(worst, rg, rcs, rd)
    assert worst <= 1.


def reproducible(work):
    T = mb.GRAM_TILE
    for N, m, n_extra, d in ((1000, 2 * T + 1, 3, 2), (1000, 2 * T + 1, 1, 0)):
        case = C.gram_case(N, m - n_extra, d, 5)
        f, cols, _, _, _ = yardstick(case, n_extra, 5)
        a = mb.gram(f=f, log_columns=cols, **arrays(case)); b = mb.gram(f=f, log_columns=cols, **arrays(case))
        same = dict((k, a[k].tobytes() == b[k].tobytes()) for k in ('G', 'colsum', 'D'))
        print('(N, M, d) = (%d, %d, %d): two calls bit-identical: %s' % (N, m, d, same))
        assert all(same.values())


def rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(want).max()) if np.size(want) else 0.


def compare_uncertainties(name, case, f, target, observables, x, edges, kT, period):
    """free_energy_uncertainty, expectation and profile of the product at f against the yardstick: the largest relative error of a variance"""
    u = U.energies(case); n_k = case['n_k']
    W, _ = U.weights(u, n_k, f)
    Pinv = U.inner_pinv(W, n_k)
    want = U.pair_variance(U.theta_d8(W, n_k, Pinv))
    got = mb.free_energy_uncertainty(f=f, **arrays(case)) ** 2
    off = ~np.eye(len(want), dtype=bool)
    worst = float((np.abs(got - want)[off] / want[off]).max())
    print('%s: var(f_i - f_j) in [%.3e, %.3e], largest relative error %.3e' % (name, want[off].min(), want[off].max(), worst))
    lw = U.target_log_weights(case, u, n_k, f, target)
    mean_w, var_w = U.expectation(u, n_k, f, lw, observables, Pinv)
    mean_g, sig_g = mb.expectation(f=f, observables=observables, target=target, **arrays(case))
    r_mean = float((np.abs(mean_g - mean_w) / np.maximum(1., np.abs(mean_w))).max())
    r_var = float((np.abs(sig_g ** 2 - var_w) / var_w).max())
    print('%s: averages %s +- %s; largest error of a mean %.3e (bound 1e-9), relative error of a variance %.3e' % (name, np.round(mean_g, 5), np.round(sig_g, 5), r_mean, r_var))
    xf = x if period == 0 else edges[0] + np.mod(x - edges[0], period)
    F_w, var_F = U.profile(u, n_k, f, lw, xf, edges, kT, Pinv)
    F_g, dF_g = mb.profile(f=f, edges=edges, kT=kT, period=period, target=target, cv=x, **arrays(case))
    full = np.isfinite(F_w)
    assert (np.isfinite(F_g) == full).all() and np.isnan(dF_g[~full]).all() and (F_g[~full] == np.inf).all()
    r_F = float(np.abs(F_g[full] - F_w[full]).max())
    nz = full & (var_F > 0)
    r_dF = float((np.abs(dF_g[nz] ** 2 - var_F[nz]) / var_F[nz]).max())
    print('%s: profile over %d bins (%d empty), dF up to %.4f; largest |F - f64| %.3e (bound 1e-9), relative error of a variance %.3e' %
          (name, len(F_w), int((~full).sum()), np.nanmax(dF_g), r_F, r_dF))
    assert r_mean <= 1e-9 and r_F <= 1e-9 and (dF_g[full & ~nz] == 0.).all()
    return max(worst, r_var, r_dF)


def uncertainty(work):
    case = M.case_harmonic()
    f = U.solve(U.energies(case), case['n_k'])
    x = case['values'][:, 0].astype('f8')
    w1 = compare_uncertainties('harmonic', case, f, (1. / 0.8, None), np.column_stack((x, x * x)), x,
                               np.concatenate((np.linspace(4., 9., 11), [40., 50.])), 0.8, 0.)
    case = M.case_periodic()
    f = U.solve(U.energies(case), case['n_k'])
    v = case['values'].astype('f8')
    w2 = compare_uncertainties('periodic', case, f, (1.25, None), np.column_stack((np.cos(v[:, 0]), v[:, 1])), v[:, 0],
                               np.linspace(-np.pi, np.pi, 9), 0.8, 2 * np.pi)
    print('largest relative error of a variance: %.3e (bound %.0e)' % (max(w1, w2), VAR_BOUND))
    assert max(w1, w2) <= VAR_BOUND


def newton(work):
    tol = 1e-10
    for name, case in (('harmonic', M.case_harmonic()), ('periodic', M.case_periodic()), ('harmonic, windows 2 and 5 empty', U.emptied(M.case_harmonic()))):
        u = U.energies(case); n_k = case['n_k']
        got = mb.mbar(tol=tol, solver='newton', n_sc=3, target=(1.25, None), **case)
        nxt, _ = M.iterate(u, n_k, got['f'])
        moved = float(np.abs(nxt - got['f']).max())
        want = U.solve(u, n_k, tol=1e-13)
        err = float(np.abs(got['f'] - want).max())
        plain = mb.mbar(tol=tol, max_iter=5000, target=(1.25, None), **case)
        print('%s: %d Newton steps and %d iterations (plain iteration: %d), last_delta %.3e (tol %.0e), one yardstick iteration moves f by %.3e '
              '(bound %.0e), |f - yardstick at 1e-13| %.3e (bound 1e-9), |f - plain iteration| %.3e' %
              (name, got['n_newton'], got['n_iter'], plain['n_iter'], got['last_delta'], tol, moved, 10 * tol, err, np.abs(got['f'] - plain['f']).max()))
        assert got['last_delta'] < tol and moved < 10 * tol and got['n_newton'] <= 10 and got['n_iter'] <= 20 and err <= 1e-9
        assert np.isfinite(got['D']).all() and abs(float(np.exp(got['log_w']).sum()) - 1.) <= 1e-12
        named = mb.mbar(tol=tol, max_iter=5000, target=(1.25, None), solver='self-consistent', **case)
        assert all(named[k].tobytes() == plain[k].tobytes() for k in ('f', 'D', 'log_w')) and named['n_iter'] == plain['n_iter'] and 'n_newton' not in plain
    print("solver='self-consistent' returns the bits of a call without the argument")


def end_to_end(work):
    import mbar_gpu_worker as W0
    fs, spec, centers, pos0 = W0.ladder(work)
    E = pkg.engine
    ens = E.Ensemble.from_files(fs)
    ens.set_pos(pos0.astype('f4'))
    ens.init_md(0.8, 21)
    bare = dict((k, v) for k, v in spec.items() if k not in pkg.config.CV_RESTRAINT_VALUES)
    rg = {'name': 'rg_all', 'kind': 'rg', 'atoms': np.arange(len(pos0), dtype='i4')}
    ens.define_cvs([rg, bare])
    ens.record_cvs(1, 200)
    ens.run_rounds(200)
    tol = 1e-10
    got = ens.umbrella_mbar(W0.NODE, 0.8, tol=tol, solver='newton', uncertainty=True)
    series = ens.read_cvs()
    ens.close()
    assert series.shape == (200, 8, 2) and np.isfinite(series).all()
    values = series[:, :, 1].reshape(-1, 1)
    rows = np.column_stack((centers, np.full(8, 2.0), np.full(8, 0.25))).astype('f4')
    case = dict(values=values, energy=None, beta=np.full(8, 1. / 0.8), rows=rows, n_k=np.full(8, 200, 'i8'), periods=np.zeros(1))
    u = U.energies(case)
    f = U.solve(u, case['n_k'], tol=1e-13)
    W, _ = U.weights(u, case['n_k'], f)
    want = U.pair_variance(U.theta_d8(W, case['n_k']))
    off = ~np.eye(8, dtype=bool)
    err_f = float(np.abs(got['f'] - f).max())
    err_v = float((np.abs(got['sigma'] ** 2 - want)[off] / want[off]).max())
    print('trpcage20, 8 windows on the end-to-end distance, T = 0.8, 200 rounds: %d Newton steps, %d iterations; f = %s' % (got['n_newton'], got['n_iter'], np.round(got['f'], 4).tolist()))
    print('sigma(f_k - f_0) = %s' % np.round(got['sigma'][:, 0], 4).tolist())
    print('|f - yardstick| %.3e (bound 1e-9), largest relative error of a variance %.3e (bound %.0e)' % (err_f, err_v, VAR_BOUND))
    assert got['last_delta'] < tol and err_f <= 1e-9 and err_v <= VAR_BOUND
    # the same ladder from files, through tools/umbrella_mbar.py --solver newton --uncertainty: /output/cv in the layout upside_hip writes
    import contextlib
    import importlib.util
    import io
    for s, path in enumerate(fs):
        pkg.config.add_collective_variables(path, [rg, bare])
        with pkg.h5lite.open_file(path, 'r+') as f:
            out = f.create_group('output') if 'output' not in f.keys() else f.group('output')
            out.write('cv', np.ascontiguousarray(series[:, s:s + 1, :]))
    spec_ = importlib.util.spec_from_file_location('umbrella_mbar_tool', os.path.join(P.ROOT, 'tools', 'umbrella_mbar.py'))
    tool = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(tool)
    argv, text = sys.argv, io.StringIO()
    sys.argv = ['umbrella_mbar.py', '--temperature', '0.8', '--node', W0.NODE, '--tol', '1e-10', '--bins', '8', '--solver', 'newton', '--uncertainty'] + list(fs)
    try:
        with contextlib.redirect_stdout(text):
            tool.main()
    finally:
        sys.argv = argv
    lines = text.getvalue().splitlines()
    print('\n'.join(lines[:3] + ['...'] + lines[-3:]))
    table = [l.split() for l in lines if not l.startswith('#')]
    windows, bins = np.array(table[:8], 'f8'), np.array(table[8:], 'f8')
    assert windows.shape == (8, 5) and bins.shape == (8, 3) and 'Newton steps' in lines[0]
    assert np.abs(windows[:, 3] - got['f']).max() < 1e-7 and np.abs(windows[:, 4] - got['sigma'][:, 0]).max() < 1e-5
    full = np.isfinite(bins[:, 1])
    assert full.any() and np.isfinite(bins[full, 2]).all() and bins[np.argmin(bins[:, 1]), 2] == 0. and (bins[full, 2] >= 0.).all()


def expect_refusal(what, fragment, call):
    try:
        call()
    except (RuntimeError, ValueError) as err:
        print('%-38s refused: %s' % (what, err))
        assert fragment in str(err), (what, str(err))
    else:
        raise AssertionError('%s was accepted' % what)


def refusals(work):
    good, cases = C.gram_refusal_cases()
    ok = mb.gram(**good)
    for label, change, fragment in cases:
        kw = dict(good); kw.update(change)
        expect_refusal(label, fragment, lambda: mb.gram(**kw))
    # what only the raw entry point can be told
    lib = pkg.default_library().calc
    v, n_k, f = np.ascontiguousarray(good['values'], 'f4'), np.ascontiguousarray(good['n_k'], 'i8'), np.ascontiguousarray(good['f'])
    beta, rows, per = np.ones(3), np.ascontiguousarray(good['rows'], 'f4'), np.zeros(1)
    out = np.zeros(64)
    p = lambda a: a.ctypes.data
    for label, n_state, n_extra, colsum, fragment in (('n_extra below 0', 3, -1, p(out), 'n_extra = -1'), ('colsum missing', 3, 0, None, 'colsum must be given'),
                                                     ('n_state + n_extra above 8192', 3, 8190, p(out), 'at most 8192')):
        rc = lib.upside_hip_mbar_gram(30, n_state, 1, p(v), None, p(beta), p(rows), p(n_k), p(per), p(f), n_extra, p(out), None, colsum, None)
        msg = lib.upside_hip_last_error().decode()
        print('%-38s refused: %s' % (label, msg))
        assert rc == 1 and fragment in msg
    again = mb.gram(**good)
    assert all(again[k].tobytes() == ok[k].tobytes() for k in ('G', 'colsum', 'D')) and np.isfinite(again['G']).all()
    print('a good call after the refusals returns the bits of the one before them')


CHECKS = dict(gram_d0=lambda w: gram_shapes(0), gram_d1=lambda w: gram_shapes(1), gram_d2=lambda w: gram_shapes(2), gram_d8=lambda w: gram_shapes(8),
              gram_slabs=gram_slabs, gram_switch=gram_switch, reproducible=reproducible, uncertainty=uncertainty, newton=newton, end_to_end=end_to_end, refusals=refusals)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
