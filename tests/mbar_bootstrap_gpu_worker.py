"""Child process of tests/test_gpu_mbar_bootstrap.py: one check of the MBAR bootstrap on the device (upside_hip_mbar_bootstrap,
csrc/kernels_mbar_boot.hip) per invocation,

    python tests/mbar_bootstrap_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is
tests/mbar_bootstrap_reference.py (float64 numpy, pinned by tests/test_mbar_bootstrap_config.py); the inputs are
tests/mbar_bootstrap_cases.py and tests/mbar_cases.py.  Bound: f_boot and columns within 1e-9 x max(1, |value|) of the yardstick after
the same number of iterations (the bound and the reasoning of tests/mbar_gpu_worker.py: both sides fp64, sums of N <= 1e5 terms);
"the same bits" is bitwise equality."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                  # noqa: E402
import mbar_cases as MC                  # noqa: E402
import mbar_reference as M               # noqa: E402
import mbar_bootstrap_reference as R     # noqa: E402
import mbar_bootstrap_cases as C         # noqa: E402

pkg = P.pkg
E = pkg.engine
mbar = pkg.mbar.mbar
bootstrap = pkg.mbar.bootstrap
BOUND = C.BOUND


def energies(case):
    v = case['values'] if case['values'] is not None else np.zeros((len(case['energy']), 0), 'f4')
    return M.reduced_energy(v, case['energy'], case['beta'], case['rows'], case['periods'])


def ratio(got, want):
    """largest |got - want| / (BOUND max(1, |want|)); entries that are +inf on both sides count as equal"""
    got = np.asarray(got, 'f8'); want = np.asarray(want, 'f8')
    same_inf = np.isinf(got) & np.isinf(want) & (np.sign(got) == np.sign(want))
    if not same_inf.all() and not np.isfinite(got[~same_inf]).all():
        return np.inf
    with np.errstate(invalid='ignore'):
        r = np.abs(got - want) / (BOUND * np.maximum(1., np.abs(want)))
    r[same_inf] = 0.
    return float(r.max())


def fixed(work, d):
    worst = 0.; worst_plain = 0.; worst_abs = 0.; at = None; n_case = 0
    for N in MC.FIXED_N:
        for K in MC.FIXED_K:
            case = MC.stressed_case(N, K, d, 1000 * d + N + K)
            counts = C.fixed_counts(case['n_k'], N + K)
            got = bootstrap(f=None, counts=counts, tol=0., max_iter=20, **case)
            want = R.solve(energies(case), case['n_k'], counts, 0., 20)
            assert (got['n_iter'] == 20).all() and (want['n_iter'] == 20).all() and not got['converged'].any()
            assert np.isfinite(got['f_boot']).all(), ('not finite', N, K, d)
            r = ratio(got['f_boot'], want['f_boot'])
            worst_abs = max(worst_abs, float(np.abs(got['f_boot'] - want['f_boot']).max()))
            if r >= worst:
                worst = r; at = (N, K, d)
            rd = float(np.abs(got['last_delta'] - want['last_delta']).max())
            assert rd <= 2 * BOUND * max(1., float(np.abs(want['f_boot']).max())), ('last_delta', N, K, d, rd)
            plain = mbar(tol=0., max_iter=20, want_denominators=False, **case)['f']
            worst_plain = max(worst_plain, ratio(got['f_boot'][0], plain))
            # ln 1 = 0 is added to every term and the walks are one body: the all-ones replicate is mbar.mbar bit for bit
            assert got['f_boot'][0].tobytes() == plain.tobytes(), ('the all-ones replicate differs from mbar.mbar in its bits', N, K, d)
            n_case += 1
    print('d = %d: %d cases, N in %s, K in %s, 5 replicates (all ones, three seeded draws, one degenerate), 20 iterations from f = 0' % (d, n_case, MC.FIXED_N, MC.FIXED_K))
    print('f_boot: largest |gpu - f64| / (1e-9 max(1, |f64|)) = %.3e at (N, K, d) = %s; largest |gpu - f64| = %.3e' % (worst, at, worst_abs))
    print('the all-ones replicate against mbar.mbar on the same input: largest ratio %.3e' % worst_plain)
    assert worst <= 1. and worst_plain <= 1.


def duplication(work):
    """independent of the yardstick: counts c against the device's own mbar.mbar on the samples repeated c times"""
    worst = 0.
    for N, K, d in ((257, 5, 1), (1000, 129, 2), (256, 4, 0), (255, 3, 8)):
        case = MC.stressed_case(N, K, d, 40 + d)
        counts = C.fixed_counts(case['n_k'], 7 * N + K)
        got = bootstrap(f=None, counts=counts, tol=0., max_iter=20, **case)
        for b in (1, 2, 4):
            want = mbar(tol=0., max_iter=20, want_denominators=False, **C.repeated(case, counts[b]))
            r = ratio(got['f_boot'][b], want['f'])
            print('(N, K, d) = (%d, %d, %d), replicate %d (largest count %d): |bootstrap - mbar on repeated samples| / bound = %.3e' % (N, K, d, b, counts[b].max(), r))
            worst = max(worst, r)
    assert worst <= 1.


def convergence(work):
    tol = C.TOL
    for name, case in (('harmonic', M.case_harmonic()), ('periodic', M.case_periodic())):
        u = energies(case); n_k = case['n_k']
        f = C.converged_start(case)
        counts = pkg.mbar.bootstrap_counts(n_k, C.N_BOOT, seed=C.BOOT_SEED)
        got = bootstrap(f=f, counts=counts, tol=tol, max_iter=5000, **case)
        moved = max(float(np.abs(R.iterate(u, n_k, got['f_boot'][b], counts[b])[0] - got['f_boot'][b]).max()) for b in range(C.N_BOOT))
        asym = pkg.mbar.free_energy_uncertainty(case['values'], case['energy'], case['beta'], case['rows'], n_k, f, case['periods'])
        boot = pkg.mbar.bootstrap_sigma(got)
        off = ~np.eye(len(n_k), dtype=bool)
        q = boot[off] / asym[off]
        print('%s: %d replicates, iterations %d .. %d, largest last_delta %.3e (tol %.0e), one yardstick iteration moves a replicate by at most %.3e '
              '(bound %.0e), bootstrap / asymptotic sigma %.3f .. %.3f (fence %s)' %
              (name, C.N_BOOT, got['n_iter'].min(), got['n_iter'].max(), got['last_delta'].max(), tol, moved, 10 * tol, q.min(), q.max(), C.SIGMA_RATIO))
        assert (got['last_delta'] < tol).all() and got['converged'].all() and got['n_iter'].max() < 5000
        assert moved < 10 * tol
        assert len(set(got['n_iter'].tolist())) > 1, 'every replicate took the same number of iterations: none left the grid early'
        assert C.SIGMA_RATIO[0] <= q.min() and q.max() <= C.SIGMA_RATIO[1]


def independence(work):
    tol = C.TOL
    case = M.case_periodic()
    n_k = case['n_k']; N = int(n_k.sum())
    f = C.converged_start(case)
    counts = pkg.mbar.bootstrap_counts(n_k, C.N_BOOT, seed=C.BOOT_SEED)
    cols, _ = C.profile_columns(case, np.linspace(-np.pi, np.pi, 7))
    kw = dict(case, f=f, tol=tol, max_iter=5000, log_numerators=cols)
    keys = ('f_boot', 'columns', 'n_iter', 'last_delta')
    full = bootstrap(counts=counts, **kw)
    again = bootstrap(counts=counts, **kw)
    same = all(full[k].tobytes() == again[k].tobytes() for k in keys)
    print('two calls on one input, 100 replicates: bit-identical: %s' % same)
    assert same
    small = bootstrap(counts=counts, workspace_bytes=8 * N, **kw)      # the smallest workspace: one replicate at a time
    assert pkg.mbar.boot_chunk(N, 8 * N) == 1
    same = all(full[k].tobytes() == small[k].tobytes() for k in keys)
    print('the batch of 100 solved one replicate at a time (workspace of %d bytes): bit-identical: %s' % (8 * N, same))
    assert same
    for b in (0, 37, 99):
        alone = bootstrap(counts=counts[b:b + 1], **kw)
        same = all(full[k][b:b + 1].tobytes() == alone[k].tobytes() for k in keys)
        print('replicate %d alone (%d iterations): the bits it has in the batch: %s' % (b, alone['n_iter'][0], same))
        assert same
    work_bytes = 8 * N * 7 + 5      # a chunk of 7
    chunk = pkg.mbar.boot_chunk(N, work_bytes)
    assert chunk == 7
    for B in (1, 2, chunk - 1, chunk, chunk + 1):
        part = bootstrap(counts=counts[40:40 + B], workspace_bytes=work_bytes, **kw)
        same = all(full[k][40:40 + B].tobytes() == part[k].tobytes() for k in keys)
        print('replicates 40 .. %d in chunks of %d: the bits they have in the batch: %s' % (40 + B - 1, chunk, same))
        assert same
    # in another order, next to other replicates
    perm = np.random.RandomState(1).permutation(C.N_BOOT)[:23]
    mixed = bootstrap(counts=counts[perm], workspace_bytes=work_bytes, **kw)
    same = all(full[k][perm].tobytes() == mixed[k].tobytes() for k in keys)
    print('23 replicates in another order, chunks of %d: bit-identical: %s' % (chunk, same))
    assert same


def columns(work):
    case = M.case_harmonic()
    u = energies(case); n_k = case['n_k']
    f = M.mbar(tol=0., max_iter=30, **case)['f']
    edges = np.linspace(2.0, 11.0, 13)
    cols, b = C.profile_columns(case, edges)
    cols = np.concatenate((cols, np.full((1, len(u)), -np.inf)))      # a column that is -inf everywhere
    counts = pkg.mbar.bootstrap_counts(n_k, 6, seed=2)
    # replicate 3 holds no sample of bin 5: its counts there move to another sample of the same state outside the bin
    start = np.concatenate(([0], np.cumsum(n_k)))
    for k in range(len(n_k)):
        seg = np.arange(start[k], start[k + 1])
        inside = seg[b[seg] == 5]; outside = seg[b[seg] != 5]
        counts[3, outside[0]] += counts[3, inside].sum(); counts[3, inside] = 0
    assert (b == 5).sum() > 0 and counts[3, b == 5].sum() == 0 and (counts[[0, 1, 2, 4, 5]][:, b == 5].sum(axis=1) > 0).all()
    got = bootstrap(f=f, counts=counts, tol=0., max_iter=12, log_numerators=cols, **case)
    want = R.solve(u, n_k, counts, 0., 12, f0=f, log_numerator=cols)
    rf, rc = ratio(got['f_boot'], want['f_boot']), ratio(got['columns'], want['columns'])
    print('harmonic case, 12 profile bins + one empty column, 6 replicates, 12 iterations: f_boot ratio %.3e, columns ratio %.3e (bound 1)' % (rf, rc))
    print('bins without samples in the full sample: %s; +inf entries per replicate: %s' % (np.flatnonzero([(b == j).sum() == 0 for j in range(12)]).tolist(),
                                                                                         np.isinf(got['columns']).sum(axis=1).tolist()))
    assert rf <= 1. and rc <= 1.
    assert (got['columns'][:, -1] == np.inf).all()
    assert got['columns'][3, 5] == np.inf and np.isfinite(got['columns'][[0, 1, 2, 4, 5], 5]).all()
    assert np.array_equal(np.isinf(got['columns']), np.isinf(want['columns'])) and not np.isnan(got['columns']).any()
    # profile_bootstrap: F of the full sample, dF_boot from the replicates' columns
    f = mbar(tol=C.TOL, max_iter=5000, want_denominators=False, **case)['f']
    F, dF = pkg.mbar.profile_bootstrap(case['values'], case['energy'], case['beta'], case['rows'], n_k, f, edges, 0.8, target=(1.25, None),
                                       periods=case['periods'], n_bootstrap=20, seed=3, tol=1e-9)
    F0, _ = pkg.mbar.profile(case['values'], case['energy'], case['beta'], case['rows'], n_k, f, edges, 0.8, target=(1.25, None), periods=case['periods'])
    full = np.isfinite(F)
    print('profile_bootstrap: F = %s, dF_boot = %s' % (np.round(F - F[full].min(), 3).tolist(), np.round(dF, 3).tolist()))
    assert F.tobytes() == F0.tobytes()
    assert np.isnan(dF[~full]).all() and np.isfinite(dF[full]).all() and dF[np.argmin(np.where(full, F, np.inf))] == 0. and (dF[full] >= 0).all()
    ref = int(np.argmin(np.where(full, F, np.inf)))
    f1 = mbar(tol=0., max_iter=1, f0=f, want_denominators=False, **case)['f']
    cnt = pkg.mbar.bootstrap_counts(n_k, 20, seed=3)
    w = R.solve(u, n_k, cnt, 1e-9, 10000, f0=f1, log_numerator=cols[:-1])
    assert (w['last_delta'] < 1e-9).all()
    want_dF = np.full(12, np.nan)
    for j in np.flatnonzero(full):
        both = np.isfinite(w['columns'][:, j]) & np.isfinite(w['columns'][:, ref])      # (a replicate without a sample in the bin is left out)
        want_dF[j] = (0.8 * (w['columns'][both, j] - w['columns'][both, ref])).std(ddof=1)
    err = float(np.nanmax(np.abs(dF - want_dF)))
    print('dF_boot against the yardstick on the same counts: largest difference %.3e (bound 1e-8: either side may stop one iteration from '
          'the other, which moves a column by at most tol = 1e-9)' % err)
    assert err <= 1e-8 and np.array_equal(np.isnan(dF), np.isnan(want_dF))


def count_range(work):
    case, counts = C.count_range_case()
    got = bootstrap(f=None, counts=counts, tol=0., max_iter=20, **case)
    want = R.solve(energies(case), case['n_k'], counts, 0., 20)
    r = ratio(got['f_boot'], want['f_boot'])
    print('n_k = %s, a replicate with counts 65535 and 465 on two samples: f_boot = %s, ratio %.3e (bound 1)' % (case['n_k'].tolist(), got['f_boot'].tolist(), r))
    assert r <= 1. and counts.max() == 65535


def end_to_end(work):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mbar_gpu_worker as W
    fs, spec, centers, pos0 = W.ladder(work)
    ens = E.Ensemble.from_files(fs)
    ens.set_pos(pos0.astype('f4'))
    ens.init_md(0.8, 21)
    bare = dict((k, v) for k, v in spec.items() if k not in pkg.config.CV_RESTRAINT_VALUES)
    ens.define_cvs([bare])
    ens.record_cvs(1, 200)
    ens.run_rounds(200)
    before = ens.umbrella_mbar(W.NODE, 0.8, tol=1e-9)
    plain = ens.umbrella_mbar(W.NODE, 0.8, tol=1e-9, n_bootstrap=0)
    assert sorted(plain.keys()) == sorted(before.keys()) == sorted(['f', 'D', 'n_iter', 'last_delta', 'values', 'rows', 'periods', 'n_k', 'names'])
    assert plain['f'].tobytes() == before['f'].tobytes()
    for dec in (False, True):
        got = ens.umbrella_mbar(W.NODE, 0.8, tol=1e-9, decorrelate=dec, n_bootstrap=16, bootstrap_seed=4)
        n_k = got['n_k']; N = int(n_k.sum())
        origin = np.repeat(np.arange(8), n_k) if dec else np.tile(np.arange(8), 200)
        assert got['boot_counts'].shape == (16, N) and got['f_boot'].shape == (16, 8)
        for k in range(8):      # every window keeps its count in every replicate: the origins follow the layout of values
            assert (got['boot_counts'][:, origin == k].sum(axis=1) == n_k[k]).all(), (dec, k)
        assert got['boot_counts'].tobytes() == pkg.mbar.bootstrap_counts(n_k, 16, seed=4, state_of_sample=origin).tobytes()
        direct = bootstrap(got['values'], None, 1. / 0.8, got['rows'], n_k, got['f'], origin, counts=got['boot_counts'], periods=got['periods'], tol=1e-9)
        s = got['sigma_boot']
        print('decorrelate=%s: %d samples, n_k = %s, %d of 16 replicates converged in %d .. %d iterations; sigma_boot(f_k - f_0) = %s' %
              (dec, N, n_k.tolist(), got['n_boot_converged'], direct['n_iter'].min(), direct['n_iter'].max(), np.round(s[:, 0], 4).tolist()))
        assert got['f_boot'].tobytes() == direct['f_boot'].tobytes()
        assert got['n_boot_converged'] == int(direct['converged'].sum()) >= 2
        assert np.isfinite(s).all() and np.array_equal(s, s.T) and (np.diag(s) == 0).all()
        # one yardstick iteration from a converged replicate's f with ITS counts leaves it where it is (10 tol, as in the convergence check)
        b = int(np.flatnonzero(direct['converged'])[0])
        u = M.reduced_energy(got['values'], None, np.full(8, 1. / 0.8), got['rows'], got['periods'])
        moved = float(np.abs(R.iterate(u, n_k, got['f_boot'][b], got['boot_counts'][b])[0] - got['f_boot'][b]).max())
        print('one yardstick iteration moves replicate %d by %.3e (bound 1e-8)' % (b, moved))
        assert moved < 1e-8
        if dec:
            assert 't0' in got and 'kept' in got
        else:
            sigma_interleaved = s
    # the same ladder from files through tools/umbrella_mbar.py --bootstrap 16 --seed 4: there the samples are grouped by window, the
    # draw of a window goes to the same frames, and only the order of the sums differs from the interleaved call above
    import contextlib
    import importlib.util
    import io
    series = ens.read_cvs(reset=False)
    ens.close()
    for w, path in enumerate(fs):
        pkg.config.add_collective_variables(path, [bare])
        with pkg.h5lite.open_file(path, 'r+') as f:
            out = f.create_group('output') if 'output' not in f.keys() else f.group('output')
            out.write('cv', np.ascontiguousarray(series[:, w:w + 1, :]))
    spec_ = importlib.util.spec_from_file_location('umbrella_mbar_tool', os.path.join(P.ROOT, 'tools', 'umbrella_mbar.py'))
    tool = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(tool)
    argv, text = sys.argv, io.StringIO()
    sys.argv = ['umbrella_mbar.py', '--temperature', '0.8', '--node', W.NODE, '--tol', '1e-9', '--bins', '8', '--bootstrap', '16', '--seed', '4'] + list(fs)
    try:
        with contextlib.redirect_stdout(text):
            tool.main()
    finally:
        sys.argv = argv
    lines = text.getvalue().splitlines()
    print('\n'.join(lines[:4] + ['...'] + lines[-3:]))
    table = [l.split() for l in lines if not l.startswith('#')]
    windows, bins = np.array(table[:8], 'f8'), np.array(table[8:], 'f8')
    assert windows.shape == (8, 5) and bins.shape == (8, 3) and 'bootstrap sigma' in '\n'.join(lines)
    err = float(np.abs(windows[:, 4] - sigma_interleaved[:, 0]).max())
    print('the printed bootstrap sigma against umbrella_mbar(n_bootstrap=16, bootstrap_seed=4): largest difference %.3e (six decimals are printed)' % err)
    assert err < 1e-5
    full = np.isfinite(bins[:, 1])
    assert full.any() and np.isfinite(bins[full, 2]).all() and bins[np.argmin(bins[:, 1]), 2] == 0. and (bins[full, 2] >= 0.).all()


def refusals(work):
    good, cases = C.boot_refusal_cases()
    ok = bootstrap(**good)
    for label, change, fragment in cases:
        kw = dict(good); kw.update(change)
        try:
            bootstrap(**kw)
        except RuntimeError as err:
            print('%-34s refused: %s' % (label, err))
            assert fragment in str(err), (label, str(err))
        else:
            raise AssertionError('%s was accepted' % label)
    calc = pkg.default_library().calc
    for label, override, fragment in C.RAW_REFUSALS:
        rc, msg = C.raw_call(calc, good, **override)
        print('%-34s refused: %s' % (label, msg))
        assert rc == 1 and fragment in msg, (label, msg)
    again = bootstrap(**good)
    assert again['f_boot'].tobytes() == ok['f_boot'].tobytes() and np.isfinite(again['f_boot']).all()
    want = R.solve(energies(good), good['n_k'], good['counts'], 0., 3)
    assert ratio(again['f_boot'], want['f_boot']) <= 1.
    print('a good call after the refusals returns the bits of the one before them')


CHECKS = dict(fixed_d0=lambda w: fixed(w, 0), fixed_d1=lambda w: fixed(w, 1), fixed_d2=lambda w: fixed(w, 2), fixed_d8=lambda w: fixed(w, 8),
              duplication=duplication, convergence=convergence, independence=independence, columns=columns, count_range=count_range,
              end_to_end=end_to_end, refusals=refusals)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
