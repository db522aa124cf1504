"""Child process of tests/test_gpu_mbar_boot_draw.py: one check of the device draw of the MBAR bootstrap counts
(upside_hip_mbar_bootstrap_counts, upside_hip_mbar_bootstrap_drawn; k_mbar_boot_draw* of csrc/kernels_mbar_boot.hip) per invocation,

    python tests/mbar_boot_draw_gpu_worker.py CHECK WORKDIR

prints every figure it compares before it asserts and ends with 'CHECK <name> PASSED'.  The yardstick is
tests/mbar_boot_draw_reference.py (integer numpy, pinned by tests/test_mbar_boot_draw_config.py); the inputs are
tests/mbar_boot_draw_cases.py and tests/mbar_bootstrap_cases.py.  Counts are integers and the solve is deterministic: every comparison
is equality, of counts or of bits."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                  # noqa: E402
import mbar_reference as M               # noqa: E402
import mbar_bootstrap_cases as C         # noqa: E402
import mbar_boot_draw_reference as D     # noqa: E402
import mbar_boot_draw_cases as DC        # noqa: E402

pkg = P.pkg
E = pkg.engine
bootstrap = pkg.mbar.bootstrap
draw = pkg.mbar.bootstrap_counts_device
KEYS = ('f_boot', 'columns', 'n_iter', 'last_delta')


def draw_equals_reference(work):
    assert pkg.mbar.BOOT_DRAW_TILE == DC.T
    n_k = np.array(DC.DRAW_N_K, 'i8')
    start = np.concatenate(([0], np.cumsum(n_k)))
    shuffled = DC.shuffled_origins(n_k)
    for block in DC.DRAW_BLOCKS:
        want = D.counts(n_k, 5, seed=DC.SEED, block=block)      # one yardstick draw serves both layouts: the layout permutes it
        for name, sos in (('grouped', None), ('shuffled', shuffled)):
            got = draw(n_k, 5, seed=DC.SEED, state_of_sample=sos, block=block)
            ref = want if sos is None else D.counts(n_k, 5, seed=DC.SEED, state_of_sample=sos, block=block)
            wrong = int((got != ref).sum())
            grouped = got if sos is None else got[:, np.argsort(sos, kind='stable')]
            sums = np.array([grouped[:, start[k]:start[k + 1]].sum(axis=1, dtype='i8') for k in range(len(n_k))]).T
            print('block %s, %s: %d x %d counts, %d differ from the yardstick; largest count %d; per-state sums equal n_k: %s' %
                  ('absent' if block is None else block, name, got.shape[0], got.shape[1], wrong, got.max(), bool((sums == n_k).all())))
            assert got.dtype == np.uint16 and got.shape == ref.shape
            assert wrong == 0 and (sums == n_k).all()
            if sos is not None:
                assert np.array_equal(grouped, want)


def independence(work):
    n_k = np.array(DC.DRAW_N_K, 'i8')
    block = DC.DRAW_BLOCKS[2]
    nine = draw(n_k, 9, seed=DC.SEED, block=block)
    part = draw(n_k, 2, seed=DC.SEED, block=block, first=3)
    again = draw(n_k, 9, seed=DC.SEED, block=block)
    print('replicates 3..4 by first=3 equal rows 3..4 of nine: %s; two calls give the same bits: %s' %
          (np.array_equal(part, nine[3:5]), nine.tobytes() == again.tobytes()))
    assert np.array_equal(part, nine[3:5]) and nine.tobytes() == again.tobytes()
    assert not np.array_equal(nine[3], nine[4])
    case = M.case_periodic()
    N = int(case['n_k'].sum())
    f = C.converged_start(case)
    kw = dict(case, f=f, tol=C.TOL, max_iter=5000, n_bootstrap=5, seed=DC.SEED, draw='device', block=4, want_counts=True)
    full = bootstrap(**kw)
    work_bytes = 8 * N * 2 + 3
    assert pkg.mbar.boot_chunk(N, work_bytes) == 2
    small = bootstrap(workspace_bytes=work_bytes, **kw)
    same_counts = full['counts'].tobytes() == small['counts'].tobytes()
    same = all(full[k].tobytes() == small[k].tobytes() for k in KEYS if k in full)
    print('bootstrap(draw=device) in chunks of 2 against the default workspace: the same counts: %s, the same f_boot, n_iter, last_delta: %s' % (same_counts, same))
    assert same_counts and same
    assert np.array_equal(full['counts'], D.counts(case['n_k'], 5, seed=DC.SEED, block=4))
    assert full['seed'] == DC.SEED and full['block'].tolist() == [4] * len(case['n_k'])
    bare = bootstrap(**dict(kw, want_counts=None))
    assert 'counts' not in bare and bare['f_boot'].tobytes() == full['f_boot'].tobytes()


def solve_equals_host_fed(work):
    case = M.case_periodic()
    n_k = case['n_k']
    f = C.converged_start(case)
    cols, _ = C.profile_columns(case, np.linspace(-np.pi, np.pi, 7))
    kw = dict(case, f=f, tol=C.TOL, max_iter=5000, log_numerators=cols)
    for block in (None, 6, np.arange(1, len(n_k) + 1) * 3):
        got = bootstrap(n_bootstrap=12, seed=DC.SEED, draw='device', block=block, want_counts=True, **kw)
        fed = bootstrap(counts=got['counts'], **kw)
        same = dict((k, got[k].tobytes() == fed[k].tobytes()) for k in KEYS)
        yard = np.array_equal(got['counts'], D.counts(n_k, 12, seed=DC.SEED, block=block))
        print('block %s: 12 replicates, %d .. %d iterations, %d converged; drawn on the device against the old entry point fed those counts, bit-identical: %s; '
              'the counts are the yardstick\'s: %s' % ('absent' if block is None else np.asarray(block).tolist(), got['n_iter'].min(), got['n_iter'].max(),
                                                      int(got['converged'].sum()), same, yard))
        assert all(same.values()) and yard
        assert np.isfinite(got['f_boot']).all() and got['converged'].all()


def end_to_end(work):
    import mbar_gpu_worker as W
    fs, spec, centers, pos0 = W.ladder(work)
    ens = E.Ensemble.from_files(fs)
    ens.set_pos(pos0.astype('f4'))
    ens.init_md(0.8, 21)
    bare = dict((k, v) for k, v in spec.items() if k not in pkg.config.CV_RESTRAINT_VALUES)
    ens.define_cvs([bare])
    # a synthetic series in place of a long run: every window around its centre, modulated by an AR(1) process (phi = 0.8, unit variance)
    rng = np.random.default_rng(9)
    T = 600
    series = np.stack([centers[s] + 0.5 * DC.ar1(T, 0.8, rng) * np.sqrt(1. - 0.8 ** 2) for s in range(8)], axis=1)[:, :, None].astype('f4')
    before = ens.umbrella_mbar(W.NODE, 0.8, tol=1e-9, series=series)
    assert sorted(before.keys()) == sorted(['f', 'D', 'n_iter', 'last_delta', 'values', 'rows', 'periods', 'n_k', 'names'])
    host = ens.umbrella_mbar(W.NODE, 0.8, tol=1e-9, series=series, n_bootstrap=16, bootstrap_seed=4)
    assert sorted(host.keys()) == sorted(list(before.keys()) + ['f_boot', 'sigma_boot', 'n_boot_converged', 'boot_counts'])
    got = ens.umbrella_mbar(W.NODE, 0.8, tol=1e-9, series=series, n_bootstrap=16, bootstrap_seed=4, bootstrap_draw='device', bootstrap_block='auto')
    assert sorted(got.keys()) == sorted(list(before.keys()) + ['f_boot', 'sigma_boot', 'n_boot_converged', 'boot_block', 'boot_g']) and 'boot_counts' not in got
    n_k = got['n_k']
    per_window = np.ascontiguousarray(series[:, :, :1].transpose(1, 0, 2))
    bias = pkg.mbar.own_state_reduced_bias(per_window.reshape(-1, 1), 1. / 0.8, got['rows'], got['periods'], np.repeat(np.arange(8), T)).reshape(8, -1)
    g = pkg.timeseries.statistical_inefficiency(bias)['g'][:, 0]
    want_block = pkg.mbar.block_lengths(g)
    print('statistical inefficiency of the windows\' own reduced bias: %s; block lengths %s, returned %s' %
          (np.round(g, 3).tolist(), want_block.tolist(), got['boot_block'].tolist()))
    assert np.array_equal(got['boot_block'], want_block) and np.array_equal(got['boot_g'], g) and (want_block > 1).all()
    origin = np.tile(np.arange(8), T)
    counts = D.counts(n_k, 16, seed=4, state_of_sample=origin, block=want_block)
    direct = bootstrap(got['values'], None, 1. / 0.8, got['rows'], n_k, got['f'], origin, counts=counts, periods=got['periods'], tol=1e-9)
    s = got['sigma_boot']
    print('16 replicates drawn on the device in blocks: %d converged; f_boot equals the old entry point fed the yardstick\'s counts bit for bit: %s; '
          'sigma_boot(f_k - f_0) = %s; with the host draw of single samples %s' %
          (got['n_boot_converged'], got['f_boot'].tobytes() == direct['f_boot'].tobytes(), np.round(s[:, 0], 4).tolist(), np.round(host['sigma_boot'][:, 0], 4).tolist()))
    assert got['f_boot'].tobytes() == direct['f_boot'].tobytes()
    assert got['n_boot_converged'] == int(direct['converged'].sum()) >= 2
    assert np.isfinite(s).all() and np.array_equal(s, s.T) and (np.diag(s) == 0).all()
    # a fixed block for every window, one per window, and what the options refuse
    fixed = ens.umbrella_mbar(W.NODE, 0.8, tol=1e-9, series=series, n_bootstrap=4, bootstrap_draw='device', bootstrap_block=7)
    assert fixed['boot_block'].tolist() == [7] * 8 and fixed['boot_g'] is None
    plain = ens.umbrella_mbar(W.NODE, 0.8, tol=1e-9, series=series, n_bootstrap=4, bootstrap_draw='device')
    assert plain['boot_block'] is None and plain['boot_g'] is None and 'boot_counts' not in plain
    for kw in (dict(bootstrap_block='auto', decorrelate=True, bootstrap_draw='device'), dict(bootstrap_block=3), dict(bootstrap_draw='gpu'),
               dict(bootstrap_block='most', bootstrap_draw='device')):
        try:
            ens.umbrella_mbar(W.NODE, 0.8, tol=1e-9, series=series, n_bootstrap=4, **kw)
        except ValueError as err:
            print('%s refused: %s' % (kw, err))
        else:
            raise AssertionError('%s was accepted' % kw)
    ens.close()
    # the same series from files through tools/umbrella_mbar.py: there the samples are grouped by window, the counts of a window are the
    # same (they do not depend on the layout), and only the order of the sums differs
    import contextlib
    import importlib.util
    import io
    for w, path in enumerate(fs):
        pkg.config.add_collective_variables(path, [bare])
        with pkg.h5lite.open_file(path, 'r+') as f:
            out = f.create_group('output') if 'output' not in f.keys() else f.group('output')
            out.write('cv', np.ascontiguousarray(series[:, w:w + 1, :]))
    spec_ = importlib.util.spec_from_file_location('umbrella_mbar_tool', os.path.join(P.ROOT, 'tools', 'umbrella_mbar.py'))
    tool = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(tool)
    argv, text = sys.argv, io.StringIO()
    sys.argv = ['umbrella_mbar.py', '--temperature', '0.8', '--node', W.NODE, '--tol', '1e-9', '--bins', '8', '--bootstrap', '16', '--seed', '4',
                '--bootstrap-draw', 'device', '--bootstrap-block', 'auto'] + list(fs)
    try:
        with contextlib.redirect_stdout(text):
            tool.main()
    finally:
        sys.argv = argv
    lines = text.getvalue().splitlines()
    print('\n'.join(lines[:5] + ['...'] + lines[-3:]))
    table = [l.split() for l in lines if not l.startswith('#')]
    windows, bins = np.array(table[:8], 'f8'), np.array(table[8:], 'f8')
    assert windows.shape == (8, 5) and bins.shape == (8, 3) and 'bootstrap sigma' in '\n'.join(lines)
    assert any(l.startswith('# bootstrap blocks') and str(want_block.tolist()) in l for l in lines)
    err = float(np.abs(windows[:, 4] - s[:, 0]).max())
    print('the printed bootstrap sigma against umbrella_mbar(bootstrap_draw=device, bootstrap_block=auto): largest difference %.3e (six decimals are printed)' % err)
    assert err < 1e-5
    full = np.isfinite(bins[:, 1])
    assert full.any() and np.isfinite(bins[full, 2]).all() and bins[np.argmin(bins[:, 1]), 2] == 0. and (bins[full, 2] >= 0.).all()


def refusals(work):
    good, cases = DC.drawn_refusal_cases()
    good = dict(good, want_counts=True)
    ok = bootstrap(**good)
    first = draw(**DC.COUNTS_GOOD)
    calc = pkg.default_library().calc
    for label, change, fragment in cases:
        try:
            bootstrap(**dict(good, **change))
        except RuntimeError as err:
            print('%-36s refused: %s' % (label, err))
            assert fragment in str(err) and 'mbar_bootstrap_drawn: ' in str(err), (label, str(err))
        else:
            raise AssertionError('%s was accepted' % label)
    for label, override, fragment in DC.RAW_DRAWN_REFUSALS:
        rc, msg = DC.raw_drawn(calc, good, **override)
        print('%-36s refused: %s' % (label, msg))
        assert rc == 1 and fragment in msg, (label, msg)
    for label, change, fragment in DC.COUNTS_REFUSALS:
        try:
            draw(**dict(DC.COUNTS_GOOD, **change))
        except RuntimeError as err:
            print('%-36s refused: %s' % (label, err))
            assert fragment in str(err) and 'mbar_bootstrap_counts: ' in str(err), (label, str(err))
        else:
            raise AssertionError('%s was accepted' % label)
    for label, override, fragment in DC.RAW_COUNTS_REFUSALS:
        rc, msg = DC.raw_counts(calc, **override)
        print('%-36s refused: %s' % (label, msg))
        assert rc == 1 and fragment in msg, (label, msg)
    again = bootstrap(**good)
    assert again['f_boot'].tobytes() == ok['f_boot'].tobytes() and again['counts'].tobytes() == ok['counts'].tobytes() and np.isfinite(again['f_boot']).all()
    assert np.array_equal(again['counts'], D.counts(good['n_k'], 2, seed=5))
    assert draw(**DC.COUNTS_GOOD).tobytes() == first.tobytes()
    kw = DC.COUNTS_GOOD
    assert np.array_equal(first, D.counts(kw['n_k'], kw['n_bootstrap'], seed=kw['seed'], block=kw['block'], first=kw['first']))
    print('good calls after the refusals return the bits of the ones before them, and the yardstick\'s counts')


CHECKS = dict(draw_equals_reference=draw_equals_reference, independence=independence, solve_equals_host_fed=solve_equals_host_fed,
              end_to_end=end_to_end, refusals=refusals)

if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'these checks need a GPU'
    which, workdir = sys.argv[1], sys.argv[2]
    CHECKS[which](workdir)
    print('CHECK %s PASSED' % which)
