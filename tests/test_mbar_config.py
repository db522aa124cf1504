"""CPU tests of the MBAR yardstick tests/mbar_reference.py (float64 numpy, the statement of upside_hip_mbar) on cases with known
answers, of config.mbar_profile, and of the entry point's refusals, which return before any device call and so need no GPU."""
import os
import numpy as np
import pytest
import parity_util as P
import mbar_reference as M
from mbar_cases import small_case, refusal_cases

pkg = P.pkg
cfg = pkg.config


def test_one_state_has_zero_free_energy():
    c = small_case(K=1)
    r = M.mbar(tol=1e-12, max_iter=50, **c)
    assert r['f'].shape == (1,) and r['f'][0] == 0.
    assert r['n_iter'] == 1 and r['last_delta'] == 0.
    # D_n = ln N - u(n) for the one state
    u = M.reduced_energy(c['values'], None, c['beta'], c['rows'], c['periods'])[:, 0]
    assert np.allclose(r['D'], np.log(40.) - u, rtol=0, atol=1e-13)


def test_duplicated_states_get_equal_free_energies():
    c = small_case(K=3)
    for k in ('beta', 'rows', 'n_k'):
        c[k] = np.concatenate((c[k], c[k][1:2]))      # state 3 repeats state 1; its samples are counted to both
    c['n_k'] = np.array([40, 20, 40, 20], 'i8')
    r = M.mbar(tol=0, max_iter=60, **c)
    assert abs(r['f'][3] - r['f'][1]) < 1e-13
    # a state without samples still receives its free energy, and does not change the others'
    c2 = dict(c); c2['n_k'] = np.array([40, 40, 40, 0], 'i8')
    r2 = M.mbar(tol=0, max_iter=60, **c2)
    assert abs(r2['f'][3] - r2['f'][1]) < 1e-13
    c3 = small_case(K=3)
    r3 = M.mbar(tol=0, max_iter=60, **c3)
    assert np.abs(r2['f'][:3] - r3['f']).max() < 1e-13


def test_log_sums_equal_naive_sums_on_a_tiny_case():
    c = small_case(K=3, n=7, d=2)
    u = M.reduced_energy(c['values'], None, c['beta'], c['rows'], c['periods'])
    f = np.zeros(3)
    for _ in range(15):
        fl, _ = M.iterate(u, c['n_k'], f)
        fn = M.naive_iterate(u, c['n_k'], f)
        assert np.abs(fl - fn).max() < 1e-13
        f = fl


def test_wrap_flat_bottom_and_energy_enter_the_reduced_energy():
    v = np.array([[3.1, 1.0], [-3.1, 2.5]], 'f4')
    rows = np.array([[-3.0, 2.0, 4.0, 2.0, 0.0, 0.25]], 'f4')      # centres -3.0, 2.0; springs 4, 2; flat widths 0, 0.25
    e = np.array([1.5, -0.5])
    u = M.reduced_energy(v, e, [2.0], rows, [2 * np.pi, 0.])[:, 0]
    v64 = v.astype('f8')
    d0 = 2 * np.pi - (v64[0, 0] + 3.0)                              # across the cut
    want0 = 2.0 * (1.5 + 0.5 * 4.0 * d0 ** 2 + 0.5 * 2.0 * (1.0 - 0.25) ** 2)
    want1 = 2.0 * (-0.5 + 0.5 * 4.0 * (v64[1, 0] + 3.0) ** 2 + 0.5 * 2.0 * (0.5 - 0.25) ** 2)
    assert abs(u[0] - want0) < 1e-13 and abs(u[1] - want1) < 1e-13
    inside = M.reduced_energy(np.array([[0., 2.2]], 'f4'), None, [1.0], np.array([[0., 2., 0., 2., 0., 0.25]], 'f4'), [0., 0.])
    assert inside[0, 0] == 0.


def test_a_distant_state_stays_finite():
    c = small_case(K=3)
    c['rows'][2, 1] = 1e7; c['rows'][2, 0] = 150.       # u ~ 1e11
    r = M.mbar(tol=0, max_iter=5, target=(1.0, None), **c)
    assert np.isfinite(r['f']).all() and np.isfinite(r['D']).all() and np.isfinite(r['log_w']).all()
    assert r['f'][2] > 1e5


def test_sample_order_does_not_matter_and_the_seeded_cases_converge():
    for case in (M.case_harmonic(), M.case_periodic()):
        r = M.mbar(tol=1e-10, max_iter=2000, **case)
        assert r['last_delta'] < 1e-10 and r['n_iter'] < 2000
        perm = np.random.RandomState(5).permutation(len(case['values']))
        c2 = dict(case, values=case['values'][perm], energy=None if case['energy'] is None else case['energy'][perm])
        a = M.mbar(tol=0, max_iter=50, **case)['f']; b = M.mbar(tol=0, max_iter=50, **c2)['f']
        assert np.abs(a - b).max() < 1e-12
    # the harmonic case has a closed form: f_k - f_0 from the Gaussian integrals of exp(-beta (U + bias_k))
    h = M.case_harmonic()
    kT, k0, x0 = 0.8, 1.5, 6.0
    c = h['rows'][:, 0].astype('f8'); k = h['rows'][:, 1].astype('f8')
    exact = (0.5 * k0 * k / (k0 + k) * (c - x0) ** 2) / kT + 0.5 * np.log((k0 + k) / k0)
    exact -= exact[0]
    f = M.mbar(tol=1e-10, max_iter=2000, **h)['f']
    print('harmonic case: largest |f - exact| = %.3f kT (statistical, 500 samples per window)' % np.abs(f - exact).max())
    assert np.abs(f - exact).max() < 0.5


def test_target_weights_are_normalised():
    c = M.case_harmonic()
    r = M.mbar(tol=1e-10, max_iter=2000, target=(1.25, None), **c)
    assert abs(np.exp(r['log_w']).sum() - 1.) < 1e-12
    assert abs(r['f_target'] + M.logsumexp(-1.25 * c['energy'] - r['D'], 0)) < 1e-12


def test_profile_of_uniform_weights_is_the_histogram():
    rng = np.random.RandomState(9)
    v = rng.uniform(0., 4., 1000)
    edges = np.linspace(0., 5., 11)
    lw = np.full(1000, -np.log(1000.))
    F = cfg.mbar_profile(v, lw, edges, 0.8)
    count = np.histogram(v, edges)[0]
    assert np.isinf(F[count == 0]).all() and (F[count == 0] > 0).all() and (count == 0).sum() == 2
    ok = count > 0
    assert np.allclose(F[ok], -0.8 * np.log(count[ok] / 1000.), rtol=0, atol=1e-12)
    # a periodic CV: values a period away fall into the same bins
    edges = np.linspace(-np.pi, np.pi, 13)
    a = rng.uniform(-np.pi, np.pi, 500)
    shifted = a + 2 * np.pi * rng.randint(-2, 3, 500)
    assert np.allclose(cfg.mbar_profile(shifted, lw[:500], edges, 1.0, period=2 * np.pi), cfg.mbar_profile(a, lw[:500], edges, 1.0), rtol=0, atol=1e-9)
    # log-weights far below the double range of exp still give a finite profile
    assert np.isfinite(cfg.mbar_profile(a, np.full(500, -5000.), np.array([-4., 4.]), 1.0)).all()
    with pytest.raises(ValueError):
        cfg.mbar_profile(a, lw, edges, 1.0)


def test_the_entry_point_states_its_refusals():
    if not os.path.exists(pkg.PRODUCT_LIB):
        pytest.fail('libupside_hip.so not built (run __graft_entry__.build())')
    good, cases = refusal_cases()
    for label, change, fragment in cases:
        kw = dict(good, tol=0., max_iter=3); kw.update(change)
        with pytest.raises(RuntimeError) as err:
            pkg.mbar.mbar(**kw)
        assert fragment in str(err.value), (label, str(err.value))
    lib = pkg.default_library().calc
    assert lib.upk_mbar_state_tile() == pkg.mbar.STATE_TILE and lib.upk_mbar_fe_tile() == pkg.mbar.FE_TILE


def test_the_ladder_tool_reads_a_window_file(tmp_path):
    """tools/umbrella_mbar.py: read_window on a window file written here through h5lite -- a cv_restraint node on the second of two
    recorded CVs and an /output/cv of 7 frames in the layout upside_hip writes, (frame, 1, n_cv)"""
    import importlib.util
    import shutil
    spec = importlib.util.spec_from_file_location('umbrella_mbar_tool', os.path.join(P.ROOT, 'tools', 'umbrella_mbar.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = str(tmp_path / 'w0.up')
    shutil.copyfile(P.fixture('trpcage20_7A'), path)
    dist = {'name': 'end_to_end', 'kind': 'distance', 'pair': (1, 58)}
    phi = {'name': 'phi', 'kind': 'dihedral', 'atoms': (2, 3, 4, 5)}
    cfg.add_collective_variables(path, [{'name': 'rg_all', 'kind': 'rg', 'atoms': np.arange(60, dtype='i4')}, dist, phi])
    cfg.add_cv_restraint(path, [dict(phi, center=-1.0, spring_const=3.0), dict(dist, center=12.5, spring_const=2.0, flat_width=0.25)])
    cv = np.arange(21, dtype='f4').reshape(7, 1, 3)
    with pkg.h5lite.open_file(path, 'r+') as f:
        out = f.create_group('output') if 'output' not in f.keys() else f.group('output')
        out.write('cv', cv)
    series, recorded, names, row, periods = tool.read_window(pkg.h5lite, cfg, path, 'cv_restraint')
    assert series.shape == (7, 3) and np.array_equal(series, cv[:, 0])
    assert recorded == ['rg_all', 'end_to_end', 'phi'] and names == ['phi', 'end_to_end']
    assert row.dtype == np.float32 and row.tolist() == [-1.0, 12.5, 3.0, 2.0, 0.0, 0.25]
    assert periods.tolist() == [2 * np.pi, 0.]
    with pytest.raises(SystemExit) as err:
        tool.read_window(pkg.h5lite, cfg, path, 'cv_restraint_other')
    assert 'cv_restraint_other' in str(err.value)
    with pytest.raises(SystemExit) as err:
        tool.read_window(pkg.h5lite, cfg, P.fixture('trpcage20_7A'), 'cv_restraint')
    assert 'collective_variables' in str(err.value)
