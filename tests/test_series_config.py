"""CPU tests of the time-series yardstick tests/series_reference.py (float64 numpy, the statement of upside_hip_series_inefficiency)
against brute force and theory, of the host-side pieces of upside-md_amd/timeseries.py and mbar.own_state_reduced_bias, and of the
margins the GPU checks of tests/test_gpu_series.py rest their exact comparisons on.  None of them needs a GPU."""
import os
import numpy as np
import pytest
import parity_util as P
import mbar_reference as M
import series_reference as R
import series_cases as C
from mbar_cases import stressed_case

pkg = P.pkg
ts = pkg.timeseries


def brute_force(A, mintime, max_lag):
    """the definition with scalar loops only"""
    Tt = len(A)
    mu = sum(A) / Tt
    s2 = sum((x - mu) ** 2 for x in A) / Tt
    g, stop = 1., None
    t = 1
    while True:
        if t == Tt - 1 or (max_lag is not None and t == max_lag + 1):
            stop = t
            break
        c = 0.
        for n in range(Tt - t):
            c += (A[n] - mu) * (A[n + t] - mu)
        c /= (Tt - t) * s2
        if c <= 0. and t > mintime:
            stop = t
            break
        g += 2. * c * (1. - t / Tt)
        t += 1
    return max(1., g), stop, mu, s2


def test_yardstick_equals_an_independent_double_loop():
    rng = np.random.RandomState(2)
    for phi in (0., 0.6, 0.95):
        a = R.ar1(rng, 40, phi)[0] + 2.
        for mintime, max_lag in ((3, None), (1, None), (10, None), (3, 5), (3, 1)):
            for t0 in (0, 7, 24):
                r = R.statistical_inefficiency(a, [t0], mintime, max_lag)
                g, stop, mu, s2 = brute_force([float(x) for x in a[t0:]], mintime, max_lag)
                assert abs(r['g'][0, 0] - g) <= 1e-12 * g and r['stop_lag'][0, 0] == stop, (phi, mintime, max_lag, t0)
                assert abs(r['mean'][0, 0] - mu) <= 1e-13 and abs(r['variance'][0, 0] - s2) <= 1e-13
                assert r['n_eff'][0, 0] == (40 - t0) / r['g'][0, 0]
    # the two cases that are no error: a tail below 16 samples and a constant tail
    r = R.statistical_inefficiency(np.arange(40.), [0, 24, 25, 39, 40, 50])
    assert r['g'][0].tolist()[2:] == [0., 0., 0., 0.] and r['stop_lag'][0].tolist()[2:] == [-1, -1, -1, -1] and r['g'][0, 1] >= 1.
    assert r['n_eff'][0].tolist()[2:] == [0., 0., 0., 0.]
    r = R.statistical_inefficiency(np.full(40, 2.5), [0, 3])      # (a constant whose sums are exact: the mean is the constant)
    assert r['g'].tolist() == [[1., 1.]] and r['stop_lag'].tolist() == [[0, 0]] and r['variance'].tolist() == [[0., 0.]]
    # lengths: what lies past a series' length does not count
    a = R.ar1(rng, 60, 0.5, K=2)
    b = a.copy(); b[1, 45:] = np.nan
    r = R.statistical_inefficiency(b, [0, 10], lengths=[60, 45])
    assert r['g'][1, 1] == R.statistical_inefficiency(a[1, :45], [10])['g'][0, 0] and np.isfinite(r['g']).all()


def test_yardstick_gives_the_inefficiency_of_an_ar1_series():
    """AR(1) with phi = 0.5 has g = (1 + phi) / (1 - phi) = 3; 2^17 samples, seed 4; the estimator's own scatter at this length is
    about g sqrt(2 (2 L + 1) / T) ~ 2 % for L ~ 15 lags, the bound is 10 %"""
    x = R.ar1(np.random.RandomState(4), 1 << 17, 0.5)[0]
    r = R.statistical_inefficiency(x)
    print('AR(1), phi = 0.5, 2^17 samples, seed 4: g = %.4f (theory 3), stop_lag %d' % (r['g'][0, 0], r['stop_lag'][0, 0]))
    assert abs(r['g'][0, 0] - 3.) <= 0.3


def test_subsample_indices_on_hand_written_cases():
    s = ts.subsample_indices
    assert s(5, 0, 1.).tolist() == [0, 1, 2, 3, 4]
    assert s(7, 0, 2.0).tolist() == [0, 2, 4, 6]
    assert s(7, 0, 2.01).tolist() == [0, 3, 6]
    assert s(10, 4, 2.5).tolist() == [4, 7]
    assert s(10, 8, 3.).tolist() == [8]           # a tail shorter than one stride keeps its first sample
    assert s(10, 10, 3.).tolist() == [] and s(10, 0, 0.).tolist() == []      # nothing there; no estimate
    assert s(9, 2, 1.5).dtype == np.int64
    for args in ((5, 0, 1.), (7, 0, 2.01), (10, 4, 2.5), (10, 0, 0.)):
        assert ts.subsample_indices(*args).tolist() == R.subsample_indices(*args).tolist()
    assert ts.equilibration_origins(1000).tolist() == (15 * np.arange(64)).tolist() == R.equilibration_origins(1000).tolist()
    assert ts.equilibration_origins(40).tolist() == list(range(40)) and ts.equilibration_origins(200, 8).tolist() == (25 * np.arange(8)).tolist()
    assert (ts.MIN_TAIL, R.MIN_TAIL) == (16, 16)


def test_own_state_reduced_bias_is_the_diagonal_of_the_reduced_energies():
    for name, case in (('periodic', M.case_periodic()), ('flat-bottomed', stressed_case(257, 5, 1, 31))):
        assert case['energy'] is None
        n_k = case['n_k']
        state = np.repeat(np.arange(len(n_k)), n_k)
        u = M.reduced_energy(case['values'], None, case['beta'], case['rows'], case['periods'])
        got = pkg.mbar.own_state_reduced_bias(case['values'], case['beta'], case['rows'], case['periods'], state)
        err = float(np.abs(got - u[np.arange(len(state)), state]).max())
        print('%s: %d samples, largest |own_state_reduced_bias - diag u| = %.3e (bound 1e-12), largest u %.3e' % (name, len(state), err, got.max()))
        assert got.dtype == np.float64 and got.shape == (len(state),) and err <= 1e-12
        assert (got > 0).any()
    with pytest.raises(ValueError):
        pkg.mbar.own_state_reduced_bias(np.zeros((4, 1), 'f4'), 1., np.zeros((2, 3), 'f4'), None, [0, 1, 2, 0])


def test_detect_equilibration_of_the_yardstick():
    d = R.detect_equilibration(C.drift_series())
    print('drift: t0 %d, g %.4f, n_eff %.2f, gap %.3e' % (d['t0'][0], d['g'][0], d['n_eff'][0], d['gap'][0]))
    assert d['t0'][0] > 0
    w = R.detect_equilibration(C.white_series())
    print('white: t0 %d, g %.4f' % (w['t0'][0], w['g'][0]))
    assert w['t0'][0] == 0 and w['g'][0] == 1.


def test_the_parity_cases_keep_their_margins():
    """what the exact comparisons of tests/test_gpu_series.py rest on, on the yardstick alone: |C(t)| >= 1e-6 at every lag where a
    stop is decided and a gap of 1e-3 between the best and the second-best origin, for the shortest and the seed that was replaced"""
    for T in (16, 63):
        a = C.parity_batch(T)
        for n_origin in (1, 8):
            r = R.statistical_inefficiency(a, C.parity_origins(T, n_origin))
            assert r['c_margin'].min() >= C.C_MARGIN
            if n_origin == 8:
                s = np.sort(r['n_eff'], axis=1)
                assert ((s[:, -1] - s[:, -2]) >= C.GAP * s[:, -1]).all()


def test_the_entry_point_states_its_refusals():
    """the refusals of upside_hip_series_inefficiency return before any device call, so they are the same with and without a GPU"""
    if not os.path.exists(pkg.PRODUCT_LIB):
        pytest.fail('libupside_hip.so not built (run __graft_entry__.build())')
    a = C.parity_batch(64, 3)
    for label, kw, fragment in C.refusal_cases(a):
        with pytest.raises(RuntimeError) as err:
            ts.statistical_inefficiency(**kw)
        assert fragment in str(err.value), (label, str(err.value))
    lib = pkg.default_library().calc
    assert lib.upk_series_lag_block() == ts.LAG_BLOCK and lib.upk_series_piece() == ts.PIECE
