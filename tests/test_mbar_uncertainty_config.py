"""CPU tests of the MBAR uncertainties: mbar.covariance (eq. D9 of Shirts & Chodera 2008, on the M x M Gram matrix) against the
yardstick tests/mbar_uncertainty_reference.py (eq. D8 with the N x N pseudo-inverse, a different formula), and the predicted
standard deviations against the empirical spread over 200 re-drawn data sets.  No device is needed: the Gram matrices here are
built in numpy; the device's are checked by tests/test_gpu_mbar_uncertainty.py."""
import numpy as np
import pytest
import parity_util as P
import mbar_reference as M
import mbar_uncertainty_reference as U

mbar = P.pkg.mbar
KT = 0.8
EDGES = np.linspace(4., 9., 11)
TARGET = (1. / KT, None)


def d9_cases():
    yield 'harmonic', M.case_harmonic(), None
    yield 'periodic', M.case_periodic(), None
    c = U.emptied(M.case_harmonic())
    yield 'harmonic, windows 2 and 5 empty, 12 extra columns', c, U.extra_columns(len(c['values']), 12, 7)


@pytest.mark.parametrize('which', [0, 1, 2])
def test_covariance_from_the_gram_matrix_equals_the_n_by_n_formula(which):
    """var(f_i - f_j) of every pair of columns by D9 on G = W.T @ W within 1e-10 of D8 on W itself, relative to the variance"""
    name, case, cols = list(d9_cases())[which]
    u = U.energies(case)
    f = U.solve(u, case['n_k'])
    W, _ = U.weights(u, case['n_k'], f, cols)
    want = U.pair_variance(U.theta_d8(W, case['n_k']))
    got = U.pair_variance(mbar.covariance(W.T @ W, case['n_k']))
    off = ~np.eye(len(want), dtype=bool)
    rel = float((np.abs(got - want)[off] / want[off]).max())
    print('%s: M = %d, var(f_i - f_j) in [%.3e, %.3e]; largest |D9 - D8| / D8 = %.3e' % (name, len(want), want[off].min(), want[off].max(), rel))
    assert (want[off] > 0).all() and np.abs(np.diag(got)).max() < 1e-12
    assert rel <= 1e-10


@pytest.fixture(scope='module')
def spread():
    """200 re-draws of case_harmonic (seeds 100 .. 299), each solved by the yardstick: f_k - f_0, <x> at the unbiased target and
    F_b - F_r over 10 bins on [4, 9]; and the predictions from the draw with seed 11"""
    case = M.case_harmonic(11)
    u = U.energies(case); n_k = case['n_k']
    f = U.solve(u, n_k)
    x = case['values'][:, 0].astype('f8')
    W, _ = U.weights(u, n_k, f)
    pred = dict(sigma=np.sqrt(U.pair_variance(mbar.covariance(W.T @ W, n_k))[:, 0]))
    Pinv = U.inner_pinv(W, n_k)
    lw = U.target_log_weights(case, u, n_k, f, TARGET)
    mean, var = U.expectation(u, n_k, f, lw, x, Pinv)
    pred['mean'], pred['mean_sigma'] = float(mean[0]), float(np.sqrt(var[0]))
    F, varF = U.profile(u, n_k, f, lw, x, EDGES, KT, Pinv)
    pred['F'], pred['dF'] = F, np.sqrt(varF)
    r = int(np.argmin(F))
    fs, means, Fs = [], [], []
    for seed in range(100, 300):
        c = M.case_harmonic(seed)
        uc = U.energies(c)
        fc = U.solve(uc, n_k, tol=1e-11)
        lwc = U.target_log_weights(c, uc, n_k, fc, TARGET)
        xc = c['values'][:, 0].astype('f8')
        fs.append(fc - fc[0]); means.append(float((np.exp(lwc) * xc).sum()))
        b = U.bin_index(xc, EDGES); w = np.exp(lwc)
        Fc = -KT * np.log(np.array([w[b == i].sum() for i in range(10)]))
        Fs.append(Fc - Fc[r])
    return dict(pred=pred, f=np.array(fs), mean=np.array(means), F=np.array(Fs), r=r)


def test_predicted_sigma_of_free_energies_matches_the_spread_of_redraws(spread):
    """sigma(f_k - f_0) predicted from one data set over the standard deviation of 200 re-draws lies in [0.8, 1.2] for every window
    (the standard deviation of 200 draws carries about 5 %)"""
    emp = spread['f'].std(axis=0, ddof=1)[1:]
    ratio = spread['pred']['sigma'][1:] / emp
    print('predicted sigma(f_k - f_0): %s\nempirical: %s\nratio: %s' % (np.round(spread['pred']['sigma'][1:], 4), np.round(emp, 4), np.round(ratio, 3)))
    assert (ratio >= 0.8).all() and (ratio <= 1.2).all()


def test_predicted_sigma_of_an_average_matches_the_spread_of_redraws(spread):
    """<x> in the unbiased state at kT = 0.8: predicted sigma over the empirical one in [0.8, 1.2]"""
    emp = spread['mean'].std(ddof=1)
    print('<x> = %.4f, predicted sigma %.4f, empirical %.4f over 200 re-draws' % (spread['pred']['mean'], spread['pred']['mean_sigma'], emp))
    assert 0.8 <= spread['pred']['mean_sigma'] / emp <= 1.2


def test_predicted_sigma_of_a_profile_matches_the_spread_of_redraws(spread):
    """dF of 10 bins over [4, 9] relative to the lowest bin: predicted over empirical in [0.8, 1.2] for every other bin"""
    r = spread['r']
    emp = spread['F'].std(axis=0, ddof=1)
    other = np.arange(10) != r
    ratio = spread['pred']['dF'][other] / emp[other]
    print('predicted dF: %s\nempirical: %s\nratio: %s' % (np.round(spread['pred']['dF'], 4), np.round(emp, 4), np.round(ratio, 3)))
    assert np.isfinite(spread['F']).all() and spread['pred']['dF'][r] == 0.
    assert (ratio >= 0.8).all() and (ratio <= 1.2).all()


def test_newton_steps_of_the_yardstick_reach_the_fixed_point_of_the_iteration():
    """pins the YARDSTICK, not the product (it passes without the feature): the solver of tests/mbar_uncertainty_reference.py against
    plain iteration of tests/mbar_reference.py gives the same f within 1e-9"""
    case = M.case_periodic()
    u = U.energies(case)
    f = U.solve(u, case['n_k'])
    want = M.mbar(tol=1e-12, max_iter=5000, **case)['f']
    assert np.abs(f - want).max() < 1e-9
    _, gmax = U.newton_step(u, case['n_k'], f)
    assert gmax < 1e-8


def test_the_gram_entry_point_states_its_refusals():
    """the refusals of upside_hip_mbar_gram return before any device call, so they are the same with and without a GPU; the accessors
    give the tile and the slab length of a workspace"""
    import os
    from mbar_uncertainty_cases import gram_refusal_cases, GRAM_TILE, GRAM_GRANULE
    if not os.path.exists(P.pkg.PRODUCT_LIB):
        pytest.fail('libupside_hip.so not built (run __graft_entry__.build())')
    good, cases = gram_refusal_cases()
    for label, change, fragment in cases:
        kw = dict(good); kw.update(change)
        with pytest.raises((RuntimeError, ValueError)) as err:
            mbar.gram(**kw)
        assert fragment in str(err.value), (label, str(err.value))
    import ctypes as ct
    lib = P.pkg.default_library().calc
    lib.upk_mbar_gram_rows.restype = ct.c_longlong
    lib.upk_mbar_gram_rows.argtypes = [ct.c_int, ct.c_size_t]
    assert lib.upk_mbar_gram_tile() == GRAM_TILE == mbar.GRAM_TILE
    lib.upk_mbar_gram_partial_bytes.restype = ct.c_size_t
    front = lib.upk_mbar_gram_partial_bytes(GRAM_TILE + 1)
    assert front > 0 and lib.upk_mbar_gram_partial_bytes(4096) == 0
    assert lib.upk_mbar_gram_rows(GRAM_TILE + 1, front + 2 * GRAM_TILE * 8 * (2 * GRAM_GRANULE + 5)) == 2 * GRAM_GRANULE
    assert lib.upk_mbar_gram_rows(GRAM_TILE + 1, front + 2 * GRAM_TILE * 8 * GRAM_GRANULE - 1) == 0
    assert lib.upk_mbar_gram_rows(8192, 512 << 20) == 8192 and lib.upk_mbar_gram_rows(8193, 512 << 20) == 0


def test_solver_argument_is_checked():
    with pytest.raises(ValueError):
        mbar.mbar(solver='steepest', tol=1e-8, **M.case_periodic())
