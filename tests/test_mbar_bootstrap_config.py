"""CPU tests of the MBAR bootstrap: the float64 yardstick tests/mbar_bootstrap_reference.py pinned on identities that need no device,
mbar.bootstrap_counts and bootstrap_sigma (pure numpy), and every refusal of upside_hip_mbar_bootstrap through the built library --
they return before any device call and so need no GPU."""
import os
import warnings
import numpy as np
import pytest
import parity_util as P
import mbar_reference as M
import mbar_uncertainty_reference as U
import mbar_bootstrap_reference as R
import mbar_bootstrap_cases as C
from mbar_cases import small_case, stressed_case

pkg = P.pkg


def energies(case):
    v = case['values'] if case['values'] is not None else np.zeros((len(case['energy']), 0), 'f4')
    return M.reduced_energy(v, case['energy'], case['beta'], case['rows'], case['periods'])


def test_unit_counts_return_the_bits_of_the_plain_iteration():
    for case in (small_case(K=4, n=40, d=2), stressed_case(257, 5, 2, 77), stressed_case(255, 4, 0, 3)):
        u = energies(case)
        f = np.zeros(u.shape[1])
        ones = np.ones(len(u), 'u2')
        for _ in range(5):
            a, Da = R.iterate(u, case['n_k'], f, ones)
            b, Db = M.iterate(u, case['n_k'], f)
            assert a.tobytes() == b.tobytes() and Da.tobytes() == Db.tobytes()
            f = a
        r = R.solve(u, case['n_k'], ones[None, :], 0., 7)
        assert r['f_boot'][0].tobytes() == M.mbar(case['values'] if case['values'] is not None else np.zeros((len(u), 0), 'f4'), case['energy'],
                                                  case['beta'], case['rows'], case['n_k'], case['periods'], 0., 7)['f'].tobytes()
        assert r['n_iter'][0] == 7


def test_counts_equal_physically_repeated_samples():
    """one iteration with counts c against mbar_reference.iterate on the samples repeated c times, to 1e-13 (a prototype measured
    1e-14): the sums differ only in c equal terms being added one by one instead of once with weight c"""
    worst = 0.
    for case, seed in ((small_case(K=4, n=40, d=2), 1), (stressed_case(257, 5, 1, 9), 2), (M.case_periodic(), 3)):
        u = energies(case)
        n_k = np.asarray(case['n_k'], 'i8')
        counts = C.fixed_counts(n_k, seed)
        f = M.mbar(tol=0., max_iter=3, **case)['f']
        for c in counts:
            got, _ = R.iterate(u, n_k, f, c)
            want, _ = M.iterate(np.repeat(u, c.astype('i8'), axis=0), n_k, f)
            err = float((np.abs(got - want) / np.maximum(1., np.abs(want))).max())
            worst = max(worst, err)
    print('largest |weighted - repeated| / max(1, |f|) = %.3e (bound 1e-13)' % worst)
    assert worst <= 1e-13


def test_columns_of_the_yardstick():
    case = small_case(K=3, n=20, d=1)
    u = energies(case)
    n_k = case['n_k']
    f = M.mbar(tol=0., max_iter=10, **case)['f']
    c = C.fixed_counts(n_k, 4)[2]
    ln = np.full((3, 60), -np.inf)
    ln[0] = -u[:, 1]                     # state 1 as a column: its free energy from the counted samples, before f_0 is taken off
    ln[1, c == 0] = 0.                   # only samples the replicate does not hold
    got = R.columns(u, n_k, f, c, ln)
    D = M.denominators(u, n_k, f)
    keep = c > 0
    want0 = -M.logsumexp(np.log(c[keep].astype('f8')) - u[keep, 1] - D[keep], 0)
    assert abs(got[0] - want0) < 1e-13 and got[1] == np.inf and got[2] == np.inf
    fn, _ = R.iterate(u, n_k, f, c)
    first = -M.logsumexp(np.log(c[keep].astype('f8')) - u[keep, 0] - D[keep], 0)
    assert abs((got[0] - first) - fn[1]) < 1e-13


def test_bootstrap_counts_keep_every_states_count_in_both_layouts():
    bc = pkg.mbar.bootstrap_counts
    n_k = np.array([7, 0, 12, 5], 'i8')
    grouped = bc(n_k, 9, seed=3)
    assert grouped.dtype == np.uint16 and grouped.shape == (9, 24)
    sos = C.grouped_origins(n_k)
    for k in range(4):
        assert (grouped[:, sos == k].sum(axis=1) == n_k[k]).all()
    assert grouped.tobytes() == bc(n_k, 9, seed=3).tobytes() and grouped.tobytes() != bc(n_k, 9, seed=4).tobytes()
    assert grouped.tobytes() == bc(n_k, 9, seed=3, state_of_sample=sos).tobytes()
    # the definition: one generator, the states in ascending order, a multinomial over the state's samples
    rng = np.random.default_rng(3)
    want = np.concatenate([rng.multinomial(m, np.full(m, 1. / m), size=9) for m in n_k if m], axis=1)
    assert np.array_equal(grouped, want)
    # interleaved (i, s): sample i * K + s belongs to state s
    eq = np.array([6, 6, 6], 'i8')
    inter = np.tile(np.arange(3), 6)
    got = bc(eq, 5, seed=8, state_of_sample=inter)
    for k in range(3):
        assert (got[:, inter == k].sum(axis=1) == 6).all()
        assert np.array_equal(got[:, inter == k], bc(eq, 5, seed=8)[:, 6 * k:6 * k + 6])      # the same draw, laid out by origin
    with pytest.raises(ValueError):
        bc(eq, 5, state_of_sample=np.tile(np.arange(3), 5))
    with pytest.raises(ValueError):
        bc(eq, 0)
    with pytest.raises(ValueError):
        bc(np.array([70000]), 1, state_of_sample=np.zeros(70000, 'i4') + 1)
    big = bc(np.array([200000], 'i8'), 2, seed=1)
    assert big.sum(axis=1).tolist() == [200000, 200000]


def test_a_count_above_65535_is_refused(monkeypatch):
    class Rng:
        def multinomial(self, n, p, size):
            out = np.zeros((size, len(p)), 'i8'); out[:, 0] = n
            return out
    monkeypatch.setattr(np.random, 'default_rng', lambda seed: Rng())
    assert pkg.mbar.bootstrap_counts(np.array([65535]), 2).max() == 65535
    with pytest.raises(ValueError) as err:
        pkg.mbar.bootstrap_counts(np.array([3, 65536]), 2)
    assert '65535' in str(err.value) and 'state 1' in str(err.value)


def test_bootstrap_sigma_leaves_unconverged_replicates_out_and_says_so():
    rng = np.random.RandomState(2)
    fb = rng.normal(size=(12, 4)); fb[:, 0] = 0.
    s = pkg.mbar.bootstrap_sigma(fb)
    assert s.shape == (4, 4) and (np.diag(s) == 0).all() and np.array_equal(s, s.T)
    assert np.allclose(s, R.pair_sigma(fb), rtol=0, atol=1e-14)
    ok = np.ones(12, bool); ok[[3, 7]] = False
    with pytest.warns(RuntimeWarning, match='2 of 12'):
        part = pkg.mbar.bootstrap_sigma(dict(f_boot=fb, converged=ok))
    assert np.allclose(part, R.pair_sigma(fb[ok]), rtol=0, atol=1e-14)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        pkg.mbar.bootstrap_sigma(fb, np.ones(12, bool))
    assert np.isnan(pkg.mbar.bootstrap_sigma(fb[:1])).all()


def test_the_yardsticks_bootstrap_sigma_is_close_to_the_asymptotic_one():
    """case_periodic, 100 replicates from default_rng(5), tol 1e-10 from the converged f: every replicate converges, and over all
    pairs the bootstrap sigma lies within [0.65, 1.5] of the asymptotic one (eq. D8 on the yardstick's weights) -- 0.96 .. 1.24 was
    measured here (0.88 .. 1.17 on case_harmonic), widened by 3 / sqrt(2 x 100), the noise of a standard deviation from 100 draws.  A
    plausibility fence on the yardstick, not a measurement of the device."""
    case = M.case_periodic()
    u = energies(case)
    n_k = case['n_k']
    f = C.converged_start(case)
    counts = pkg.mbar.bootstrap_counts(n_k, C.N_BOOT, seed=C.BOOT_SEED)
    r = R.solve(u, n_k, counts, C.TOL, 5000, f0=f)
    assert (r['last_delta'] < C.TOL).all() and r['n_iter'].max() < 5000
    W, _ = U.weights(u, n_k, f)
    asym = np.sqrt(np.maximum(U.pair_variance(U.theta_d8(W, n_k)), 0.))
    boot = R.pair_sigma(r['f_boot'])
    off = ~np.eye(len(n_k), dtype=bool)
    ratio = boot[off] / asym[off]
    print('iterations %d .. %d; bootstrap / asymptotic sigma %.3f .. %.3f (fence %s)' % (r['n_iter'].min(), r['n_iter'].max(), ratio.min(), ratio.max(), C.SIGMA_RATIO))
    assert C.SIGMA_RATIO[0] <= ratio.min() and ratio.max() <= C.SIGMA_RATIO[1]
    assert len(set(r['n_iter'].tolist())) > 1


def test_the_entry_point_states_its_refusals():
    if not os.path.exists(pkg.PRODUCT_LIB):
        pytest.fail('libupside_hip.so not built (run __graft_entry__.build())')
    good, cases = C.boot_refusal_cases()
    for label, change, fragment in cases:
        kw = dict(good); kw.update(change)
        with pytest.raises(RuntimeError) as err:
            pkg.mbar.bootstrap(**kw)
        assert fragment in str(err.value), (label, str(err.value))
        assert 'mbar_bootstrap: ' in str(err.value), (label, str(err.value))
    calc = pkg.default_library().calc
    for label, override, fragment in C.RAW_REFUSALS:
        rc, msg = C.raw_call(calc, good, **override)
        assert rc == 1 and fragment in msg, (label, msg)
    # what Python refuses before the library is asked
    for change in (dict(counts=np.ones((2, 29), 'u2')), dict(counts=np.full((1, 30), 70000)), dict(counts=np.ones((1, 30)) * 1.5),
                   dict(f=np.zeros(2)), dict(log_numerators=np.zeros((2, 31))), dict(state_of_sample=np.zeros(7, 'i4'))):
        with pytest.raises(ValueError):
            pkg.mbar.bootstrap(**dict(good, **change))


def test_the_chunk_is_what_the_workspace_holds():
    if not os.path.exists(pkg.PRODUCT_LIB):
        pytest.fail('libupside_hip.so not built (run __graft_entry__.build())')
    chunk = pkg.mbar.boot_chunk
    assert chunk(1000, 8000) == 1 and chunk(1000, 7999) == 0 and chunk(1000, 16000) == 2 and chunk(1000, 23999) == 2
    assert chunk(1 << 26, 512 << 20) == 1 and chunk((1 << 26) + 1, 512 << 20) == 0
    assert chunk(1, 512 << 20) == 32768 and chunk(0, 1 << 20) == 0
