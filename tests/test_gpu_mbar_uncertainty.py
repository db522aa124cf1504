"""GPU tests of the MBAR Gram pass and what is built on it (upside_hip_mbar_gram, csrc/kernels_mbar_gram.hip; mbar.gram,
free_energy_uncertainty, expectation, profile, mbar(solver='newton'), Ensemble.umbrella_mbar(uncertainty=True)): every check runs in
a child process with its own time limit (tests/mbar_uncertainty_gpu_worker.py, which prints each figure before it asserts) against
the float64 yardstick tests/mbar_uncertainty_reference.py, itself pinned by tests/test_mbar_uncertainty_config.py.  Bounds:
|dG_kl| <= 1e-9 sqrt(G_kk G_ll) and colsum within 1e-9 relative (both sides fp64: a sum of at most 1e4 positive terms carries about
1e-12 and the exponent, where reduced energies of 3e5 cancel, about 1e-10); variances within 1e-6 relative (a relative perturbation
eps of G moves them by about 14 eps); two calls are compared bitwise."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mbar_uncertainty_gpu_worker.py')


def run_check(which, tmp_path, timeout):
    try:
        r = subprocess.run([sys.executable, WORKER, which, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    except subprocess.TimeoutExpired as err:      # a hang: nothing more is started
        pytest.exit('check %s did not finish in %d s:\n%s' % (which, timeout, (err.stdout or b'').decode()[-3000:]), returncode=3)
    out = r.stdout.decode()
    print(out)
    if r.returncode not in (0, 1):      # killed by a signal or aborted: nothing more is started on a device that may have faulted
        pytest.exit('check %s ended with status %d:\n%s' % (which, r.returncode, out[-3000:]), returncode=3)
    assert r.returncode == 0, out[-6000:]
    assert 'CHECK %s PASSED' % which in out, out[-2000:]
    return out


@pytest.mark.parametrize('d', [0, 1, 2, 8])
def test_gram_matrix_and_column_sums_match_the_float64_yardstick(tmp_path, d):
    """f after 20 yardstick iterations; N in {1, 255, 256, 257, 1000} x M in {1, 2, 63, 64, 65, 129} (the tile is 64) x n_extra in
    {0, 1, 3} (one explicit column with -inf entries) for d = 0 with energies, 1, 2 and 8: a periodic CV across the cut, flat
    bottoms, at least two empty states, one state with reduced energies above 1e5 (up to 3e5; asserted for d > 0 -- the temperature
    ladder d = 0 has no stiff state).  G within 1e-9 sqrt(G_kk G_ll), colsum within
    1e-9 relative, D within 1e-9 max(1, |D|); G bitwise symmetric; everything finite; the colsum-only pass returns the same bits"""
    run_check('gram_d%d' % d, tmp_path, 300)


def test_gram_launcher_over_slab_boundaries_and_a_converged_f(tmp_path):
    """upk_mbar_gram with a workspace of exactly one granule of rows R (M = 129, d = 2, 3 explicit columns): N in {R - 1, R, R + 1,
    3 R + 1} within the bounds, one byte less is refused with 9405; for f converged to 1e-10 on the harmonic and the periodic case
    colsum of every sampled state is 1 within 1e-9"""
    run_check('gram_slabs', tmp_path, 300)


def test_gram_on_both_sides_of_the_switch_between_partial_sums_and_direct_accumulation(tmp_path):
    """upk_mbar_gram with one granule of rows, N = 100 (four slabs), d = 2, 3 explicit columns: M = 1984 (a slab cut into 2 ranges with
    partial matrices) and M = 1985, 2049 (the tiles accumulate in G itself, stride M no multiple of 64, G read back on every later
    slab): G, colsum and D within the bounds of the shape check, and two calls bit-identical"""
    run_check('gram_switch', tmp_path, 300)


def test_two_gram_calls_return_the_same_bits(tmp_path):
    """G, colsum and D of two calls on one input are bit-identical (M = 129 with d = 2; d = 0)"""
    run_check('reproducible', tmp_path, 300)


def test_uncertainties_match_the_n_by_n_formula(tmp_path):
    """free_energy_uncertainty, expectation (two observables) and profile (with an empty bin; a periodic CV) on the harmonic and the
    periodic case: every variance within 1e-6 relative of eq. D8 on the yardstick's weight matrix, means and F within 1e-9"""
    run_check('uncertainty', tmp_path, 300)


def test_newton_solver_converges_in_a_few_steps(tmp_path):
    """solver='newton', tol = 1e-10, n_sc = 3 on the harmonic case, the periodic case and the harmonic case with windows 2 and 5 empty:
    last_delta < tol, one yardstick iteration moves f by less than 10 tol, at most 10 Newton steps and 20 iterations, f within 1e-9 of
    the yardstick converged to 1e-13; solver='self-consistent' returns the bits of a call without the argument"""
    run_check('newton', tmp_path, 300)


def test_umbrella_ladder_with_uncertainties_end_to_end(tmp_path):
    """trpcage20_7A, 8 windows on the end-to-end distance, 200 recorded rounds: umbrella_mbar(uncertainty=True, solver='newton') gives
    f within 1e-9 and sigma^2 within 1e-6 relative of the yardstick on read_cvs(); tools/umbrella_mbar.py --solver newton --uncertainty on
    the same series written to the window files prints the same f and sigma and a profile with its dF column"""
    run_check('end_to_end', tmp_path, 300)


def test_gram_refusals_state_their_reason_and_leave_the_library_usable(tmp_path):
    """f not finite, a log-column entry NaN or +inf, more than 8192 columns, n_extra < 0, colsum NULL and refusals shared with
    upside_hip_mbar: an error with its message; a good call afterwards returns the bits of the one before"""
    run_check('refusals', tmp_path, 300)
