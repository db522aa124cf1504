"""GPU tests of the MBAR bootstrap (upside_hip_mbar_bootstrap, csrc/kernels_mbar_boot.hip; mbar.bootstrap, bootstrap_sigma,
profile_bootstrap, Ensemble.umbrella_mbar(n_bootstrap=...)): every check runs in a child process with its own time limit
(tests/mbar_bootstrap_gpu_worker.py, which prints each figure before it asserts) against the float64 yardstick
tests/mbar_bootstrap_reference.py, itself pinned by tests/test_mbar_bootstrap_config.py.  Bound: f_boot and columns within
1e-9 x max(1, |value|) of the yardstick after the same number of iterations -- the bound and the reasoning of tests/test_gpu_mbar.py
(both sides are fp64; a sum of N <= 1e5 terms carries about N eps ~ 1e-11 and the iteration contracts); "the same bits" is bitwise
equality."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mbar_bootstrap_gpu_worker.py')


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
def test_twenty_iterations_of_five_replicates_match_the_float64_yardstick(tmp_path, d):
    """tol = 0, max_iter = 20, f0 = 0 on mbar_cases.stressed_case for N in {1, 255, 256, 257, 1000} x K in {1, 2, 3, 4, 5, 127, 128,
    129}, samples grouped by state, 5 replicates: all ones, three seeded draws, one with each state's whole count on a single sample.
    f_boot within the bound of the yardstick; the all-ones replicate within the bound of mbar.mbar on the same input"""
    run_check('fixed_d%d' % d, tmp_path, 300)


def test_counts_equal_repeated_samples_on_the_device(tmp_path):
    """independent of the yardstick: a replicate with counts c equals the device's own mbar.mbar on the samples repeated c times,
    20 iterations, within the bound (d = 0, 1, 2, 8; the degenerate replicate among them)"""
    run_check('duplication', tmp_path, 300)


def test_a_hundred_replicates_converge_and_leave_the_grid_one_by_one(tmp_path):
    """case_harmonic and case_periodic, 100 replicates from bootstrap_counts(seed=5), tol = 1e-10 from the converged f: every
    last_delta below tol, one yardstick iteration from each returned f_b moves it by less than 10 tol, the iteration counts are not
    all equal, and bootstrap_sigma over the asymptotic sigma lies within [0.65, 1.5]"""
    run_check('convergence', tmp_path, 300)


def test_a_replicates_bits_do_not_depend_on_the_batch(tmp_path):
    """case_periodic with profile columns: f_boot, columns, n_iter and last_delta of a replicate are bit-identical alone, in the batch
    of 100, in a batch solved one replicate at a time (the smallest workspace), for B in {1, 2, chunk - 1, chunk, chunk + 1} at a
    workspace that holds chunk = 7, among other replicates in another order, and in two calls on one input"""
    run_check('independence', tmp_path, 300)


def test_columns_and_the_bootstrap_profile(tmp_path):
    """profile bins as columns against the yardstick within the bound; a column that is -inf everywhere is +inf; a bin whose samples
    all have count 0 in one replicate is +inf in that replicate only; profile_bootstrap returns the F of profile() and the standard
    deviation the yardstick gives on the same counts"""
    run_check('columns', tmp_path, 300)


def test_counts_up_to_65535(tmp_path):
    """K = 2 with n_k = [66000, 10]: a replicate with 65535 on one sample of state 0 and 465 on another, within the bound"""
    run_check('count_range', tmp_path, 300)


def test_umbrella_ladder_with_bootstrap_end_to_end(tmp_path):
    """trpcage20_7A, 8 windows, 200 rounds: umbrella_mbar(n_bootstrap=16) with and without decorrelate -- every window keeps its
    count in every replicate under the layout of values, f_boot equals mbar.bootstrap on the returned values with the returned
    counts bit for bit, sigma_boot is finite and symmetric with zero diagonal; n_bootstrap=0 returns exactly the keys of a call
    without it; tools/umbrella_mbar.py --bootstrap 16 --seed 4 on the same series written to the window files prints the same
    bootstrap sigma (to its six decimals) and a bootstrap dF column of the profile"""
    run_check('end_to_end', tmp_path, 300)


def test_refusals_state_their_reason_and_leave_the_library_usable(tmp_path):
    """every refusal of the entry point with its message; a good call afterwards returns the bits of the one before"""
    run_check('refusals', tmp_path, 300)
