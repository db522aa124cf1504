"""GPU tests of MBAR on the device (upside_hip_mbar, csrc/kernels_mbar.hip; mbar.mbar, Ensemble.umbrella_mbar): every check runs in
a child process with its own time limit (tests/mbar_gpu_worker.py, which prints each figure before it asserts) against the float64
yardstick tests/mbar_reference.py, itself pinned by tests/test_mbar_config.py.  Bound: f and D within 1e-9 x max(1, |value|) of the
yardstick after the same number of iterations (both sides are fp64; a sum of N <= 1e4 terms carries about N eps ~ 1e-12 and the
iteration contracts: three orders of margin); log-weights within 1e-9 and normalised to 1e-12; two calls are compared bitwise."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mbar_gpu_worker.py')


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


def test_twenty_iterations_match_the_float64_yardstick(tmp_path):
    """from f = 0, tol = 0, max_iter = 20: f and D within the bound for N in {1, 255, 256, 257, 1000} x K in {1, 2, 3, 4, 5, 127, 128,
    129} (the state tile of the denominator pass is 128, the free-energy pass takes 4 states per workgroup) x d in {0 with energies,
    1, 2, 8}: a periodic CV with windows at +-3.0 and samples on both sides of the cut, flat bottoms holding none, some and all of
    the samples, unequal counts with at least two empty states, one state whose reduced energies pass 1e5; everything finite"""
    run_check('fixed', tmp_path, 300)


def test_converged_free_energies_are_a_fixed_point_of_the_yardstick(tmp_path):
    """the harmonic (K = 8, 500 samples each, kT = 0.8) and the periodic two-CV case (5 x 257 samples) with tol = 1e-10: last_delta
    below tol, and one yardstick iteration from the returned f moves it by less than 10 tol"""
    run_check('convergence', tmp_path, 300)


def test_temperature_ladder_and_target_weights(tmp_path):
    """d = 0, six beta, seeded energies: f and D within the bound; the log-weights of a target temperature within 1e-9 of the
    yardstick's and normalised to 1e-12; a target with a bias of its own (d = 2, one periodic CV)"""
    run_check('temperature', tmp_path, 300)


def test_umbrella_ladder_end_to_end(tmp_path):
    """trpcage20_7A, 8 systems at T = 0.8, a cv_restraint ladder of 8 windows on the end-to-end distance written by
    write_umbrella_windows, record_cvs(1) over 200 rounds with the node's CV as the SECOND recorded column: umbrella_mbar(tol = 0,
    max_iter = 20) equals the yardstick on read_cvs() within the bound; its rows are the configuration's, bit for bit"""
    run_check('end_to_end', tmp_path, 300)


def test_two_calls_return_the_same_bits(tmp_path):
    """f, D and the target's log-weights of two calls on one input are bit-identical (K = 129, d = 2; d = 8; d = 0)"""
    run_check('reproducible', tmp_path, 300)


def test_refusals_state_their_reason_and_leave_the_library_usable(tmp_path):
    """every limit of the entry point (d > 8, no state, no sample, N x K at 2^62, counts that are negative, all zero or do not add up,
    entries that are not finite, negative spring_const, flat_width or period, tol < 0, max_iter < 1) and a node CV that is not
    recorded: an error with its message; a good call afterwards returns the bits of the one before"""
    run_check('refusals', tmp_path, 300)
