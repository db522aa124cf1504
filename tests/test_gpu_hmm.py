"""GPU tests of the TorusDBN backbone prior (torus_dbn, fixed_hmm): every check runs in a child process with its own time limit
(tests/hmm_gpu_worker.py, which prints each figure before it asserts) against the float64 yardstick tests/hmm_reference.py,
itself pinned by tests/test_hmm_config.py.  The configurations are written into the test's temporary directory; the parameters
come from a seeded generator.  Tolerances: parity_util.RTOL as relative RMS, 10 x RTOL for the largest element
(parity_util.compare)."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hmm_gpu_worker.py')


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


def test_engine_constructs_with_the_prior_appended(tmp_path):
    """trpcage20_7A and proteinG56_7A with a 55-state prior: the engine constructs and the total energy is the unmodified
    fixture's plus -log Z"""
    run_check('construct', tmp_path, 600)


def test_forward_outputs_match_the_yardstick(tmp_path):
    """get_output('torus_dbn') and the potential of fixed_hmm at n_state = 1, 3, 5, 55, 64, 65 and 128 over the whole interior of
    the chain, and with an id of length 1 (one residue: no transition)"""
    run_check('forward', tmp_path, 600)


def test_sensitivities_match_the_yardstick(tmp_path):
    """get_sens('torus_dbn') equals the posterior marginals; rama_coord's sens as the difference to an engine built from the
    unmodified fixture at the same positions; a reversed chain gives the yardstick's gradient at index[r]"""
    run_check('backward', tmp_path, 600)


def test_wide_energy_ranges_stay_finite_and_exact(tmp_path):
    """transition energies spanning 0..60 and emission energies spanning more than 50 within every residue: finite, and within
    the same tolerance"""
    run_check('energy_range', tmp_path, 600)


def test_potential_deriv_agreement_with_the_prior(tmp_path):
    """upside_hip --potential-deriv-agreement on proteinG56_7A with the prior appended reports an overall relative error of at
    most 2 x the figure of the unmodified fixture in the same run"""
    run_check('agreement', tmp_path, 1500)


def test_parameters_derivatives_and_set_param(tmp_path):
    """both get_param orders; both get_param_deriv against the yardstick; the forward pass after set_param of each node; a vector of
    the wrong length raises; an Ensemble that has run MD steps uses the new transition_energy in the steps that follow"""
    run_check('parameters', tmp_path, 900)


@pytest.mark.parametrize('which', ['batch64', 'batch600'])
def test_batch_is_deterministic_and_independent_of_position(tmp_path, which):
    """64 and 600 systems at distinct positions, systems 0, 7 and the last alike: those three bit-identical; every system against
    a one-system engine to RTOL; accumulate + read against the float64 weighted sum; two runs bit-identical"""
    run_check(which, tmp_path, 1500)


def test_md_with_the_prior_is_reproducible(tmp_path):
    """init_md + 200 steps on 8 systems: finite and bit-identical across two runs"""
    out = run_check('md', tmp_path, 900)
    assert 'bit-identical across two runs' in out


def test_bad_configurations_are_refused_on_the_host(tmp_path):
    """non-square transition_energy, a width mismatch with the argument, an empty index, out-of-range or repeated id / index, a
    restypes entry >= n_restype, n_state above the limit: construction fails with the message and the process stays usable; a
    two-file ladder that differs only in transition_energy is refused with a message naming the file, the node and the dataset"""
    run_check('errors', tmp_path, 600)
