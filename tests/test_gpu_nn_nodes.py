"""GPU tests of the learned backbone potential (backbone_featurizer, conv1d, scaled_sum): every check runs in a child
process with its own time limit (tests/nn_gpu_worker.py, which prints each figure before it asserts) against the float64
yardstick tests/nn_reference.py, itself pinned by tests/test_nn_config.py.  The network files are written into the test's
temporary directory.  Tolerances: parity_util.RTOL as relative RMS, 10 x RTOL for the largest element (parity_util.compare)."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'nn_gpu_worker.py')


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


def test_engine_constructs_with_a_network_appended(tmp_path):
    """proteinG56_7A and syn300_10A with 6 -> 32 (W 5, ReLU) -> 32 (W 5, Tanh) -> 1 (W 1, Identity), trpcage20_7A with one
    6 -> 1 (W 3, Identity) layer: the engine constructs and the total energy is the unmodified fixture's plus the network term"""
    run_check('construct', tmp_path, 600)


def test_forward_outputs_match_the_yardstick(tmp_path):
    """get_output of the featurizer, of every layer and the scaled_sum potential against nn_reference fed with the engine's own
    rama_coord and protein_hbond outputs"""
    run_check('forward', tmp_path, 600)


def test_sensitivities_match_the_yardstick(tmp_path):
    """get_sens of every layer and of the featurizer; rama_coord and column 6 of protein_hbond as the difference to an engine
    built from the unmodified fixture at the same positions, relative to the scale of the larger operand"""
    run_check('backward', tmp_path, 600)


def test_potential_deriv_agreement_with_a_smooth_network(tmp_path):
    """upside_hip --potential-deriv-agreement on proteinG56_7A with a Tanh / Tanh / Identity network reports an overall
    relative error of at most 2 x the figure of the unmodified fixture in the same run (the noise of an fp32 difference quotient;
    a missing or mis-signed term gives 0.1 to 1)"""
    run_check('agreement', tmp_path, 1500)


def test_weight_gradients_and_set_param(tmp_path):
    """get_param_deriv of every conv1d and of scaled_sum; get_param in the stated order; the forward pass after set_param; a
    vector of the wrong length raises; an Ensemble that has run MD steps uses the new weights in the steps that follow"""
    run_check('weights', tmp_path, 900)


@pytest.mark.parametrize('which', ['batch64', 'batch600'])
def test_batch_is_deterministic_and_independent_of_position(tmp_path, which):
    """64 and 600 systems (the second crosses the 512-system paths) at distinct positions, systems 0, 7 and the last alike:
    those three bit-identical; every system against a one-system engine to RTOL; accumulate + read against the float64
    weighted sum; two runs bit-identical"""
    run_check(which, tmp_path, 1500)


def test_md_with_the_network_is_reproducible(tmp_path):
    """init_md + 200 steps on 8 systems: finite, bit-identical across two runs, and (where the unmodified fixture has that
    property) between run_steps(200) and 200 x run_steps(1)"""
    out = run_check('md', tmp_path, 900)
    assert 'bit-identical across two runs' in out


def test_size_edges(tmp_path):
    """W = 15 with 64 -> 64 channels on syn300_10A (the weights do not fit LDS: sliced tiles), W = chain length (one output row),
    and a layer beyond the stated limits, which is either right or refused with the documented message"""
    run_check('edges', tmp_path, 900)


def test_bad_configurations_are_refused_on_the_host(tmp_path):
    """wrong activation name, two activations, C_in mismatch, wrong bias length, W > rows, scaled_sum on width 2, out-of-range
    rama_idx / hbond_idx: construction fails with the message and the process stays usable; a two-file ladder that differs
    only in `weights` is refused with a message naming the file, the node and the dataset"""
    run_check('errors', tmp_path, 600)
