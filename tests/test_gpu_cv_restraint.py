"""GPU tests of the cv_restraint node (an umbrella bias on the device collective variables): every check runs in a child process
with its own time limit (tests/cv_restraint_gpu_worker.py, which prints each figure before it asserts) against the float64
yardstick tests/cv_restraint_reference.py, itself pinned by tests/test_cv_restraint_config.py.  The configuration files are
written into the test's temporary directory.  Tolerances: 1e-6 relative for energies, parity_util.RTOL as relative RMS and
10 x RTOL for the largest element of a derivative; equalities between engine runs are bitwise."""
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cv_restraint_gpu_worker.py')


def run_check(which, tmp_path, timeout, env=None):
    try:
        r = subprocess.run([sys.executable, WORKER, which, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout,
                           env=None if env is None else dict(os.environ, **env))
    except subprocess.TimeoutExpired as err:      # a hang: nothing more is started
        pytest.exit('check %s did not finish in %d s:\n%s' % (which, timeout, (err.stdout or b'').decode()[-3000:]), returncode=3)
    out = r.stdout.decode()
    print(out)
    if r.returncode not in (0, 1):      # killed by a signal or aborted: nothing more is started on a device that may have faulted
        pytest.exit('check %s ended with status %d:\n%s' % (which, r.returncode, out[-3000:]), returncode=3)
    assert r.returncode == 0, out[-6000:]
    assert 'CHECK %s PASSED' % which in out, out[-2000:]
    return out


def test_forces_and_energies_match_the_yardstick(tmp_path):
    """trpcage20 (60 atoms) and syn300 (900 atoms), the node alone: Rg over all atoms and over the first 255 / 256 / 257, two rmsd CVs
    with different selections and one over exactly 3 atoms, contacts with 1 pair and with the CA native list, two distances sharing
    an atom; every k > 0, some CVs inside their flat bottom; all together and each alone; coincident atoms give zero force"""
    run_check('forces', tmp_path, 300)


def test_values_are_the_bits_of_the_cv_kernel(tmp_path):
    """restraint_values after energies() against cvs() of the same definition, 1 and 64 systems"""
    run_check('same_bits', tmp_path, 300)


def test_ladder_equals_separate_engines(tmp_path):
    """8 windows of proteinG56_7A with its full potential plus an rmsd and a Q restraint: from_files against 8 copies of window i
    (bitwise), against an engine of window i alone (1e-6), and set_param_system on copies of window 0 (bitwise)"""
    run_check('ladder', tmp_path, 600)


def test_batch_is_deterministic_and_independent_of_position(tmp_path):
    """64 and 600 systems at distinct positions and windows; systems 0, 7 and the last equal: bit-identical; two runs bit-identical;
    every system matches a one-system engine"""
    run_check('batch', tmp_path, 600)


def test_md_separates_low_and_high_windows(tmp_path):
    """trpcage20 with its full potential, 8 systems at T = 0.8, Rg over the CA atoms with k = 50 and centres 0.7 / 1.5 x Rg0: finite,
    two runs bit-identical, every low window's mean Rg over the last 100 of 200 rounds below every high window's; captured-graph
    replay and plain launches agree bit for bit where they do for the unmodified fixture"""
    res = {}
    for g in ('1', '0'):
        run_check('md', tmp_path, 600, env={'UPSIDE_HIP_GRAPH': g})
        res[g] = np.load(str(tmp_path / ('md_graph%s.npz' % g)))
    free_same = all(np.array_equal(res['1'][k], res['0'][k]) for k in ('free_pos', 'free_mom'))
    same = all(np.array_equal(res['1'][k], res['0'][k]) for k in ('pos', 'mom', 'series'))
    print('UPSIDE_HIP_GRAPH=1 against =0: the unmodified fixture bit-identical: %s; with the restraint: %s' % (free_same, same))
    if free_same:
        assert same


def test_values_rewritten_in_place_reach_a_captured_graph(tmp_path):
    """after run_rounds, set_param_system moves one window's centre: the next energies() equals a fresh engine built with that centre
    at the same positions, and the following rounds move that system (and no other) off the trajectory of an unmoved engine"""
    run_check('inplace', tmp_path, 600)


def test_device_swap_set_matches_the_host_procedure(tmp_path):
    """a 16-window Q ladder with a temperature ladder on top: hamiltonian_swap against upside_hip_swap_between +
    upside_replica_decide_lboltz, one round of both swap sets"""
    run_check('swap', tmp_path, 600)


def test_upside_hip_runs_window_files(tmp_path):
    """upside_hip on 4 window files with --replica-interval and two --swap-set: every file gets /output with replica_index, frame 0
    of potential equals Ensemble.from_files(...).energies() at the initial structure (1e-6)"""
    run_check('cli', tmp_path, 600)


def test_refusals_leave_the_process_usable(tmp_path):
    """every refusal of the node's construction, by its message; after each the process constructs a good engine; a ladder whose
    files differ in `atoms` is refused naming file, node and dataset"""
    run_check('refusals', tmp_path, 600)
