"""GPU tests of the moving restraint on collective variables (node cv_steer: csrc/kernels_cv.hip k_cv_steer and k_cv_steer_advance):
every check runs in a child process with its own time limit (tests/cv_steer_gpu_worker.py, which prints each figure before it
asserts) against the float64 yardstick tests/cv_steer_reference.py, itself pinned by tests/test_cv_steer_config.py.  Everything runs
on trpcage20_7A (60 atoms) with 1 to 64 systems; the configuration files are written into the test's temporary directory.  Bounds: an
energy within 1e-6 relative; a derivative within parity_util.RTOL as relative RMS and 10 x RTOL of its scale in the largest element; a
centre within 1e-15 relative of config.steer_center; the accumulated work within 1e-12 x sum_n sum_c (|E_c(v_n, c(n))| + |E_c(v_n,
c(n-1))|) of config.steer_work of the recorded CV series (derived in the worker's docstring); equalities between engine runs are
bitwise."""
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cv_steer_gpu_worker.py')


def run_check(which, tmp_path, timeout, env=None):
    try:
        r = subprocess.run([sys.executable, WORKER, which, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout,
                           env=dict(os.environ, **(env or {})))
    except subprocess.TimeoutExpired as err:      # a hang: nothing more is started
        pytest.exit('check %s did not finish in %d s:\n%s' % (which, timeout, (err.stdout or b'').decode()[-3000:]), returncode=3)
    out = r.stdout.decode()
    print(out)
    if r.returncode not in (0, 1):      # killed by a signal or aborted: nothing more is started on a device that may have faulted
        pytest.exit('check %s ended with status %d:\n%s' % (which, r.returncode, out[-3000:]), returncode=3)
    assert r.returncode == 0, out[-6000:]
    assert 'CHECK %s PASSED' % which in out, out[-2000:]
    return out


def test_at_rest_it_is_a_cv_restraint(tmp_path):
    """rate = 0 on 11 CVs of every kind (those of cv_restraint_cases plus two dihedrals and the helix content): energy and derivative
    within the bounds of the yardstick and of a cv_restraint node with the same rows; steer_values equals cvs() bitwise; the clock does
    not matter; nodes of one CV (an rmsd, a dihedral) work too"""
    run_check('static', tmp_path, 300)


def test_the_centre_follows_each_systems_clock(tmp_path):
    """16 noisy systems, the 11 CVs pulled up and down over 20 rounds: at clocks 0, 1, 7, 19, 20 and 10^6 past the end the centres in
    force equal config.steer_center and energy and derivative are within the bounds at the yardstick's centres; every system its own
    clock; a dihedral whose centre has travelled from +3.0 to an unwrapped 3.5 with the value at -2.9 feels the nearest image"""
    run_check('moving', tmp_path, 300)


def test_rows_do_not_depend_on_the_batch(tmp_path):
    """identical positions, rows and clocks at systems 0, 7 and 63 of 64 (the others pull at their own speeds and clocks) give
    bit-identical energies, derivatives, centres and values; two runs are bit-identical"""
    run_check('batch', tmp_path, 300)


def test_work_is_a_function_of_the_recorded_series(tmp_path):
    """8 systems of trpcage20 with its full potential at T = 0.8, CVs (end-to-end distance, Rg, psi of residue 10), every system its
    own rates, 40 rounds from clock 0 with record_cvs(1): the work on the device equals config.steer_work of the recorded series
    within the bound; clocks are 40; work is non-zero and differs between systems; after set_steer_state(clock=0, work=0) and the same
    seed a second run gives bitwise the same work"""
    run_check('work', tmp_path, 300)


def test_pulling_holds(tmp_path):
    """8 systems: the end-to-end distance steered from its initial value by +8 A (four systems) and -4 A (four) with spring_const 20
    over 150 rounds plus 50 at the end, the rows set per system: every final value is nearer its own end than the other group's (12 A
    apart: a margin of 6 A); positions finite; centres equal center_end exactly"""
    run_check('pull', tmp_path, 300)


def test_captured_graph_replays_the_pulling(tmp_path):
    """12 rounds under UPSIDE_HIP_GRAPH=1 and =0 with a set_steer_state after six of them, which the next rounds see: two runs of one
    setting bit-identical; positions, momenta, work, clocks and centres bit-identical between the settings"""
    res = {}
    for g in ('1', '0'):
        run_check('graph', tmp_path, 300, env={'UPSIDE_HIP_GRAPH': g})
        res[g] = np.load(str(tmp_path / ('graph%s.npz' % g)))
    same = dict((k, bool(np.array_equal(res['1'][k], res['0'][k]))) for k in ('pos', 'mom', 'work', 'clock', 'center', 'series'))
    print('UPSIDE_HIP_GRAPH=1 against =0, bit-identical: %s' % same)
    assert all(same.values())


def test_upside_hip_writes_work_clock_and_centre_per_frame(tmp_path):
    """a file with the node and the same CVs in /input/collective_variables, one frame per round: /output/cv_steer/<node>/{work,
    clock, center} with one row per frame, the last work equal to config.steer_work of /output/cv within the bound; a file without
    the node has no /output/cv_steer"""
    run_check('cli', tmp_path, 600)


def test_bad_rows_and_states_are_refused_and_leave_the_earlier_ones_in_force(tmp_path):
    """every check_param refusal at construction, as a ladder's row and through set_param / set_param_system, the earlier row staying
    in force; a negative clock or work that is not finite; steer_* on a node that is no cv_steer; a ladder differing in a foreign
    dataset or in the CV definition names file, node and dataset; a ladder of two speeds is served; the process stays usable"""
    run_check('refusals', tmp_path, 300)
