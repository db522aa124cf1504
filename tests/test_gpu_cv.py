"""GPU tests of the collective variables (csrc/kernels_cv.hip behind upside_hip_cv_*): every check runs in a child process with
its own time limit (tests/cv_gpu_worker.py, which prints each figure before it asserts) against the float64 yardstick
tests/cv_reference.py, itself pinned by tests/test_cv_config.py.  All checks run on proteinG56_7A, syn300_10A and trpcage20_7A
(the refusals on trpcage20_7A).  Bound on every value, RMSD included: |gpu - float64| <= parity_util.RTOL x max(|value|, scale),
scale = the Rg of the reference structure for lengths and 1 for Q.  Nothing here puts a bound on the cost of recording."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cv_gpu_worker.py')


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


def test_values_match_the_float64_yardstick(tmp_path):
    """64 systems: the fixture plus seeded Gaussian noise growing from 0 to 3 Angstrom, one exact rigid motion of the reference, one
    with a contact pair stretched to 900 Angstrom; seven CVs of the four kinds; every value within the bound above, the RMSD of the
    rigid motion and of the reference itself below RTOL x Rg, Q finite and the stretched pair's own Q exactly 0"""
    run_check('values', tmp_path, 600)


def test_rows_do_not_depend_on_the_batch(tmp_path):
    """identical positions at systems 0, 7 and the last of 64 and of 600 systems give bit-identical rows, the same for both batch
    sizes; two runs are bit-identical"""
    run_check('batch', tmp_path, 900)


@pytest.mark.parametrize('graph', ['0', '1'])
def test_recording_inside_the_md_loop(tmp_path, graph):
    """8 systems, init_md, record_cvs(every=5, capacity=64), run_rounds(200): 40 samples, bit-identical to a second engine that
    alternates run_rounds(5) and cvs(); final positions and momenta bit-identical to a third engine that never defined a CV; capacity
    10 stores 10 of 40 attempted.  With the captured MD graph forced off (UPSIDE_HIP_GRAPH=0) and on (=1)"""
    out = run_check('record', tmp_path, 1200, env={'UPSIDE_HIP_GRAPH': graph, 'UPSIDE_HIP_GRAPH_DEBUG': '1'})
    assert 'UPSIDE_HIP_GRAPH=%s' % graph in out
    assert ('graph: captured 6 MD steps' in out) == (graph == '1'), 'the MD graph was%s captured' % (' not' if graph == '1' else '')


def test_samples_follow_the_slot_under_exchange(tmp_path):
    """after swap_systems(1, 2) the next sample of slots 1 and 2 equals cvs() of the traded coordinates"""
    run_check('slots', tmp_path, 600)


def test_upside_hip_writes_output_cv(tmp_path):
    """upside_hip on a file with /input/collective_variables: /output/cv (frame, 1, n_cv) f32 with the frame count of /output/pos,
    every row equal to the yardstick on that frame's stored pos within the bound, the names as attributes; two such files in one
    run alike; the same file without the group has no /output/cv"""
    run_check('cli', tmp_path, 900)


def test_bad_definitions_are_refused_and_leave_the_previous_one_in_force(tmp_path):
    """unknown kind, atom out of range, empty selection, rmsd under 3 atoms, odd contacts list, r0 <= 0, a distance of 3 atoms, more
    CVs or list entries than the stated limits: an error with the message, and cvs() still returns the earlier definition's values"""
    run_check('refusals', tmp_path, 600)
