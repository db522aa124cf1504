"""GPU tests of the path collective variables (kinds path_s and path_z of csrc/cv_path_device.h) and of the biases built on them:
every check runs in a child process with its own time limit (tests/cv_path_gpu_worker.py, which prints each figure before it
asserts) against the float64 yardstick tests/cv_path_reference.py, itself pinned by tests/test_cv_path_config.py.  The paths are
config.interpolate_path from a fixture to the fixture plus seeded smooth noise (tests/cv_path_cases.py) on trpcage20_7A (60 atoms)
and, for lane boundaries, proteinG56_7A (168 atoms); the configuration files are written into the test's temporary directory.
Bounds: path_s within parity_util.RTOL x max(|s|, 1); path_z within RTOL x max(|z|, Rg^2); a bias energy within 1e-6 relative; a
derivative within RTOL as relative RMS and 10 x RTOL of its scale in the largest element; equalities between engine runs are bitwise."""
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cv_path_gpu_worker.py')


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
    """16 systems per fixture, smooth noise growing from 0 to 3 Angstrom; K in {2, 3, 4, 5, 63, 64} frames, n in {3, 20, 60} atoms of
    trpcage and {63, 64, 65, 128, 129, 168} of protein G, lambda from path_lambda and 100 times that (one frame dominates, the far
    weights underflow): every s and z within the bound, s in [1, K]"""
    run_check('values', tmp_path, 300)


def test_rows_do_not_depend_on_the_batch(tmp_path):
    """identical positions at systems 0, 7 and the last of 64 systems give bit-identical values, energies and forces; two runs are
    bit-identical; a batch of 3 holds the bits of the batch of 64"""
    run_check('batch', tmp_path, 300)


def test_restraint_matches_the_yardstick(tmp_path):
    """the cv_restraint node alone on path_s, path_z (with a flat bottom) and an rg together and on each alone, for K and n on both
    sides of the wavefront boundaries: energies and forces; restraint_values equals cvs() bitwise; a dominating frame (100 x lambda,
    most coefficients exactly 0); a structure sitting exactly on a frame gives finite energy and finite forces"""
    run_check('restraint', tmp_path, 300)


def test_steering_along_s_matches_the_yardstick(tmp_path):
    """the cv_steer node on path_s: energy and forces at clocks 0 and 7 on 4 systems; after 7 rounds of MD with the full potential
    the accumulated work is the yardstick's restatement from the recorded series"""
    run_check('steer', tmp_path, 300)


def test_metadynamics_in_s_and_z_matches_the_yardstick(tmp_path):
    """the cv_metadynamics node alone, d = 2 over (s, z): 1, 255, 256 and 257 hills within +-2 sigma, energy and derivative;
    metad_values equals cvs() bitwise; deposited centres are the bits of cvs()"""
    run_check('metad', tmp_path, 300)


def test_captured_graph_replays_the_deposition(tmp_path):
    """12 rounds of (s, z) well-tempered metadynamics under UPSIDE_HIP_GRAPH=1 and =0: two runs of one setting bit-identical;
    hills, positions and momenta bit-identical between the settings"""
    res = {}
    for g in ('1', '0'):
        run_check('graph', tmp_path, 300, env={'UPSIDE_HIP_GRAPH': g})
        res[g] = np.load(str(tmp_path / ('graph%s.npz' % g)))
    same = dict((k, bool(np.array_equal(res['1'][k], res['0'][k]))) for k in ('pos', 'mom', 'centers', 'weights'))
    print('UPSIDE_HIP_GRAPH=1 against =0, bit-identical: %s' % same)
    assert all(same.values())


def test_md_holds_s_at_its_window(tmp_path):
    """trpcage20 with its full potential, 8 systems at T = 0.8, path_s over K = 8 frames of the CA atoms with spring_const 10 and
    centres s = 2 (four systems) and s = 7 (four): after 200 rounds every s is closer to its own centre than to the other group's
    (the centres are 5 apart: a margin of 2.5); positions finite"""
    run_check('md', tmp_path, 300)


def test_recording_output_cv_and_mbar(tmp_path):
    """record_cvs over 20 rounds equals alternating run_rounds and cvs() bitwise; upside_hip on a file with both kinds in
    /input/collective_variables writes /output/cv whose rows equal the yardstick on the stored frames within the bound; a 4-window
    ladder in s fed to umbrella_mbar returns finite free energies"""
    run_check('record', tmp_path, 600)


def test_bad_definitions_are_refused_and_leave_the_previous_one_in_force(tmp_path):
    """K < 2 or K > 64, n < 3, lambda not finite or not positive, frames not finite, a wrong row count, the path arrays missing (NULL
    through upside_hip_cv_define3, a path kind through upside_hip_cv_define2 and upside_hip_cv_define, absent in a file): an error
    with the message, through the entry point and through a file, and cvs() still returns the earlier definition's values; kinds 6
    and 7 still unknown; a file without the path datasets loads as before; a ladder whose files differ in a path dataset is refused
    naming file, node and dataset"""
    run_check('refusals', tmp_path, 300)
