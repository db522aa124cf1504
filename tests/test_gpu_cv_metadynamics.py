"""GPU tests of the cv_metadynamics node (a history-dependent bias on the device collective variables): every check runs in a child
process with its own time limit (tests/cv_metad_gpu_worker.py, which prints each figure before it asserts) against the float64
yardstick tests/cv_metad_reference.py, itself pinned by tests/test_cv_metadynamics_config.py.  The configuration files are written
into the test's temporary directory; everything runs on trpcage20 (60 atoms).  Tolerances: 1e-6 relative for energies and
well-tempered weights, parity_util.RTOL as relative RMS and 10 x RTOL for the largest element of a derivative; equalities between
engine runs, and between hill centres and cvs(), are bitwise."""
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cv_metad_gpu_worker.py')


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


def test_bias_matches_the_yardstick(tmp_path):
    """the node alone with hills loaded by set_metad_hills (centres within +-2 sigma of the current values, weights in [0.1, 1]):
    d = 1 (rg), 2 (rmsd over CA + contacts), 3 (rg over 3 atoms, a distance, contacts with one pair), 4; 0, 1, 255, 256, 257 and
    1000 hills; no hills: energy and every force component exactly 0; the values are the bits of cvs(); two coincident atoms in a
    distance CV: finite, zero force from that CV"""
    run_check('bias', tmp_path, 300)


def test_deposition_follows_the_cv_kernel(tmp_path):
    """pace 2, capacity 5, the full trpcage potential at T = 0.8, seven calls of run_rounds(2): the newest centre is the bits of
    cvs(), its weight `height` exactly, earlier hills unchanged, 5 hills and 7 attempts at the end; with kdT = 2: weight 0 is
    `height`, weight k within 1e-6 of height exp(-V_yardstick / kdT) and strictly below `height`"""
    run_check('deposit', tmp_path, 300)


def test_captured_graph_replays_the_deposition(tmp_path):
    """12 rounds of that MD under UPSIDE_HIP_GRAPH=1 and =0: two runs of one setting bit-identical; hills, positions and momenta
    agree bit for bit between the settings where they do for the unmodified fixture"""
    res = {}
    for g in ('1', '0'):
        run_check('graph', tmp_path, 300, env={'UPSIDE_HIP_GRAPH': g})
        res[g] = np.load(str(tmp_path / ('graph%s.npz' % g)))
    free_same = all(np.array_equal(res['1'][k], res['0'][k]) for k in ('free_pos', 'free_mom'))
    same = all(np.array_equal(res['1'][k], res['0'][k]) for k in ('pos', 'mom', 'centers', 'weights'))
    print('UPSIDE_HIP_GRAPH=1 against =0: the unmodified fixture bit-identical: %s; with the node (hills included): %s' % (free_same, same))
    if free_same:
        assert same


def test_batch_is_deterministic_and_independent_of_position(tmp_path):
    """shared = 0, 64 and 600 systems at distinct positions with their own hills; systems 0, 7 and the last share positions and 300
    hills: bit-identical within and across the engines and equal to a one-system engine; two runs bit-identical; swap_systems leaves
    the hills with the system index"""
    run_check('batch', tmp_path, 300)


def test_walkers_fill_one_shared_list(tmp_path):
    """shared = 1, 4 systems, pace 1, capacity 10: after 3 rounds 8 hills are visible (the third deposit is dropped for all) and 3
    attempts counted; slot 4 k + s holds system s's cvs() of round k; each system's bias equals, bitwise, an unshared one-system
    engine holding the same 8 hills"""
    run_check('walkers', tmp_path, 300)


def test_hills_read_back_and_written_hills_reach_a_captured_graph(tmp_path):
    """set_metad_hills then metad_hills is bitwise; after 3 written hills two deposits land in slots 3 and 4; hills written after
    run_rounds, captured graph on, reach the next force pass: energies equal a fresh engine with those hills at the same positions"""
    run_check('readback', tmp_path, 300, env={'UPSIDE_HIP_GRAPH': '1'})


def test_upside_hip_writes_and_continues_hills(tmp_path):
    """upside_hip for 6 rounds at pace 2 leaves 3 hills under /output/metadynamics/<node>; copied to /input/metadynamics/<node> of a
    second configuration, that run's frame-0 potential equals Ensemble + set_metad_hills + energies() at the initial structure
    (1e-6) and it ends with 6 hills"""
    run_check('cli', tmp_path, 600)


def test_refusals_leave_the_process_usable(tmp_path):
    """sigma <= 0 or not finite, d = 5, pace 0, capacity 0, kdT < 0, height 0; n_hill > capacity, hills that are not finite, a
    shared n_hill that is no multiple of the systems; files of one engine differing in sigma: each by its message, and after each
    the process builds a good engine"""
    run_check('refusals', tmp_path, 300)
