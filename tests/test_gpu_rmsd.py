"""GPU tests of the pairwise RMSD of frames on the device (upside_hip_frames_create, upside_hip_rmsd_matrix, _nearest, _count,
csrc/kernels_rmsd.hip; upside-md_amd/cluster.py; tools/cluster_frames.py): every check runs in a child process with its own time
limit (tests/rmsd_gpu_worker.py, which prints each figure before it asserts) against the float64 yardstick tests/rmsd_reference.py,
itself pinned by tests/test_rmsd_config.py.  Bound, on d2 where it is uniform: |d2 - d2_ref| <= 1e-12 (G_a + G_b) / n (both sides are
fp64; a sum of n <= 1024 products carries about n eps ~ 2e-13 of G; the yardstick's two float64 routes differ by 1.4e-15: three
orders over what the yardstick shows, about one over the worst-case sum).  It makes distances below about 1e-6 sqrt((G_a + G_b) / n)
rounding noise: two copies of a frame come out near 1e-7 A, not 0, in the yardstick too.  Nearest indices and counts are compared
exactly, on inputs whose yardstick keeps the competing d2 1e-9 (G_a + G_b) / n apart; two calls are compared bitwise."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rmsd_gpu_worker.py')


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


def test_matrix_nearest_and_count_match_the_float64_yardstick(tmp_path):
    """n in {3, 4, 5, 63, 64, 65, 168} (below, at and above the k-step and an LDS chunk) x F in {1, 2, 15, 16, 17, 63, 64, 65, 130}
    (below, at and above a 16-block and a 64-tile; three tiles with a ragged edge): the symmetric matrix within the bound, its diagonal
    exactly 0, bitwise symmetric; rectangular 1 x 130, 130 x 1, 65 x 17 and 17 x 65 and index lists that permute and repeat frames;
    nearest and count_within on the same shapes against 17 and 65 centres (rows = a centre plus noise of 0.05; the cutoff in the
    widest gap of the middle three fifths of the yardstick's distances): dist within the bound, index and count exact"""
    run_check('parity', tmp_path, 300)


def test_stressed_frames(tmp_path):
    """duplicates at different tile positions, a mirror image (d > 0, the Kabsch value), a pair differing by 1e-3 noise, all frames
    translated by 1e4, collinear atoms (lambda degenerate), planar frames, n = 3, one frame scaled by 100 against one at unit scale:
    the bound holds everywhere, nothing is negative or NaN; a pair has the same bits at every tile position, and among duplicate
    centres nearest returns the lowest position"""
    run_check('stress', tmp_path, 300)


def test_two_calls_return_the_same_bits_and_a_pair_does_not_see_its_call(tmp_path):
    """the 130-frame matrix twice: the same bits; entry (a, b), a < b, has the bits it has when a and b are alone in a 1 x 1 rectangular
    call, alone in a frame set of their own, and when an index list moves them to other tile positions; nearest over 65 centres gives
    the same bits and indices as one list and assembled by the host from two calls over 32 and 33 centres; counts add up likewise"""
    run_check('reproducible', tmp_path, 300)


def test_kcenters_and_gromos_return_the_yardsticks_clusters(tmp_path):
    """130 frames as 5 well-separated chains plus noise (40, 30, 26, 20 and 14 members): kcenters(k = 5; a cutoff; another first frame;
    k = 3) and gromos(cutoff) return exactly the centres, assignment and sizes of the yardstick's restatements on the yardstick matrix;
    config.path_neighbour_table is the matrix of its frames"""
    run_check('clustering', tmp_path, 300)


def test_ensemble_frames_and_the_tool_end_to_end(tmp_path):
    """trpcage20_7A as an Ensemble of 16 systems, 20 MD rounds: cluster.rmsd_matrix(ens.get_pos(), atoms=C-alpha) against the yardstick
    within the bound; tools/cluster_frames.py on an /output/pos file of these frames written with h5lite reproduces gromos"""
    run_check('end_to_end', tmp_path, 300)


def test_refusals_state_their_reason_and_leave_the_library_usable(tmp_path):
    """every refusal of the entry points (NULL handles and outputs, n_atom < 3, n_frame < 1, 2^40 coordinates, a coordinate that is not
    finite, different n_atom, nA or nB < 1 or not the set's size, an index outside its set, a bad cutoff, 2^40 matrix entries, a
    device allocation that fails): status 1 with its message; good calls afterwards return the bits of the ones before"""
    run_check('refusals', tmp_path, 300)
