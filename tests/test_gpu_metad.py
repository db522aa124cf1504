"""GPU tests of the metadynamics analysis on the device (upside_hip_metad_bias and upside_hip_metad_grid, csrc/kernels_metad.hip;
metad.py; Ensemble.metad_reweight): every check runs in a child process with its own time limit (tests/metad_gpu_worker.py, which
prints each figure before it asserts) against the float64 yardstick tests/metad_reference.py, itself pinned by
tests/test_metad_config.py.  Bounds, with A(x) = sum |w_h| e_h(x): |V - V_ref| <= 1e-11 A and |lse - lse_ref| <= 1e-11 + 1e-11 |scale|
max_g A(g) -- both sides are fp64, sums of at most about 10^3 terms carry about 1e-13 and an exponent of up to 128 carries 4e-14: two
orders of margin; two calls are compared bitwise."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'metad_gpu_worker.py')


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


def test_bias_at_points_matches_the_float64_yardstick(tmp_path):
    """d = 1 .. 4; 1, 3 and 65 lists of unequal lengths from {0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000} hills (one of them empty)
    with 1, 255, 256, 257 or 1000 points each; n_visible NULL, all 0, ascending and shuffled; one periodic dimension with hills beside
    +-pi; weights of both signs: V within 1e-11 A of the yardstick, and exactly 0 where no hill is visible"""
    run_check('bias', tmp_path, 300)


def test_grid_bias_and_log_sum_exps_match_the_float64_yardstick(tmp_path):
    """axes from {1, 15, 16, 17, 63, 64, 65, 100} in d = 1 and 2 (rows and columns on both sides of the tile borders), 5 x 13 x 17,
    3 x 5 x 7 x 9 and other small grids in d = 3 and 4, the hill counts above, checkpoints at 0 (lse = ln G), at counts that are no
    multiples of 4, repeated, and ending below the list's length, scales {0, 1, -2.5}: V_last and lse within the bounds, V_last within
    the bound of upside_hip_metad_bias fed the grid as points, lse unchanged with V_last NULL; both paths forced at shapes the routing
    sends to the other; a segment longer than a slab (4000 x 8, partial ranges) and a grid of 272 tiles (none)"""
    run_check('grid', tmp_path, 300)


def test_two_calls_return_the_same_bits_and_a_list_does_not_see_its_batch(tmp_path):
    """65 lists on 33 x 20, 50 and 5 x 13 x 17: two calls return the same bits; list 0 alone and as the last of 3 has the bits it has
    among the 65; chunks of one list and of a few lists (forced through the workspace argument of the internal solve) return the bits of
    the unchunked run; the same for the bias at points"""
    run_check('reproducible', tmp_path, 300)


def test_reweighting_of_a_run_end_to_end(tmp_path):
    """trpcage20_7A, a well-tempered node on the end-to-end distance and Rg, pace 2, record_cvs(1), 60 rounds, 4 systems, once with a
    list per system and once with a shared list: metad_reweight returns n_visible, V, c and log_w equal to the yardstick on metad_hills
    and read_cvs within the bounds; at every deposit round the frame's CV bits are the hill's centre and |V + kdT ln(w_hill / height)|
    <= 2e-7 kdT + 1e-11 A (the float32 rounding of the stored weight), which ties the prefix rule to what the engine applied; a CV of
    the node that is not recorded raises ValueError naming it"""
    run_check('end_to_end', tmp_path, 300)


def test_refusals_state_their_reason_and_leave_the_library_usable(tmp_path):
    """every refusal of the two entry points: an error with its message, naming the entry point; good calls afterwards return the bits
    of the ones before"""
    run_check('refusals', tmp_path, 300)


def test_the_command_line_tool_on_a_run_of_upside_hip(tmp_path):
    """trpcage20_7A with the node on the end-to-end distance and Rg and three recorded CVs, 24 rounds of `upside_hip` with a frame
    every 2 (12 frames, 12 hills): every frame after the first is the centre of the hill deposited at its round; tools/metad_reweight.py prints F_hills on a
    12 x 12 grid and the reweighted profile along the CV that was not biased, both equal to the yardstick on the file's hills and
    frames to the six digits printed"""
    run_check('cli', tmp_path, 300)
