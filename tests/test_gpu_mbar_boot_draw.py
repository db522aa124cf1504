"""GPU tests of the device draw of the MBAR bootstrap counts (upside_hip_mbar_bootstrap_counts, upside_hip_mbar_bootstrap_drawn;
k_mbar_boot_draw* of csrc/kernels_mbar_boot.hip; mbar.bootstrap_counts_device, mbar.bootstrap(draw='device'),
Ensemble.umbrella_mbar(bootstrap_draw='device')): every check runs in a child process with its own time limit
(tests/mbar_boot_draw_gpu_worker.py, which prints each figure before it asserts) against the integer yardstick
tests/mbar_boot_draw_reference.py, itself pinned by tests/test_mbar_boot_draw_config.py.  There is no bound: counts are compared for
equality and solves bit for bit."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mbar_boot_draw_gpu_worker.py')


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


def test_the_drawn_counts_equal_the_yardstick(tmp_path):
    """n_k = (0, 1, 2, 255, 256, 257, 1000, T - 1, T, T + 1, 2 T + 3) with T = UPK_MBAR_BOOT_DRAW_TILE, the size up to which a state is
    counted in LDS and above which it is counted by global atomics (T + 1 is the state just above); 5 replicates, seed 2^40 + 3;
    block absent, 7 everywhere, and (1, 1, 2, 3, 256, 300, 64, T, T + 5, 2, 10^6) per state; samples grouped by state and under a
    shuffled state_of_sample: the uint16 counts of bootstrap_counts_device are equal to the yardstick's"""
    run_check('draw_equals_reference', tmp_path, 120)


def test_a_replicates_counts_do_not_depend_on_the_call(tmp_path):
    """replicates 3..4 by first=3 are rows 3..4 of a 9-replicate call; two calls give the same bits; bootstrap(draw='device',
    want_counts=True) at a workspace holding chunk = 2 returns the counts and the solve of the default workspace"""
    run_check('independence', tmp_path, 120)


def test_the_solve_on_drawn_counts_equals_the_old_entry_point_fed_those_counts(tmp_path):
    """case_periodic with profile columns: bootstrap(draw='device', block=..., want_counts=True) returns f_boot, columns, n_iter and
    last_delta bit-identical to bootstrap(counts=those counts) through upside_hip_mbar_bootstrap"""
    run_check('solve_equals_host_fed', tmp_path, 120)


def test_umbrella_ladder_with_block_bootstrap_end_to_end(tmp_path):
    """trpcage20_7A, 8 windows, a synthetic AR(1)-modulated series passed as series=: umbrella_mbar(n_bootstrap=16,
    bootstrap_draw='device', bootstrap_block='auto') -- boot_block equals mbar.block_lengths of the g that
    timeseries.statistical_inefficiency returns, f_boot equals mbar.bootstrap fed the yardstick's counts bit for bit, no boot_counts
    key; a call without the new options returns today's key set; tools/umbrella_mbar.py --bootstrap 16 --bootstrap-draw device
    --bootstrap-block auto prints the same sigma to its six decimals"""
    run_check('end_to_end', tmp_path, 300)


def test_refusals_state_their_reason_and_leave_the_library_usable(tmp_path):
    """every refusal of the two entry points with its message; good calls afterwards return the bits of the ones before"""
    run_check('refusals', tmp_path, 120)
