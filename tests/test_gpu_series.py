"""GPU tests of the time-series analysis on the device (upside_hip_series_inefficiency, csrc/kernels_series.hip; timeseries.py;
Ensemble.umbrella_mbar(decorrelate=True)): every check runs in a child process with its own time limit (tests/series_gpu_worker.py,
which prints each figure before it asserts) against the float64 yardstick tests/series_reference.py, itself pinned by
tests/test_series_config.py.  Bound: |g - g_ref| <= 1e-9 max(1, g_ref) (both sides are fp64; a sum of up to 4099 products carries
about N eps ~ 1e-12: three orders of margin); stop_lag and the chosen origin are compared exactly, on cases whose yardstick shows no
|C(t)| below 1e-6 where a stop is decided and a gap of 1e-3 between the best and the second-best origin; two calls are compared
bitwise."""
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'series_gpu_worker.py')


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


def test_inefficiency_matches_the_float64_yardstick(tmp_path):
    """n_series in {1, 3, 65} x T in {16, 63, 64, 65, 257, 1000, 4099} (below, at and above a tile, a k-step, a lag block and a piece),
    seeded AR(1) series with phi in {0, 0.5, 0.9, 0.98} (stop lags from 4 to 601: up to five lag blocks), one origin and 8 origins at
    multiples of T // 8 (segments that start inside a tile), one batch of unequal lengths with NaN behind each series' end: g, mean,
    variance and n_eff within the bound, stop_lag and the best origin exact, everything finite; detect_equilibration over 64 origins
    picks the yardstick's origin"""
    run_check('parity', tmp_path, 300)


def test_stressed_series(tmp_path):
    """a series at 1e6 with unit scatter within 1e-7 max(1, g) (products formed before centring would miss it by three orders);
    constant series give g = 1, stop_lag = 0; a drift of five sigma decaying over T / 8 moves the origin to the yardstick's, above 0;
    white noise keeps origin 0 with g = 1; max_lag below the natural stop (1, 5 and around the lag block of 128) gives stop_lag =
    max_lag + 1; mintime 1 and 10; tails under 16 samples give g = 0, stop_lag = -1; everything returned is finite"""
    run_check('stress', tmp_path, 300)


def test_two_calls_return_the_same_bits_and_a_series_does_not_see_its_batch(tmp_path):
    """65 series twice: the same bits; series 0 alone and as the last of 3 has the bits it has in the 65 (T = 4099 with 8 origins,
    T = 1000 with one, T = 65 with 8)"""
    run_check('reproducible', tmp_path, 300)


def test_umbrella_ladder_decorrelated_end_to_end(tmp_path):
    """the setup of test_umbrella_ladder_end_to_end (trpcage20_7A, 8 windows on the end-to-end distance, record_cvs(1), 200 rounds):
    umbrella_mbar(decorrelate=True) returns t0 and kept equal to the yardstick on the own-state bias series and g within the bound;
    n_k are the lengths of kept; f and sigma have the bits of mbar.mbar and free_energy_uncertainty called on the kept samples;
    decorrelate=False returns the bits of a direct call on the full series and none of the new keys"""
    run_check('end_to_end', tmp_path, 300)


def test_refusals_state_their_reason_and_leave_the_library_usable(tmp_path):
    """every refusal of the entry point (no series, no origin, lengths outside 1 .. stride, origins negative or not ascending,
    mintime < 1, max_lag < 1, NULL arrays, entries that are not finite, n_series x stride at 2^40): an error with its message; a good
    call afterwards returns the bits of the one before"""
    run_check('refusals', tmp_path, 300)
