"""Host-only test of tools/refine_groups.py: the trip model of the list refine (a row served by a group of LPR lanes, the 64 / LPR groups
of a wavefront waiting for the longest row of their set) on hand-made row lengths, counted by hand."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import refine_groups as RG       # noqa: E402


def test_rows_per_set():
    assert [RG.rows_per_set(l) for l in (16, 32, 64)] == [4, 2, 2]


def test_trips_of_a_run_counted_by_hand():
    # every border of a 16-lane trip, rows in run order
    cnt = [0, 1, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129]
    # LPR 16, sets of four: (0 1 15 16) 1 trip, (17 31 32 33) 3, (64 65 128 129) 9
    assert RG.trips_of_run(cnt, 16) == (13, 3)
    # LPR 32, sets of two: 1 + 1 + 1 + 2 + 3 + 5
    assert RG.trips_of_run(cnt, 32) == (13, 6)
    # two rows per trip of 64 words each: 1 + 1 + 1 + 1 + 2 + 3
    assert RG.trips_of_run(cnt, 64) == (9, 6)


def test_a_ragged_run_and_empty_sets():
    # five rows: the last set has one row; a set of empty rows makes no trip
    assert RG.trips_of_run([40, 0, 0, 0, 3], 16) == (4, 2)
    assert RG.trips_of_run([40, 0, 0, 0, 3], 32) == (2 + 0 + 1, 3)
    assert RG.trips_of_run([0, 0, 0, 0], 16) == (0, 1)
    assert RG.trips_of_run([16, 16, 16, 16, 17, 0, 0, 0], 16) == (3, 2)


def test_rows_are_dealt_to_wavefronts_in_runs():
    cnt = np.array([16] * 8 + [17] * 8 + [1])
    # runs of 8 rows: (2 sets x 1 trip), (2 sets x 2 trips), (1 set, 1 trip)
    assert RG.trips_of_rows(cnt, 16, 8) == (7, 5, 3)
    # one run of 17 rows: sets (16 x4) (16 x4) (17 x4) (17 x4) (1)
    assert RG.trips_of_rows(cnt, 16, 64) == (1 + 1 + 2 + 2 + 1, 5, 1)


def test_expected_trips_of_independent_rows():
    one_length = np.zeros(21); one_length[20] = 7          # every row holds 20 words
    assert RG.expected_trips_per_set(one_length, 16) == 2.
    assert RG.expected_trips_per_set(one_length, 32) == 1.
    half_empty = np.zeros(41); half_empty[0] = 5; half_empty[40] = 5
    # a set makes ceil(40 / LPR) trips unless all its rows are empty: probability 1/4 for two rows, 1/16 for four
    assert abs(RG.expected_trips_per_set(half_empty, 32) - 2 * 0.75) < 1e-12
    assert abs(RG.expected_trips_per_set(half_empty, 16) - 3 * (15. / 16.)) < 1e-12
    assert abs(RG.expected_trips_per_set(half_empty, 64) - 1 * 0.75) < 1e-12
