"""The float64 definition of the alignment scores (tests/alignment_score_refs.py) on cases worked out by hand.  Host-only."""
import math

import numpy as np
import pytest

from tests import alignment_score_refs as R


def _one_hot(n, at, Ha=2, N=1, S=None):
    w = np.zeros((Ha, N, S or n))
    w[:, :, at] = 3.5
    return w


def test_one_hot_inside_its_interval_has_all_the_mass_and_no_spread():
    n = 40
    w = _one_hot(n, 17, N=2)
    mass, spread = R.token_scores(w, n, [15, 20], 0)          # token 0 owns frames 15 .. 19, token 1 frames 20 .. 39
    assert mass[0] == 1.0 and spread[0] == 0.0
    assert mass[1] == 0.0 and spread[1] == 0.0                # the same attention, but the path put token 1 elsewhere
    mass, _ = R.token_scores(w, n, [15, 20], 3)               # a collar of 3 reaches frame 17 from token 1's window
    assert mass.tolist() == [1.0, 1.0]


@pytest.mark.parametrize("n, lo, hi, c", [(50, 10, 20, 0), (50, 10, 20, 4), (7, 2, 3, 1), (1500, 700, 731, 3)])
def test_uniform_row_mass_and_closed_form_spread(n, lo, hi, c):
    w = np.full((3, 2, n), 0.25)
    mass, spread = R.token_scores(w, n, [lo, hi], c)
    assert mass[0] == pytest.approx((hi - lo + 2 * c) / n, rel=1e-12)        # [lo - c, hi + c) lies inside 0 .. n here
    # a uniform distribution over 0 .. n-1 has variance (n^2 - 1) / 12
    assert spread[0] == pytest.approx(0.02 * math.sqrt((n * n - 1) / 12.0), rel=1e-12)
    assert spread[1] == spread[0]                                            # the spread does not look at the path
    assert mass[1] == pytest.approx((n - hi + c) / n, rel=1e-12)             # the last token runs to n: the collar is cut there


def test_collar_is_clipped_at_both_ends():
    n = 10
    w = np.full((1, 2, n), 1.0)
    mass, _ = R.token_scores(w, n, [1, 8], 5)
    assert mass[0] == pytest.approx(1.0)                      # [1 - 5, 8 + 5) -> [0, 10)
    assert mass[1] == pytest.approx(7 / 10)                   # [8 - 5, 10 + 5) -> [3, 10)
    mass, _ = R.token_scores(w, n, [1, 8], n)                 # a collar of n covers everything from anywhere
    assert mass.tolist() == pytest.approx([1.0, 1.0])
    # frames at or beyond n never count, whatever they hold
    wide = np.concatenate([w, np.full((1, 2, 6), np.nan)], axis=2)
    m2, s2 = R.token_scores(wide, n, [1, 8], 5)
    m1, s1 = R.token_scores(w, n, [1, 8], 5)
    assert m1.tolist() == m2.tolist() and s1.tolist() == s2.tolist()


def test_equal_consecutive_first_frames_give_a_one_frame_window():
    n = 12
    w = np.zeros((1, 3, n))
    w[0, :, 4] = 1.0
    w[0, :, 5] = 3.0
    mass, spread = R.token_scores(w, n, [4, 4, 6], 0)
    assert mass[0] == pytest.approx(0.25)                     # fc[0] == fc[1]: hi = lo + 1, frame 4 alone
    assert mass[1] == pytest.approx(1.0)                      # frames 4 .. 5
    assert mass[2] == 0.0                                     # frames 6 .. 11
    # two frames with weights 1/4 and 3/4: variance 3/16 frames^2
    assert spread.tolist() == pytest.approx([0.02 * math.sqrt(3 / 16)] * 3)


def test_undefined_cases_are_nan():
    w = np.full((2, 3, 8), 1.0)
    mass, spread = R.token_scores(w, 0, [0, 0, 0], 2)         # no frame reached the DTW
    assert np.all(np.isnan(mass)) and np.all(np.isnan(spread))
    w[1, 1, :] = 0.0                                          # one head saw nothing for token 1
    mass, spread = R.token_scores(w, 8, [0, 2, 5], 0)
    assert np.isnan(mass).tolist() == [False, True, False] and np.isnan(spread).tolist() == [False, True, False]
    w[1, 1, :] = 1.0
    w[1, 1, 6:] = 0.0
    mass, _ = R.token_scores(w[:, :, :], 6, [0, 2, 5], 0)     # zero only behind n: not a zero row
    assert not np.any(np.isnan(mass))
    mass, spread = R.token_scores(w, 8, [0, -1, 5], 0)        # no first frame for token 1
    assert np.isnan(mass).tolist() == [False, True, False] and np.isnan(spread).tolist() == [False, True, False]
    assert mass[0] == pytest.approx(1 / 8)                    # fc[1] < 0 leaves token 0 with hi = lo + 1


def test_heads_are_normalised_before_they_are_averaged():
    n = 4
    w = np.zeros((2, 2, n))
    w[0, :] = [1, 1, 0, 0]                                    # head 0: half its attention on frame 0
    w[1, :] = [0, 0, 0, 1000]                                 # head 1: all of it on frame 3, with a large scale
    mass, spread = R.token_scores(w, n, [0, 1], 0)            # token 0 owns frame 0 alone
    assert mass[0] == pytest.approx(0.25)                     # mean of 1/2 and 0, not 1 / 1002
    pbar = np.array([0.25, 0.25, 0.0, 0.5])
    mu = float((pbar * np.arange(4)).sum())
    assert spread[0] == pytest.approx(0.02 * math.sqrt(float((pbar * (np.arange(4) - mu) ** 2).sum())))


def test_word_values_are_group_means_and_a_dropped_token_counts_nowhere():
    mass = np.array([0.9, 0.5, 0.1, 1000.0, 0.3, np.nan, 0.7])
    spread = np.array([0.1, 0.3, 0.2, 1000.0, 0.4, 0.5, 0.6])
    groups = [[0, 1], [2], [4, 6], [5, 6]]                    # token 3 was dropped by a seam merge: in no group
    got = R.word_scores(groups, mass, spread)
    assert got[0] == (pytest.approx(0.7), pytest.approx(0.2))
    assert got[1] == (pytest.approx(0.1), pytest.approx(0.2))
    assert got[2] == (pytest.approx(0.5), pytest.approx(0.5))
    assert math.isnan(got[3][0]) and got[3][1] == pytest.approx(0.55)         # NaN if any member is NaN
    assert all(abs(m) < 2 for m, _ in got[:3])


def test_ncols_follow_the_double_slice_rule():
    assert R.timestamp_ncols([3000, 3000]) == [1500, 1500]
    assert R.timestamp_ncols([1000, 1000]) == [500, 500]
    assert R.timestamp_ncols([1000, 3000]) == [500, 1500]
    assert R.timestamp_ncols([0]) == [0] and R.timestamp_ncols([1]) == [0] and R.timestamp_ncols([7]) == [3]
    assert R.timestamp_ncols([-4]) == [1496]                  # python's negative slice, twice


def test_bounds_come_from_the_number_formats():
    assert R.mass_tolerance(1) == 2.0 ** -23 and R.mass_tolerance(1500) == 3000 * 2.0 ** -24
    lo, hi = R.spread_interval(np.array([0.0, 100.0]), 749)
    assert lo[0] == 0.0 and 0 <= hi[0] < 1e-11               # a one-hot row: the float64 reference's own error, 1e-12 s
    assert lo[1] < 0.2 < hi[1] and (hi[1] - lo[1]) < 0.2 * (2 * 749 + 5) * R.U
