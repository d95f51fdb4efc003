"""CPU suite: the numpy statement of ssde_path_speed (tests/speed_ref.py) on the draws of tests/draws_ref.py,
against a per-track, per-draw, per-row loop written here from the definition, and the rules the definition implies: NaN for a
track without a state row and for a (track, draw) with a non-finite velocity and for nothing else, counts that lose only the row
of a NaN, positions that are not looked at, a zero speed that adds nothing to the resultant, the smaller row on a tie, and --
bitwise -- the independence of the draw batching (counts adding up), weight = None as ones, and thresholds as independent columns.

Limit against the loop: 1e-13 (1 + max|ref|).  Both sides add the same at most 8 terms per statistic, in different orders; each
addition rounds by 1.1e-16 relative, so the two sums differ by ~1e-15 relative at the most.  The row of the maximum and the counts
are exact."""
import math

import numpy as np
import pytest

from cases import make_spec, problem_from_spec
from draws_ref import draws_ref
from speed_cases import clear_maxima, clear_of_thresholds, dt_weights, make_thresholds
from speed_ref import speed_ref, velocity_columns

LENGTHS = [9, 1, 2, 7]                           # rows 0-8 | 9 | 10-11 | 12-18
NA_ROWS = (3, 15)
_CASE = {}


def _case(d):
    """problem, eight reference draws, thresholds and weights of a CTCRW of d columns, computed once"""
    if d not in _CASE:
        spec = make_spec(f"sh_CTCRW_{d}", "CTCRW", d, seed=71 + d, lengths=LENGTHS, na_rows=NA_ROWS)
        pb = problem_from_spec(spec)
        draws = draws_ref(pb, spec["par"], seed=13, n_draws=8)
        draws.setflags(write=False)
        thr = make_thresholds(draws, pb.seg_start, d, 8)
        w = dt_weights(pb.seg_start, pb.times)
        _CASE[d] = (spec, pb, draws, thr, w)
    return _CASE[d]


def _brute(draws, seg_start, d, thr, weight):
    nd, n, _ = draws.shape
    cols = velocity_columns(d)
    bounds = list(seg_start) + [n]
    out = np.full((nd, len(bounds) - 1, 5 + len(thr)), np.nan)
    below = np.zeros((n, len(thr)), dtype=np.uint32)
    for q in range(nd):
        for k in range(len(bounds) - 1):
            first, last = bounds[k], bounds[k + 1] - 1
            if last < first + 1:
                continue
            vel = [[float(draws[q, j, c]) for c in cols] for j in range(first + 1, last + 1)]
            spd = [math.sqrt(v[0] ** 2 + v[1] ** 2) if d > 1 else abs(v[0]) for v in vel]
            for j, s in zip(range(first + 1, last + 1), spd):
                for r, t in enumerate(thr):
                    if math.isfinite(s) and s <= t:
                        below[j, r] += 1
            if any(not math.isfinite(x) for v in vel for x in v):
                continue
            total, best, arg, res, band = 0.0, -1.0, -1, [0.0, 0.0], [0.0] * len(thr)
            for j, v, s in zip(range(first + 1, last + 1), vel, spd):
                total += weight[j] * s
                if s > best:                                         # strictly: the first (smallest) row keeps a tie
                    best, arg = s, j
                if s > 0:
                    for c in range(d):
                        res[c] += weight[j] * (v[c] / s)
                for r, t in enumerate(thr):
                    if s <= t:
                        band[r] += weight[j]
            out[q, k, :5] = [total, best, arg, res[0], res[1]]
            out[q, k, 5:] = band
    return out, below


@pytest.mark.parametrize("d", [1, 2])
def test_speed_ref_is_the_definition(d):
    spec, pb, draws, thr, w = _case(d)
    assert len(thr) == 8 and thr[5] == 0.0 and np.isinf(thr[6]) and np.all(thr[:5] > 0)
    assert clear_of_thresholds(draws, pb.seg_start, d, thr) and clear_maxima(draws, pb.seg_start, d)
    got, gb = speed_ref(draws, pb.seg_start, d, thresholds=thr, weight=w)
    ref, rb = _brute(draws, pb.seg_start, d, thr, w)
    assert got.shape == (8, 4, 13) and gb.shape == (19, 8) and gb.dtype == np.uint32
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    for k in range(13):
        gap = np.nanmax(np.abs(got[:, :, k] - ref[:, :, k])) / (1.0 + np.nanmax(np.abs(ref[:, :, k])))
        print(f"GAP ref-loop CTCRW d={d} stat {k}: {gap:.2e}")
        assert gap <= 1e-13, (k, gap)
    assert np.array_equal(got[:, :, 2], ref[:, :, 2], equal_nan=True) and np.array_equal(gb, rb)
    band = got[:, [0, 3], 5:10]
    assert np.any(band > 0) and np.any(band == 0)                    # both branches of the indicator
    assert np.all(got[:, [0, 2, 3], 5 + 5] == 0.0)                   # thr = 0 holds no row
    if d == 1:
        assert np.all(got[:, [0, 2, 3], 4] == 0.0)


@pytest.mark.parametrize("d", [1, 2])
def test_nan_rules_counts_and_positions(d):
    spec, pb, draws, thr, w = _case(d)
    got, gb = speed_ref(draws, pb.seg_start, d, thresholds=thr, weight=w)
    assert np.all(np.isnan(got[:, 1, :]))                           # the one-row track
    assert np.all(np.isfinite(got[:, [0, 2, 3], :]))
    assert np.all(got[:, 2, 2] == 11.0)                             # two rows: one state row, its own maximum
    first = np.asarray(pb.seg_start)
    assert np.all(gb[first] == 0)                                   # rows without a state
    state = np.setdiff1d(np.arange(pb.n), first)
    assert np.all(gb[state, 6] == 8) and np.all(gb[:, 5] == 0) and np.all(gb[state, 7] == 8)   # +inf: every draw; 0: none; above all: every draw
    bad = np.array(draws)
    bad[1, 14, velocity_columns(d)[-1]] = np.nan                    # one velocity of (track 3, draw 1)
    hit, hb = speed_ref(bad, pb.seg_start, d, thresholds=thr, weight=w)
    assert np.all(np.isnan(hit[1, 3, :]))
    hit[1, 3, :] = got[1, 3, :]
    assert np.array_equal(hit, got, equal_nan=True)                 # ... and nothing else
    lost = gb.astype(np.int64) - hb.astype(np.int64)                # the same NaN lowers only its own row's counts, by the one draw
    assert np.all(lost[np.arange(pb.n) != 14] == 0) and np.array_equal(lost[14], (speed_at(draws, d, 1, 14) <= thr).astype(np.int64))
    assert lost[14, 6] == 1
    inf = np.array(draws)
    inf[2, 5, velocity_columns(d)[0]] = np.inf                      # +-inf is not finite either, and is not counted below +inf
    hi, hib = speed_ref(inf, pb.seg_start, d, thresholds=thr, weight=w)
    assert np.all(np.isnan(hi[2, 0, :])) and hib[5, 6] == 7
    pos = np.array(draws)                                           # a position column is no velocity
    pos[:, :, 0::2] = np.nan
    ps, pbl = speed_ref(pos, pb.seg_start, d, thresholds=thr, weight=w)
    assert np.array_equal(ps, got, equal_nan=True) and np.array_equal(pbl, gb)


def speed_at(draws, d, q, j):
    v = draws[q, j, velocity_columns(d)]
    return float(np.abs(v[0]) if d == 1 else np.sqrt((v ** 2).sum()))


@pytest.mark.parametrize("d", [1, 2])
def test_zero_speed_and_ties(d):
    spec, pb, draws, thr, w = _case(d)
    got, _ = speed_ref(draws, pb.seg_start, d, thresholds=thr, weight=w)
    still = np.array(draws)
    still[3, 6, 1::2] = 0.0                                         # s = 0 at row 6 of (track 0, draw 3): it adds nothing to the resultant
    z, zb = speed_ref(still, pb.seg_start, d, thresholds=thr, weight=w)
    rows = [j for j in range(1, 9) if j != 6]
    for c in range(d):
        v = draws[3, rows, 2 * c + 1]
        s = np.array([speed_at(draws, d, 3, j) for j in rows])
        assert abs(z[3, 0, 3 + c] - float(np.sum(w[rows] * (v / s)))) <= 1e-13 * (1.0 + abs(z[3, 0, 3 + c]))
    assert np.isfinite(z[3, 0, :]).all() and zb[6, 5] == 1          # ... and 0 <= thr = 0 counts it
    assert z[3, 0, 10] == w[6]
    tie = np.array(draws)                                           # a planted tie: the smaller row
    big = 2.0 * got[5, 3, 1]
    for j in (14, 17):
        tie[5, j, 1::2] = 0.0
        tie[5, j, 1] = -big if j == 14 else big
    t, _ = speed_ref(tie, pb.seg_start, d, thresholds=thr, weight=w)
    assert t[5, 3, 1] == big and t[5, 3, 2] == 14.0


@pytest.mark.parametrize("d", [1, 2])
def test_batching_weights_and_thresholds_bitwise(d):
    spec, pb, draws, thr, w = _case(d)
    whole, wb = speed_ref(draws, pb.seg_start, d, thresholds=thr, weight=w)
    a, ab = speed_ref(draws_ref(pb, spec["par"], seed=13, draw0=0, n_draws=4), pb.seg_start, d, thresholds=thr, weight=w)
    b, bb = speed_ref(draws_ref(pb, spec["par"], seed=13, draw0=4, n_draws=4), pb.seg_start, d, thresholds=thr, weight=w)
    assert np.array_equal(whole, np.concatenate([a, b]), equal_nan=True)          # [0, 8) = [0, 4) + [4, 8)
    assert np.array_equal(wb, ab + bb)                                            # ... with the counts added
    none, nb = speed_ref(draws, pb.seg_start, d, thresholds=thr, weight=None)
    ones, ob = speed_ref(draws, pb.seg_start, d, thresholds=thr, weight=np.ones(pb.n))
    assert np.array_equal(none, ones, equal_nan=True) and np.array_equal(nb, ob) and np.array_equal(nb, wb)
    assert not np.array_equal(none, whole, equal_nan=True)
    perm = np.random.default_rng(5).permutation(8)
    mixed, mb = speed_ref(draws, pb.seg_start, d, thresholds=thr[perm], weight=w)
    assert np.array_equal(mixed[:, :, :5], whole[:, :, :5], equal_nan=True)
    assert np.array_equal(mixed[:, :, 5:], whole[:, :, 5:][:, :, perm], equal_nan=True) and np.array_equal(mb, wb[:, perm])
    bare, none_b = speed_ref(draws, pb.seg_start, d, weight=w)                    # no thresholds
    assert bare.shape == (8, 4, 5) and none_b.shape == (19, 0) and np.array_equal(bare, whole[:, :, :5], equal_nan=True)
