"""Thresholds, preconditions and the comparison shared by the tests of ssde_path_speed (test infrastructure).

A 1e-15 difference between two implementations must flip neither a count nor an argmax.  So the thresholds are
np.round(np.quantile(reference speeds, [.1, .25, .5, .75, .9]), 3) + 5e-4, plus 0, +inf and one value above every speed, and every
comparison asserts on its reference draws, before it compares anything:
  (a) clear_of_thresholds: every finite speed is more than 1e-5 (1 + thr) from every finite threshold;
  (b) clear_maxima: in every (track, draw) with two or more state rows the two largest speeds differ by more than 1e-5 (1 + max).
A seed that violates one is changed, never skipped or masked."""
import numpy as np

from path_cases import dt_weights  # noqa: F401  (the weights are ssde_path_stats')
from speed_ref import speeds, state_rows


def make_thresholds(ref_draws, seg_start, d, n_thr=8):
    """the five quantile thresholds, then 0, +inf and one above every speed; the first n_thr of them"""
    s = speeds(ref_draws, d)[:, state_rows(seg_start, ref_draws.shape[1])]
    s = s[np.isfinite(s)]
    thr = list(np.round(np.quantile(s, [.1, .25, .5, .75, .9]), 3) + 5e-4) + [0.0, np.inf, float(np.ceil(s.max())) + 1.0]
    return np.array(thr[:n_thr], dtype=np.float64)


def threshold_distance(ref_draws, seg_start, d, thr):
    """the smallest |s - thr| / (1 + thr) over finite speeds on state rows and finite thresholds"""
    s = speeds(ref_draws, d)[:, state_rows(seg_start, ref_draws.shape[1])]
    s = s[np.isfinite(s)]
    best = np.inf
    for t in np.asarray(thr, dtype=np.float64).ravel():
        if np.isfinite(t) and s.size:
            best = min(best, np.min(np.abs(s - t)) / (1.0 + t))
    return best


def clear_of_thresholds(ref_draws, seg_start, d, thr):
    return threshold_distance(ref_draws, seg_start, d, thr) > 1e-5


def maxima_gap(ref_draws, seg_start, d):
    """the smallest (largest - second largest) / (1 + largest) over (track, draw) with two or more state rows and finite speeds"""
    s = speeds(ref_draws, d)
    n = s.shape[1]
    bounds = np.r_[np.asarray(seg_start, dtype=np.int64), n]
    best = np.inf
    for k in range(len(bounds) - 1):
        if bounds[k + 1] - bounds[k] < 3:
            continue
        part = np.sort(s[:, bounds[k] + 1:bounds[k + 1]], axis=1)
        ok = np.isfinite(part).all(axis=1)
        if ok.any():
            best = min(best, np.min((part[ok, -1] - part[ok, -2]) / (1.0 + part[ok, -1])))
    return best


def clear_maxima(ref_draws, seg_start, d):
    return maxima_gap(ref_draws, seg_start, d) > 1e-5


def compare(got, ref, tag):
    """(stats, row_below) pairs.  |got - ref| <= 1e-9 (1 + max|ref|) per statistic, identical NaN patterns; statistic 2 (the row of
    the maximum) and the counts exact.  Prints and returns the largest gap."""
    (gs, gb), (rs, rb) = got, ref
    assert gs.shape == rs.shape, (gs.shape, rs.shape)
    assert np.array_equal(np.isnan(gs), np.isnan(rs)), tag
    worst = 0.0
    for k in range(rs.shape[2]):
        g, r = gs[:, :, k], rs[:, :, k]
        ok = ~np.isnan(r)
        gap = np.max(np.abs(g[ok] - r[ok]), initial=0.0) / (1.0 + np.max(np.abs(r[ok]), initial=0.0))
        print(f"GAP {tag} stat {k}: {gap:.2e}")
        if k == 2:
            assert np.array_equal(g[ok], r[ok]), (tag, "max_row")
        assert gap <= 1e-9, (tag, k, gap)
        worst = max(worst, gap)
    if rb is not None or gb is not None:
        assert gb is not None and rb is not None and gb.shape == rb.shape and gb.dtype == np.uint32, tag
        print(f"GAP {tag} row_below: {int(np.max(np.abs(gb.astype(np.int64) - rb.astype(np.int64)), initial=0))}")
        assert np.array_equal(gb, rb), (tag, "row_below")
    return worst
