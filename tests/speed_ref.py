"""numpy restatement of ssde_path_speed for the tests (test infrastructure): the definition and nothing else, on
an array of draws -- those of tests/draws_ref.py, of the host twin, or a GPU's own.

* A track's state rows are rows first + 1 .. last of `seg_start`'s segments.
* Velocity columns: state column 2a + 1 of a CTCRW's response column a.  Speed s = |v_1| (d = 1), sqrt(v_1^2 + v_2^2) (d = 2).
* Statistic 0: sum_j w_j s_j.  1: max_j s_j.  2: the row (of the data, 0-based) attaining it, the smallest on a tie.  3, 4: the
  resultant sum_j w_j v_jc / s_j, rows with s_j = 0 adding nothing (4 is 0 for d = 1).  5 + r: sum_j w_j 1[s_j <= thr_r].
* NaN in every statistic of a track without a state row, and of a (track, draw) with a non-finite velocity on a state row.
* row_below[j, r]: the number of draws with a finite s_j <= thr_r; 0 on rows without a state.
"""
from __future__ import annotations

import numpy as np


def velocity_columns(d):
    return [2 * a + 1 for a in range(d)]


def speeds(draws, d):
    """(n_draws, n): the speed at every row (also rows without a state, where the draws hold NaN)"""
    v = np.asarray(draws, dtype=np.float64)[:, :, velocity_columns(d)]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(v[:, :, 0]) if d == 1 else np.sqrt((v ** 2).sum(axis=2))


def state_rows(seg_start, n):
    """True on rows first + 1 .. last of every track"""
    has = np.ones(n, dtype=bool)
    has[np.asarray(seg_start, dtype=np.int64)] = False
    return has


def speed_ref(draws, seg_start, d, thresholds=None, weight=None):
    """(stats (n_draws, n_tracks, 5 + n_thr), row_below (n, n_thr) uint32) from draws (n_draws, n, 2 d) of a CTCRW"""
    draws = np.asarray(draws, dtype=np.float64)
    nd, n, sd = draws.shape
    assert sd == 2 * d and d in (1, 2)
    thr = np.zeros(0) if thresholds is None else np.asarray(thresholds, dtype=np.float64).ravel()
    w = np.ones(n) if weight is None else np.asarray(weight, dtype=np.float64)
    bounds = np.r_[np.asarray(seg_start, dtype=np.int64), n]
    out = np.full((nd, len(bounds) - 1, 5 + len(thr)), np.nan)
    below = np.zeros((n, len(thr)), dtype=np.uint32)
    s_all = speeds(draws, d)
    for k in range(len(bounds) - 1):
        rows = np.arange(bounds[k] + 1, bounds[k + 1])
        if len(rows) == 0:
            continue
        v = draws[:, rows][:, :, velocity_columns(d)]                      # n_draws x m x d
        s = s_all[:, rows]
        wr = w[rows][None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, k, 0] = (wr * s).sum(axis=1)
            out[:, k, 1] = s.max(axis=1)
            out[:, k, 2] = rows[np.argmax(np.where(np.isnan(s), -1.0, s), axis=1)]          # the first of equal maxima: the smallest row
            unit = np.where((s > 0)[:, :, None], v / s[:, :, None], 0.0)
            out[:, k, 3] = (wr * unit[:, :, 0]).sum(axis=1)
            out[:, k, 4] = (wr * unit[:, :, 1]).sum(axis=1) if d == 2 else 0.0
            for r in range(len(thr)):
                at = np.isfinite(s) & (s <= thr[r])
                out[:, k, 5 + r] = np.where(at, wr, 0.0).sum(axis=1)
                below[rows, r] = at.sum(axis=0)
        out[~np.isfinite(v).all(axis=(1, 2)), k, :] = np.nan
    return out, below
