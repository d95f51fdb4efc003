"""numpy restatement of ssde_path_stats for the tests (test infrastructure): the definition and nothing else, on
an array of draws -- those of tests/draws_ref.py, of the host twin, or a GPU's own.

* A track's state rows are rows first + 1 .. last of `seg_start`'s segments.
* Position columns: state column 2a of a CTCRW, a otherwise.
* Statistic 0: the sum over consecutive state rows of the Euclidean distance between their positions (|dp| for d = 1; 0 for one
  row).  Statistic 1: the distance between the positions at the last and the first state row.  Statistic 2 + r: the sum over state
  rows of w_j where lo_c <= p_jc < hi_c for every position column c of region r = (lo_1, hi_1, lo_2, hi_2); a weight is added where
  the row is inside and nowhere else.
* NaN in every statistic of a track without a state row, and of a (track, draw) with a non-finite position on a state row.
"""
from __future__ import annotations

import numpy as np


def position_columns(model, d):
    return [2 * a for a in range(d)] if model == "CTCRW" else list(range(d))


def path_ref(draws, seg_start, model, d, regions=None, weight=None):
    """(n_draws, n_tracks, 2 + n_regions) from draws (n_draws, n, sdim)"""
    draws = np.asarray(draws, dtype=np.float64)
    nd, n, _ = draws.shape
    cols = position_columns(model, d)
    reg = np.zeros((0, 4)) if regions is None else np.asarray(regions, dtype=np.float64).reshape(-1, 4)
    w = np.ones(n) if weight is None else np.asarray(weight, dtype=np.float64)
    bounds = np.r_[np.asarray(seg_start, dtype=np.int64), n]
    out = np.full((nd, len(bounds) - 1, 2 + len(reg)), np.nan)
    for k in range(len(bounds) - 1):
        rows = np.arange(bounds[k] + 1, bounds[k + 1])
        if len(rows) == 0:
            continue
        p = draws[:, rows][:, :, cols]                                    # n_draws x m x d
        with np.errstate(invalid="ignore"):
            dp, net = np.diff(p, axis=1), p[:, -1] - p[:, 0]
            if d == 1:
                out[:, k, 0] = np.abs(dp[:, :, 0]).sum(axis=1)
                out[:, k, 1] = np.abs(net[:, 0])
            else:
                out[:, k, 0] = np.sqrt((dp ** 2).sum(axis=2)).sum(axis=1)
                out[:, k, 1] = np.sqrt((net ** 2).sum(axis=1))
            for r in range(len(reg)):
                inside = np.ones(p.shape[:2], dtype=bool)
                for c in range(d):
                    inside &= (reg[r, 2 * c] <= p[:, :, c]) & (p[:, :, c] < reg[r, 2 * c + 1])
                out[:, k, 2 + r] = np.where(inside, w[rows][None, :], 0.0).sum(axis=1)
        out[~np.isfinite(p).all(axis=(1, 2)), k, :] = np.nan
    return out
