"""Regions and weights shared by the tests of ssde_path_stats (test infrastructure).

Region edges must not sit on a drawn position, or a 1e-15 difference between two implementations would flip a count: per position
column the edges are np.round(np.quantile(obs[:, a], [.25, .75]), 3) + 5e-4, further boxes are those shifted by whole units, one
region is a half-plane with infinite bounds, and clear_of_edges() is the precondition every comparison asserts on its reference
draws: every finite drawn coordinate is more than 1e-5 from every finite edge."""
import numpy as np

from path_ref import position_columns

# whole-unit shifts of the base box, (column 1, column 2), for regions 2 ... 7
_SHIFTS = [(3.0, -2.0), (-4.0, 1.0), (7.0, 7.0), (-1.0, -6.0), (12.0, 0.0), (0.0, 15.0)]


def base_edges(obs, d):
    """(d, 2): lo, hi per position column"""
    e = np.empty((d, 2))
    for a in range(d):
        col = np.asarray(obs)[:, a]
        e[a] = np.round(np.quantile(col[~np.isnan(col)], [.25, .75]), 3) + 5e-4
    return e


def make_regions(obs, d, n_regions):
    """(n_regions, 4) rows of lo_1, hi_1, lo_2, hi_2: the quantile box, a half-plane (column 1 below its upper edge), shifted boxes.
    For d = 1 the second pair holds lo > hi on purpose: it must not be read."""
    e = base_edges(obs, d)
    second = lambda s: [e[1, 0] + s, e[1, 1] + s] if d == 2 else [1.0, -1.0]
    reg = [[e[0, 0], e[0, 1]] + second(0.0), [-np.inf, e[0, 1]] + ([-np.inf, np.inf] if d == 2 else [1.0, -1.0])]
    reg += [[e[0, 0] + s1, e[0, 1] + s1] + second(s2) for s1, s2 in _SHIFTS]
    return np.array(reg[:n_regions], dtype=np.float64).reshape(n_regions, 4)


def edge_distance(draws, model, d, regions):
    """the smallest distance of a finite drawn position coordinate to a finite edge of its column"""
    best = np.inf
    reg = np.asarray(regions, dtype=np.float64).reshape(-1, 4)
    for c, col in enumerate(position_columns(model, d)):
        p = draws[:, :, col]
        p = p[np.isfinite(p)]
        for edge in np.unique(reg[:, 2 * c:2 * c + 2]):
            if np.isfinite(edge) and p.size:
                best = min(best, np.min(np.abs(p - edge)))
    return best


def clear_of_edges(draws, model, d, regions):
    return edge_distance(draws, model, d, regions) > 1e-5


def dt_weights(seg_start, times):
    """the time from a row to the track's next row, 0 at a track's last row"""
    times = np.asarray(times, dtype=np.float64)
    w = np.r_[np.diff(times), 0.0]
    w[np.asarray(seg_start, dtype=np.int64)[1:] - 1] = 0.0
    return w


def compare(got, ref, tag):
    """|got - ref| <= 1e-9 (1 + max|ref|) per statistic, identical NaN patterns; returns the largest gap"""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), tag
    worst = 0.0
    for k in range(ref.shape[2]):
        g, r = got[:, :, k], ref[:, :, k]
        ok = ~np.isnan(r)
        gap = np.max(np.abs(g[ok] - r[ok]), initial=0.0) / (1.0 + np.max(np.abs(r[ok]), initial=0.0))
        print(f"GAP {tag} stat {k}: {gap:.2e}")
        assert gap <= 1e-9, (tag, k, gap)
        worst = max(worst, gap)
    return worst
