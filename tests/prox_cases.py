"""Shared by the proximity suites (test_prox_hostsim.py, test_gpu_prox.py): the points of the calls, the radii, and the statistical
case.  A point is a pair of ssde_predict_draws queries; nothing requires the two sides of a point to share a clock time, so most
cases draw the two sides' rows and offsets independently, which reaches more (row, offset) patterns than common times would."""
import numpy as np

from predict_cases import intervals

RADII = [0.37, 1.3, np.inf]
RADII8 = [0.0, 0.11, 0.37, 0.9, 1.3, 2.9, 7.1, np.inf]
EDGE_SIZES = [0, 1, 255, 256, 257, 600]             # pairs of one call: empty, one point, around a tile, three tiles


def track_of_row(pb, rows):
    return np.searchsorted(np.asarray(pb.seg_start), np.asarray(rows), side="right") - 1


def side_queries(pb, n, rng, tracks=None, forecast=0.0):
    """n queries with a state: interior rows (of `tracks`, or of every track) at a uniform offset inside their interval; a share
    `forecast` of them on a last row instead, up to 3 past it"""
    first, last, dt = intervals(pb)
    trk = track_of_row(pb, np.arange(pb.n))
    mine = np.ones(pb.n, dtype=bool) if tracks is None else np.isin(trk, np.asarray(tracks))
    inner, ends = np.flatnonzero(mine & ~first & ~last), np.flatnonzero(mine & ~first & last)
    rows = rng.choice(inner, n)
    offs = rng.uniform(0.0, 1.0, n) * dt[rows]
    if forecast > 0.0 and len(ends):
        f = rng.uniform(0.0, 1.0, n) < forecast
        rows[f] = rng.choice(ends, int(f.sum()))
        offs[f] = rng.uniform(0.0, 3.0, int(f.sum()))
    return rows.astype(np.int64), offs


def points(pb, sizes, seed, tracks_a=None, tracks_b=None, forecast=0.0, near=0.5):
    """(qa_rows, qa_offs, qb_rows, qb_offs, pair_ptr): pairs of the given sizes.  The test tracks lie far apart, so a share `near` of
    the points takes side B in side A's own interval at a smaller offset: those distances are of the size of the radii, the others
    are far outside every finite one."""
    rng = np.random.default_rng(seed)
    n = int(np.sum(sizes))
    ra, oa = side_queries(pb, n, rng, tracks_a, forecast)
    rb, ob = side_queries(pb, n, rng, tracks_b, forecast)
    close = rng.uniform(0.0, 1.0, n) < near
    rb[close] = ra[close]
    ob[close] = oa[close] * rng.uniform(0.0, 1.0, int(close.sum()))
    return ra, oa, rb, ob, np.r_[0, np.cumsum(sizes)].astype(np.int64)


def concat(ra, oa, rb, ob):
    """the one call of predict_draws whose states the proximity call pairs: all the A queries, then all the B queries"""
    return np.r_[ra, rb], np.r_[oa, ob]


# ---- the statistical check: two tracks, one common time, 512 draws ----
STAT_SEED, STAT_DRAWS = 7, 512


def stat_problem():
    """two CTCRW tracks of 12 rows (d = 2) and one clock time inside both"""
    from smoothsde_amd import capi
    from smoothsde_amd.synth import simulate
    ID, times, obs = simulate("CTCRW", 2, 12, 2, seed=23)
    times[12:] = times[:12] + 0.25                      # the second track on the first one's clock, a quarter step later
    pb = capi.Problem("CTCRW", ID, times, obs)
    par = np.array([-1.0, 0.05, -0.05, 0.4, 0.1])
    t = np.asarray(pb.times, dtype=np.float64)
    ta, tb = t[:12], t[12:]
    clock = 0.5 * (max(ta[1], tb[1]) + min(ta[-1], tb[-1])) + 0.0137          # inside both tracks, on no time stamp
    ja, jb = int(np.searchsorted(ta, clock, side="right")) - 1, int(np.searchsorted(tb, clock, side="right")) - 1
    assert 1 <= ja < 11 and 1 <= jb < 11 and ta[ja] < clock < ta[ja + 1] and tb[jb] < clock < tb[jb + 1]
    rows = np.array([ja, 12 + jb], dtype=np.int64)
    return pb, par, rows, clock - t[rows]


def stat_ratio(min_dist, mean, cov, z=(0, 2)):
    """|mean over the draws of dist^2 - (|m_a - m_b|^2 + tr(V_a + V_b))| in standard errors of that Monte Carlo mean (estimated from the
    draws); mean (2, sdim) and cov (2, sdim, sdim) from predict at the two queries, z the position columns"""
    z = list(z)
    d2 = np.asarray(min_dist, dtype=np.float64) ** 2
    want = float(np.sum((mean[0, z] - mean[1, z]) ** 2) + sum(cov[k][c, c] for k in (0, 1) for c in z))
    se = float(np.std(d2, ddof=1) / np.sqrt(len(d2)))
    return abs(float(d2.mean()) - want) / se
