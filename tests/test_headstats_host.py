"""CPU suite: the Gram statistics of the lag-path head's rows (ssde_headforms.hpp: head_track_stats, through
ssde_headstats_host) against direct sums in numpy.longdouble: per track and coordinate w = (x0 - y_0, v0, the increments of rows
1 .. 127), G = sum w w' over tracks and coordinates, s_a = sum w per coordinate, n = the tracks.  Bound: 1e-12 of the largest entry,
the bound of the lag statistics' tests.  A batch with a track shorter than the statistics' 128 rows reports "not built"."""
import numpy as np
import pytest

from smoothsde_amd import capi

ROWS = 300
C = 128


def make_batch(n_tracks, seed, rows=ROWS):
    rng = np.random.default_rng(seed)
    lengths = [rows] * n_tracks if np.isscalar(rows) else list(rows)
    # a drift: positions wander far from 0, increments stay O(1); a0 near the first row with a velocity of its own
    tracks = [np.cumsum(rng.standard_normal((L, 2)) + 0.3, axis=0) + 50.0 for L in lengths]
    a0 = np.stack([np.array([t[0, 0] + 0.2, 0.4, t[0, 1] - 0.1, -0.3]) + 0.05 * rng.standard_normal(4) for t in tracks])
    return tracks, a0


def direct(tracks, a0, nw):
    G = np.zeros((nw, nw), dtype=np.longdouble)
    s = np.zeros((2, nw), dtype=np.longdouble)
    for y, a in zip(tracks, a0):
        y = y.astype(np.longdouble)
        a = a.astype(np.longdouble)
        for c in range(2):
            w = np.zeros(nw, dtype=np.longdouble)
            w[0] = a[2 * c] - y[0, c]
            w[1] = a[2 * c + 1]
            w[2:] = y[1:C, c] - y[0:C - 1, c]
            G += np.outer(w, w)
            s[c] += w
    return G, s


@pytest.mark.parametrize("n_tracks", [3, 70])
def test_the_host_reference_matches_direct_longdouble_sums(n_tracks):
    nw = capi.head_components()
    assert nw == C + 1
    tracks, a0 = make_batch(n_tracks, 40 + n_tracks)
    got = capi.headstats_host(tracks, a0)
    assert got is not None
    G, s, n = got
    Gd, sd = direct(tracks, a0, nw)
    assert n == n_tracks
    gap_G = float(np.max(np.abs(G - Gd))) / float(np.max(np.abs(Gd)))
    gap_s = float(np.max(np.abs(s - sd))) / float(np.max(np.abs(sd)))
    print("tracks %d: G %.2e s %.2e" % (n_tracks, gap_G, gap_s))
    assert gap_G <= 1e-12 and gap_s <= 1e-12
    assert np.array_equal(G, G.T)
    # rows past the statistics' do not enter
    longer = [np.vstack([t, t[-1:] + 7.0]) for t in tracks]
    G2, s2, n2 = capi.headstats_host(longer, a0)
    assert np.array_equal(G2, G) and np.array_equal(s2, s) and n2 == n


def test_a_track_shorter_than_the_statistics_rows_reports_not_built():
    tracks, a0 = make_batch(4, 7, rows=(300, 100, 300, 128))
    assert capi.headstats_host(tracks, a0) is None
    # ... and exactly 128 rows are enough
    tracks, a0 = make_batch(3, 8, rows=(128, 300, 129))
    got = capi.headstats_host(tracks, a0)
    assert got is not None and got[2] == 3
    Gd, sd = direct(tracks, a0, capi.head_components())
    assert float(np.max(np.abs(got[0] - Gd))) <= 1e-12 * float(np.max(np.abs(Gd)))
