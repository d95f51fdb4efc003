"""CPU suite: the lag statistics of the stationary bulk -- the Toeplitz lag sums plus the corrections at the
bulk's two ends, assembled into M (ssde_lagstats.hpp: lag_assemble), and the telescoped s -- against a direct NumPy loop over
the bulk rows, on small ragged tracks (some too short to have a bulk)."""
import numpy as np
import pytest

from smoothsde_amd import capi


def _direct(tracks, N, A):
    M = np.zeros((N, N))
    s = np.zeros((2, N))
    n = 0.0
    lags = np.arange(N)
    for y in tracks:
        rows, d = y.shape
        if rows <= A:
            continue
        Dy = np.full_like(y, np.nan)
        Dy[1:] = y[1:] - y[:-1]
        for t in range(A, rows):
            w = Dy[t - lags]                     # (N, d): Dy_{t-i}
            M += w @ w.T
            s[:d] += w.T
            n += 1.0
    return M, s, n


@pytest.mark.parametrize("d", [1, 2])
def test_lag_statistics_match_a_direct_loop_on_ragged_tracks(d):
    rng = np.random.default_rng(11 + d)
    _, _, _, A = capi.lagstats_host([np.zeros((1, d))])
    lengths = [A + 1, A + 37, 2 * A + 5, A - 10, 3 * A, A, 700]
    tracks = []
    for L in lengths:
        steps = rng.standard_normal((L, d)) + 0.3           # a drift: positions wander far from 0, increments stay O(1)
        tracks.append(np.cumsum(steps, axis=0) + 50.0)
    M, s, n, A = capi.lagstats_host(tracks)
    N = M.shape[0]
    Md, sd, nd = _direct(tracks, N, A)
    assert n == nd == sum(max(0, L - A) for L in lengths)
    assert np.max(np.abs(M - Md)) <= 1e-13 * np.max(np.abs(Md)), np.max(np.abs(M - Md)) / np.max(np.abs(Md))
    assert np.array_equal(M, M.T)
    assert np.max(np.abs(s - sd)) <= 1e-13 * np.max(np.abs(sd))
    if d == 1:
        assert np.all(s[1] == 0.0)


def test_no_bulk_without_rows_past_the_first_bulk_row():
    _, _, _, A = capi.lagstats_host([np.zeros((1, 2))])
    M, s, n, _ = capi.lagstats_host([np.ones((A, 2)), np.ones((10, 2))])
    assert n == 0.0 and not M.any() and not s.any()
