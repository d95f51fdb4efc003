"""CPU suite: the lag statistics at the early cuts (ssde_lagstats.hpp: lag_track_stats_cut, lag_assemble_cut, through
ssde_lagstats_host_cut) against direct sums in numpy.longdouble over the rows past the cut: M_ik = sum_{t >= cut} Dy_{t-i} Dy_{t-k} and
s_{a,i} = sum_{t >= cut} Dy_{a,t-i} for the lags i, k < cut, zeros elsewhere; a track of n <= cut rows contributes nothing."""
import numpy as np
import pytest

from smoothsde_amd import capi

LENGTHS = (31, 32, 33, 63, 64, 65, 256, 257, 300)
CUTS = (32, 64, 128)


def direct_cut(tracks, N, cut):
    """(M, s, n) by a loop over the bulk rows, in longdouble"""
    M = np.zeros((N, N), dtype=np.longdouble)
    s = np.zeros((2, N), dtype=np.longdouble)
    n = 0
    lags = np.arange(min(cut, N))
    for y in tracks:
        rows, d = y.shape
        if rows <= cut:
            continue
        y = y.astype(np.longdouble)
        Dy = np.zeros_like(y)
        Dy[1:] = y[1:] - y[:-1]
        for t in range(cut, rows):
            w = Dy[t - lags]                     # (lags, d): Dy_{t-i}; t - i >= 1
            M[:len(lags), :len(lags)] += w @ w.T
            s[:d, :len(lags)] += w.T
            n += 1
    return M, s, n


def make_tracks(d, seed, lengths=LENGTHS):
    rng = np.random.default_rng(seed)
    # a drift: positions wander far from 0, increments stay O(1)
    return [np.cumsum(rng.standard_normal((L, d)) + 0.3, axis=0) + 50.0 for L in lengths]


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("cut", CUTS)
def test_the_host_reference_matches_direct_longdouble_sums(d, cut):
    tracks = make_tracks(d, 100 + 7 * d + cut)
    M, s, n = capi.lagstats_host_cut(tracks, cut)
    N = M.shape[0]
    Md, sd, nd = direct_cut(tracks, N, cut)
    assert n == nd == sum(max(0, L - cut) for L in LENGTHS)
    big = float(np.max(np.abs(Md)))
    assert float(np.max(np.abs(M - Md))) <= 1e-12 * big, float(np.max(np.abs(M - Md))) / big
    assert np.array_equal(M, M.T)
    assert not M[cut:, :].any() and not M[:, cut:].any() and not s[:, cut:].any()
    assert float(np.max(np.abs(s - sd))) <= 1e-12 * float(np.max(np.abs(sd)))
    if d == 1:
        assert np.all(s[1] == 0.0)


@pytest.mark.parametrize("cut", CUTS)
def test_every_length_on_its_own(cut):
    """one track per batch: the lengths at and around the cut (no bulk, one bulk row) and around row 256"""
    for L in LENGTHS:
        tracks = make_tracks(2, 5000 + L, lengths=(L,))
        M, s, n = capi.lagstats_host_cut(tracks, cut)
        Md, sd, nd = direct_cut(tracks, M.shape[0], cut)
        assert n == nd == max(0, L - cut)
        if L <= cut:
            assert not M.any() and not s.any()
            continue
        assert float(np.max(np.abs(M - Md))) <= 1e-12 * float(np.max(np.abs(Md))), (L, cut)
        assert float(np.max(np.abs(s - sd))) <= 1e-12 * float(np.max(np.abs(sd))), (L, cut)


def test_the_late_cut_is_the_late_statistics_and_other_cuts_are_refused():
    tracks = make_tracks(2, 9)
    M0, s0, n0, A = capi.lagstats_host(tracks)
    M, s, n = capi.lagstats_host_cut(tracks, A)
    assert np.array_equal(M, M0) and np.array_equal(s, s0) and n == n0
    for cut in (0, 16, 40, 144, 255):
        with pytest.raises(ValueError):
            capi.lagstats_host_cut(tracks, cut)


def test_an_early_cut_is_the_late_statistics_plus_the_head_rows():
    """what the device pass builds: M(cut) = M(256) + the statistics of the tracks cut off after 256 rows, on the lags below the cut"""
    tracks = make_tracks(2, 17, lengths=(300, 700, 257, 256, 100, 40))
    _, _, _, A = capi.lagstats_host(tracks)
    Ml, sl, nl, _ = capi.lagstats_host(tracks)
    for cut in capi.LAG_CUTS:
        M, s, n = capi.lagstats_host_cut(tracks, cut)
        Mh, sh, nh = capi.lagstats_host_cut([t[:A] for t in tracks], cut)
        assert n == nl + nh
        big = np.max(np.abs(M))
        assert np.max(np.abs(M[:cut, :cut] - (Ml[:cut, :cut] + Mh[:cut, :cut]))) <= 1e-12 * big
        assert np.max(np.abs(s[:, :cut] - (sl[:, :cut] + sh[:, :cut]))) <= 1e-12 * np.max(np.abs(s))
