"""CPU suite: the lag statistics of the three models the lag-statistics path serves, through ssde_lagstats_host_m.

OU_SSM takes the statistics of the LEVELS z = y - ref: M_ik = sum z_{t-i} z_{t-k} (over tracks, bulk rows and coordinates) and
s_{a,i} = sum z_{a,t-i}, here against direct numpy.longdouble sums, every one of the 192 lags, to 1e-12 of max|M| and max|s| (the
figure tests/test_gpu_lagstats.py holds the device's statistics to).  CTCRW and BM_SSM take those of the increments: bitwise what
ssde_lagstats_host returns."""
import numpy as np
import pytest

from smoothsde_amd import capi

TOL = 1e-12
LENGTHS = [300, 517, 256, 900, 120, 640, 431, 257]          # three tracks without a bulk (<= the bulk's first row), one with one bulk row


def _tracks(d, seed):
    """levels that stay within a few standard deviations of 20 (an AR(1) around it, observed with noise)"""
    rng = np.random.default_rng(seed)
    out = []
    for L in LENGTHS:
        x = np.zeros((L, d))
        e = rng.standard_normal((L, d))
        for t in range(1, L):
            x[t] = 0.6 * x[t - 1] + 0.8 * e[t]
        out.append(20.0 + x + 0.1 * rng.standard_normal((L, d)))
    return out


def _direct_levels(tracks, ref, A, n_taps):
    LD = np.longdouble
    d = tracks[0].shape[1]
    M = np.zeros((n_taps, n_taps), dtype=LD)
    s = np.zeros((2, n_taps), dtype=LD)
    n = 0
    for y in tracks:
        rows = y.shape[0]
        if rows <= A:
            continue
        n += rows - A
        t = np.arange(A, rows)
        for a in range(d):
            z = y[:, a].astype(LD) - LD(ref[a])
            Z = np.stack([z[t - i] for i in range(n_taps)], axis=1)          # Z[t, i] = z_{t-i}
            M += Z.T @ Z
            s[a] += Z.sum(axis=0)
    return M, s, n


@pytest.mark.parametrize("d", [1, 2])
def test_ou_ssm_level_statistics_match_direct_longdouble_sums(d):
    tracks = _tracks(d, 40 + d)
    _, _, _, A = capi.lagstats_host([np.zeros((1, d))])
    first = next(y for y in tracks if y.shape[0] > A)
    ref = first[A - 1].copy()                                  # one observation: what a handle centres its levels on
    M, s, n, A2 = capi.lagstats_host(tracks, model="OU_SSM", ref=ref)
    n_taps = M.shape[0]
    assert A2 == A == 256 and n_taps == 192
    assert sum(1 for L in LENGTHS if L <= A) >= 2
    Mr, sr, nr = _direct_levels(tracks, ref, A, n_taps)
    assert n == nr == sum(max(0, L - A) for L in LENGTHS)
    eM = float(np.max(np.abs(M.astype(np.longdouble) - Mr)) / np.max(np.abs(Mr)))
    es = float(np.max(np.abs(s[:d].astype(np.longdouble) - sr[:d])) / np.max(np.abs(sr)))
    print("d=%d: M %.3e  s %.3e" % (d, eM, es))
    assert eM <= TOL and es <= TOL
    assert np.array_equal(M, M.T)
    if d == 1:
        assert np.all(s[1] == 0.0)
    # tracks without a bulk contribute nothing
    M2, s2, n2, _ = capi.lagstats_host([y for y in tracks if y.shape[0] > A], model="OU_SSM", ref=ref)
    assert n2 == n and np.array_equal(M, M2) and np.array_equal(s, s2)
    # the statistics are those of the levels: another ref gives other numbers
    M3, _, _, _ = capi.lagstats_host(tracks, model="OU_SSM", ref=ref + 1.0)
    assert not np.array_equal(M, M3)


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("model", ["CTCRW", "BM_SSM"])
def test_increment_models_are_bitwise_the_existing_statistics(model, d):
    tracks = _tracks(d, 50 + d)
    M0, s0, n0, A0 = capi.lagstats_host(tracks)
    for ref in (np.zeros(d), np.full(d, 7.5)):                   # (ref is ignored; passing one routes CTCRW through the new entry too)
        M, s, n, A = capi.lagstats_host(tracks, model=model, ref=ref)
        assert A == A0 and n == n0 and np.array_equal(M, M0) and np.array_equal(s, s0)
    if model == "BM_SSM":
        M, s, n, A = capi.lagstats_host(tracks, model=model)
        assert n == n0 and np.array_equal(M, M0) and np.array_equal(s, s0)


def test_arguments_out_of_range_are_refused():
    tracks = _tracks(1, 3)
    with pytest.raises(ValueError):
        capi.lagstats_host(tracks, model="OU_SSM")               # levels need a ref
    with pytest.raises(ValueError):
        capi.lagstats_host(tracks, model="OU", ref=np.zeros(1))  # a model outside the three
    with pytest.raises(ValueError):
        capi.lagstats_host([np.zeros((300, 3))], model="OU_SSM", ref=np.zeros(3))
