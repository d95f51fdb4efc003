"""CPU suite: the bulk's forms of one evaluation on the lag-statistics path (ssde_lagforms.hpp through
ssde_lagforms_host) -- the raw sums S = sum u^2, C_k = sum u r_{t-k}, su_a = sum u_a that an evaluation forms from M, s and n on the
host -- against the direct sum over tracks and bulk rows of the same signals, built in numpy.longdouble by convolving the increments
with the taps the entry returns.

Tolerance: 1e-12 on the scale the forms' own check uses, max(|sum|, sqrt(|S| n)) -- the figure tests/test_gpu_lagstats.py holds M
to.  A plain float64 convolution is first shown to meet that bound against the longdouble one on these inputs (otherwise the inputs,
not the code, would be what the bound measures)."""
import numpy as np
import pytest

from smoothsde_amd import capi

TOL = 1e-12
LENGTHS = [300, 517, 900, 256, 640, 431]          # one track without a bulk (<= the bulk's first row)


def _tracks(d, seed):
    rng = np.random.default_rng(seed)
    out = []
    for L in LENGTHS:
        steps = rng.standard_normal((L, d)) + 0.3           # a drift: positions wander, increments stay O(1)
        out.append(np.cumsum(steps, axis=0) + 20.0)
    return out


def _theta(d, mu):
    return np.array([np.log(0.1)] + [mu * (1.0 - 0.4 * a) for a in range(d)] + [np.log(2.0), 0.0])


def _direct(tracks, taps, K, cm, A, dtype):
    """S, C_1..3, su_1, su_2 over the rows t >= A of every track, with the taps 0..K: u_t = sum_i lam_i dy_{t-i},
    r_{t-k} = sum_{i >= k} rr_{i-k} dy_{t-i}, dy_t = y_t - y_{t-1} - mu dt."""
    lam, rr = taps[0].astype(dtype), taps[1].astype(dtype)
    out = np.zeros(6, dtype=dtype)
    n = 0
    for y in tracks:
        rows, d = y.shape
        if rows <= A:
            continue
        n += rows - A
        for a in range(d):
            dy = np.zeros(rows, dtype=dtype)
            dy[1:] = y[1:, a].astype(dtype) - y[:-1, a].astype(dtype) - dtype(cm[a])
            t = np.arange(A, rows)
            u = np.zeros(len(t), dtype=dtype)
            r = np.zeros((3, len(t)), dtype=dtype)
            for i in range(K + 1):
                w = dy[t - i]
                u += lam[i] * w
                for k in range(1, 4):
                    if i >= k:
                        r[k - 1] += rr[i - k] * w
            out[0] += np.sum(u * u)
            for k in range(3):
                out[1 + k] += np.sum(u * r[k])
            out[4 + a] += np.sum(u)
    return out, float(n)


def _scale(x, S, n):
    return max(abs(float(x)), np.sqrt(abs(float(S)) * n))


@pytest.mark.parametrize("K", [16, 48, 191])
@pytest.mark.parametrize("mu", [0.0, 0.25])
@pytest.mark.parametrize("d", [1, 2])
def test_forms_match_the_direct_sums_over_the_bulk_rows(d, mu, K):
    tracks = _tracks(d, 31 + d)
    M, s, n, A = capi.lagstats_host(tracks)
    assert n == sum(max(0, L - A) for L in LENGTHS) and min(LENGTHS) <= A
    # the track without a bulk contributes nothing
    M2, s2, n2, _ = capi.lagstats_host([y for y in tracks if y.shape[0] > A])
    assert n2 == n and np.array_equal(M, M2) and np.array_equal(s, s2)
    theta, dt = _theta(d, mu), 1.0
    f = capi.lagforms_host(M, s, n, theta, dt, K)
    taps = f["taps"]
    assert taps.shape == (2, M.shape[0]) and np.all(taps[:, K + 1:] == 0.0) and taps[0, 0] != 0.0
    cm = theta[1:1 + d] * dt
    for cut, Kc in enumerate((K, K - 16)):
        ref, nref = _direct(tracks, taps, Kc, cm, A, np.longdouble)
        assert nref == n
        # the inputs are well enough conditioned for the bound: plain float64 sums meet it
        ref64, _ = _direct(tracks, taps, Kc, cm, A, np.float64)
        for j in range(4 + d):
            e64 = abs(float(ref64[j] - ref[j])) / _scale(ref[j], ref[0], n)
            assert e64 <= TOL, ("float64 convolution", cut, j, e64)
        for j in range(4 + d):
            err = abs(float(np.longdouble(f["raw"][cut, j]) - ref[j])) / _scale(ref[j], ref[0], n)
            print("d=%d mu=%g K=%d cut=%d sum %d: %.3e" % (d, mu, K, Kc, j, err))
            assert err <= TOL, (cut, j, err, f["raw"][cut, j], float(ref[j]))
        if d == 1:
            assert f["raw"][cut, 5] == 0.0
    # the two cuts differ by no more than the check value says, on its scale
    S = f["raw"][0, 0]
    for j in range(4 + d):
        a, b = f["raw"][0, j], f["raw"][1, j]
        sc = max(abs(a), abs(b), np.sqrt(abs(S) * n))
        assert abs(a - b) <= f["chk"] * sc * (1.0 + 1e-14), (j, a, b, f["chk"])
    assert np.isfinite(f["chk"])
    # the accumulators: the value is 0.5 iF S (iF > 0, S > 0), and mu's directions are -iF c su_a with one constant c for both
    # coordinates: proportional to the raw sums su_a
    acc, su = f["acc"], f["raw"][0, 4:4 + d]
    assert acc.shape == (4 + d,) and acc[0] > 0.0 and S > 0.0
    assert np.all(acc[2:2 + d] != 0.0) and np.all(acc[[1, 2 + d, 3 + d]] != 0.0)
    if d == 2:
        assert abs(acc[2] * su[1] - acc[3] * su[0]) <= 1e-14 * abs(acc[2] * su[1])


@pytest.mark.parametrize("K", [16, 48, 191])
def test_taps_beyond_the_cut_are_never_read(K):
    d = 2
    tracks = _tracks(d, 77)
    M, s, n, _ = capi.lagstats_host(tracks)
    theta = _theta(d, 0.25)
    f = capi.lagforms_host(M, s, n, theta, 1.0, K)
    g = capi.lagforms_host(M, s, n, theta, 1.0, K, taps=f["taps"])
    assert np.array_equal(f["raw"], g["raw"]) and np.array_equal(f["acc"], g["acc"]) and f["chk"] == g["chk"]
    junk = f["taps"].copy()
    junk[:, K + 1:] = 1e30 * (1.0 + np.random.default_rng(5).random(junk[:, K + 1:].shape))
    h = capi.lagforms_host(M, s, n, theta, 1.0, K, taps=junk)
    assert np.array_equal(f["raw"], h["raw"]) and np.array_equal(f["acc"], h["acc"]) and f["chk"] == h["chk"]


def test_arguments_out_of_range_are_refused():
    tracks = _tracks(1, 3)
    M, s, n, _ = capi.lagstats_host(tracks)
    for K in (15, M.shape[0]):
        with pytest.raises(ValueError):
            capi.lagforms_host(M, s, n, _theta(1, 0.0), 1.0, K)
