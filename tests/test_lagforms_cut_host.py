"""CPU suite: the bulk's forms on the lag statistics of an early cut (ssde_lagstats_host_cut, then ssde_lagforms_host)
against the stationary lanes' own recursion (ssde_tf.hpp: TfCtcrw::step_stat) run row by row in numpy.longdouble over the rows past the
cut:
    dy = y_t - y_{t-1} - mu dt,   w = dy - d1 w_{t-1} - d2 w_{t-2},   u = w - e w_{t-1},   r = w - d1 r_{t-1} - d2 r_{t-2},
    S = sum u^2,   C_k = sum u r_{t-k} (k = 1, 2, 3),   su_a = sum u_a          over t >= cut.
The recursion's three constants are read off the taps the entry returns (the impulse responses of u and r: lam_1 = -d1 - e,
rr_1 = -2 d1, lam_2 = d1^2 - d2 + e d1).  The recursion starts at row 1 of every track and so remembers every row; the forms remember
K.  The parameters are the bench's, whose taps past the K used here sum to less than 1e-15 of the first (asserted below), so the two
agree far inside the tolerance: 1e-12 on the scale the forms' own check uses, max(|sum|, sqrt(|S| n))."""
import numpy as np
import pytest

from smoothsde_amd import capi

from test_lagstats_cut_host import LENGTHS, make_tracks

TOL = 1e-12
# cut -> K: K < cut (the statistics hold the lags below the cut), K >= 16 + ... the check's cut K - 16 is not compared here
CASES = ((32, 24), (64, 48), (128, 112))


def _theta(d, mu):
    return np.array([np.log(0.1)] + [mu * (1.0 - 0.4 * a) for a in range(d)] + [np.log(2.0), 0.0])


def lane_recursion(tracks, cut, e, nd1, nd2, cm):
    """S, C_1..3, su_1, su_2 over the rows t >= cut, the lanes' recursion from row 1 of every track"""
    ld = np.longdouble
    e, nd1, nd2 = ld(e), ld(nd1), ld(nd2)
    out = np.zeros(6, dtype=ld)
    n = 0
    for y in tracks:
        rows, d = y.shape
        if rows <= cut:
            continue
        n += rows - cut
        for a in range(d):
            ya = y[:, a].astype(ld)
            w1 = w2 = r1 = r2 = r3 = ld(0.0)
            for t in range(1, rows):
                dy = (ya[t] - ya[t - 1]) - ld(cm[a])
                w0 = nd1 * w1 + nd2 * w2 + dy
                u = w0 - e * w1
                if t >= cut:
                    out[0] += u * u
                    out[1] += u * r1
                    out[2] += u * r2
                    out[3] += u * r3
                    out[4 + a] += u
                r0 = nd1 * r1 + nd2 * r2 + w0
                r3, r2, r1 = r2, r1, r0
                w2, w1 = w1, w0
    return out, float(n)


@pytest.mark.parametrize("cut,K", CASES)
@pytest.mark.parametrize("mu", [0.0, 0.25])
@pytest.mark.parametrize("d", [1, 2])
def test_forms_on_an_early_cut_match_the_lanes_recursion(d, mu, cut, K):
    tracks = make_tracks(d, 400 + d + cut)
    M, s, n = capi.lagstats_host_cut(tracks, cut)
    assert n == sum(max(0, L - cut) for L in LENGTHS) and K < cut
    theta, dt = _theta(d, mu), 1.0
    f = capi.lagforms_host(M, s, n, theta, dt, K)
    # the recursion's constants from the long impulse responses, and the precondition: nothing is left past K taps
    long_taps = capi.lagforms_host(M, s, n, theta, dt, M.shape[0] - 1)["taps"]
    lam, rr = long_taps
    assert lam[0] == 1.0 and rr[0] == 1.0
    assert np.sum(np.abs(lam[K + 1:])) <= 1e-15 and np.sum(np.abs(rr[K - 2:])) <= 1e-15
    assert np.array_equal(f["taps"][:, :K + 1], long_taps[:, :K + 1])
    nd1 = 0.5 * rr[1]
    e = nd1 - lam[1]
    nd2 = lam[2] - nd1 * nd1 + e * nd1
    ref, nref = lane_recursion(tracks, cut, e, nd1, nd2, theta[1:1 + d] * dt)
    assert nref == n
    for j in range(4 + d):
        sc = max(abs(float(ref[j])), np.sqrt(abs(float(ref[0])) * n))
        err = abs(float(np.longdouble(f["raw"][0, j]) - ref[j])) / sc
        print("d=%d mu=%g cut=%d K=%d sum %d: %.3e" % (d, mu, cut, K, j, err))
        assert err <= TOL, (j, err, f["raw"][0, j], float(ref[j]))
    if d == 1:
        assert f["raw"][0, 5] == 0.0
    assert np.isfinite(f["chk"]) and f["acc"][0] > 0.0


def test_the_forms_of_cut_and_late_statistics_differ_by_the_head_rows():
    """the same theta and K on the statistics of cut 64 and of row 256: the raw sums differ by the lanes' sums over rows [64, 256)"""
    d, cut, K = 2, 64, 48
    tracks = make_tracks(d, 77, lengths=(300, 517, 256, 640, 100, 40))
    theta = _theta(d, 0.25)
    Ml, sl, nl, A = capi.lagstats_host(tracks)
    Mc, sc_, nc = capi.lagstats_host_cut(tracks, cut)
    fl, fc = capi.lagforms_host(Ml, sl, nl, theta, 1.0, K), capi.lagforms_host(Mc, sc_, nc, theta, 1.0, K)
    lam, rr = capi.lagforms_host(Ml, sl, nl, theta, 1.0, Ml.shape[0] - 1)["taps"]
    nd1 = 0.5 * rr[1]
    e = nd1 - lam[1]
    nd2 = lam[2] - nd1 * nd1 + e * nd1
    head, nh = lane_recursion([t[:A] for t in tracks], cut, e, nd1, nd2, theta[1:1 + d])
    assert nc == nl + nh
    for j in range(4 + d):
        scale = max(abs(fc["raw"][0, j]), np.sqrt(abs(fc["raw"][0, 0]) * nc))
        assert abs(float(np.longdouble(fc["raw"][0, j]) - np.longdouble(fl["raw"][0, j]) - head[j])) <= TOL * scale, j
