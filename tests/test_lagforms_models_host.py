"""CPU suite: the bulk's forms of OU_SSM and BM_SSM on the lag-statistics path (ssde_lagforms.hpp through
ssde_lagforms_host_m) -- the raw sums S = sum u^2, S1 = sum u A1, S3 = sum u A3, su_a = sum u_a and the accumulators formed from them --
against the stationary lanes' own recursion (ssde_tf.hpp: BasisScal::step_stat), run here row by row in numpy.longdouble over the
bulk rows of every track, with the stationary gain and its sensitivities iterated in longdouble too.

Cuts: the smallest legal one is the warm-up the window plan asks for at that theta, ceil(log 1e-18 / log rho) + 16 rows (rho the
closed-loop factor; ssde_windows.hpp: warmup_rows) -- an evaluation never takes the path with fewer taps, and what a cut K leaves out is
O(rho^K) <= 1e-18 by that rule; then one half-way to the longest, and the longest (191).  The recursion starts 255 >= K + 64 rows
before the bulk, from u = 0.

Tolerance: 1e-12 on the forms' own scale max(|sum|, sqrt(|S| n)), the TOL of tests/test_lagforms_host.py.  An accumulator is a fixed
linear combination of raw sums (BasisScal::finish), so it is held to the same combination of their scales."""
import numpy as np
import pytest

from smoothsde_amd import capi

LD = np.longdouble
TOL = 1e-12
A_ROW = 256
LENGTHS = [300, 517, 900, 256, 640, 431]          # one track without a bulk
DT = 1.0


def _tracks(model, d, seed):
    rng = np.random.default_rng(seed)
    out = []
    for L in LENGTHS:
        if model == "OU_SSM":                       # stationary around 20, process variance ~1
            x = np.zeros((L, d))
            e = rng.standard_normal((L, d))
            for t in range(1, L):
                x[t] = 0.6 * x[t - 1] + 0.8 * e[t]
            out.append(20.0 + x + 0.1 * rng.standard_normal((L, d)))
        else:                                       # a drifting walk: positions wander, increments stay O(1)
            out.append(np.cumsum(0.7 * rng.standard_normal((L, d)) + 0.3, axis=0) + 20.0)
    return out


def _theta(model, d, ratio):
    if model == "OU_SSM":                           # process scale sqrt(kappa) = 1
        mu = [19.6 + 0.7 * a for a in range(d)]
        return np.array([np.log(ratio * 1.0)] + mu + [np.log(2.0), 0.0])
    mu = [0.25 - 0.4 * a for a in range(d)]         # process scale sigma = 0.7
    return np.array([np.log(ratio * 0.7)] + mu + [np.log(0.7)])


def _stationary(model, theta, d):
    """The stationary gain of the scalar filter and its sensitivities (ssde_math.hpp: scal_cov_step, the scored branch), in longdouble."""
    ou = model == "OU_SSM"
    h = np.exp(LD(2.0) * LD(theta[0]))
    if ou:
        tau, kappa = np.exp(LD(theta[1 + d])), np.exp(LD(theta[2 + d]))
        z = LD(DT) / tau
        t = np.exp(-z)
        b, q, dt_, db, dq = 1 - t, kappa * (1 - t * t), t * z, -t * z, -2 * kappa * t * t * z
    else:
        sg = np.exp(LD(theta[1 + d]))
        t, b, q, dt_, db = LD(1), LD(DT), sg * sg * LD(DT), LD(0), LD(0)
        dq = 2 * q
    p, dp = LD(1), np.zeros(3, dtype=LD)
    for _ in range(4000):
        F = p + h
        iF = 1 / F
        a_, b_ = h * iF, p * iF
        c, k = t * a_, t * b_
        diF, dk, ndp = np.zeros(3, dtype=LD), np.zeros(3, dtype=LD), np.zeros(3, dtype=LD)
        for j in range(3):
            if j == 2 and not ou:
                continue
            dF = dp[j] + (2 * h if j == 0 else 0)
            diF[j] = -iF * iF * dF
            dk[j] = t * iF * a_ * dp[j]
            ndp[j] = t * c * a_ * dp[j]
            if j == 0:
                dk[j] -= t * iF * b_ * 2 * h
                ndp[j] += k * t * b_ * 2 * h
            if j == 1:
                dk[j] += dt_ * b_
                ndp[j] += 2 * dt_ * c * p + dq
            if j == 2:
                ndp[j] += q
        p, dp = t * c * p + q, ndp
    return dict(iF=iF, k=k, c=c, t=t, b=b, dt_=dt_, db=db, hd=diF / 2, dk=dk, ou=ou)


def _recursion(tracks, g, mu, start):
    """S, S1, S3, su_a, macc_a over the bulk rows, from BasisScal::step_stat run from row `start` of every track (all tracks at once)."""
    d = tracks[0].shape[1]
    bulk = [y for y in tracks if y.shape[0] > A_ROW]
    nmax = max(y.shape[0] for y in bulk)
    Y = np.zeros((len(bulk), nmax, d), dtype=LD)
    ns = np.array([y.shape[0] for y in bulk])
    for i, y in enumerate(bulk):
        Y[i, :y.shape[0]] = y
    mu = np.asarray(mu, dtype=LD)[None, :]
    x = Y[:, start].copy()
    A1, A3, mx = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    S = S1 = S3 = LD(0)
    su, macc = np.zeros(d, dtype=LD), np.zeros(d, dtype=LD)
    for t in range(start, nmax):
        u = Y[:, t] - x
        if t >= A_ROW:
            w = (t < ns).astype(LD)[:, None]
            S += np.sum(w * u * u); S1 += np.sum(w * u * A1); S3 += np.sum(w * u * A3)
            su += np.sum(w * u, axis=0); macc += np.sum(w * u * mx, axis=0)
        A1 = g["c"] * A1 + u
        A3 = g["c"] * A3 + g["dt_"] * x + g["db"] * mu
        mx = g["c"] * mx + g["b"]
        x = g["k"] * u + g["t"] * x + g["b"] * mu
    return S, S1, S3, su, macc, float(np.sum(ns - A_ROW))


def _finish(g, d, mask, S, S1, S3, macc):
    """BasisScal::finish: ([value | sigma_obs | mu | par d | par d + 1], the same combination of the terms' magnitudes given |.| inputs)"""
    out = np.zeros(4 + d, dtype=LD)
    out[0] = g["iF"] / 2 * S
    s3 = [0, S3, 0]
    slot = [1, 2 + d, 3 + d]
    for j in range(3):
        if (mask & (1, 4, 8)[j]) and (j < 2 or g["ou"]):
            out[slot[j]] = g["hd"][j] * S - g["iF"] * (g["dk"][j] * S1 + s3[j])
    if mask & 2:
        out[2:2 + d] = -g["iF"] * macc
    return out


def _cuts(g):
    kmin = int(np.ceil(np.log(1e-18) / np.log(float(g["c"])))) + 16
    return [kmin, (kmin + 191) // 2, 191]


CASES = [(m, d, r) for m in ("OU_SSM", "BM_SSM") for d in (1, 2) for r in (0.1, 0.5)]
_cache = {}


def _case(model, d, ratio):
    """statistics, stationary constants and the longdouble recursion of one (model, d, ratio): computed once, shared"""
    key = (model, d, ratio)
    if key not in _cache:
        tracks = _tracks(model, d, 60 + d)
        theta = _theta(model, d, ratio)
        ref = next(y for y in tracks if y.shape[0] > A_ROW)[A_ROW - 1].copy() if model == "OU_SSM" else None
        M, s, n, A = capi.lagstats_host(tracks, model=model, ref=ref)
        assert A == A_ROW
        g = _stationary(model, theta, d)
        rec = _recursion(tracks, g, theta[1:1 + d], A_ROW - 255)
        assert rec[5] == n
        _cache[key] = (theta, ref, M, s, n, g, rec)
    return _cache[key]


@pytest.mark.parametrize("free_mu", [True, False], ids=["mu_free", "mu_fixed"])
@pytest.mark.parametrize("model,d,ratio", CASES)
def test_forms_match_the_lanes_stationary_recursion(model, d, ratio, free_mu):
    theta, ref, M, s, n, g, (S, S1, S3, su, macc, _) = _case(model, d, ratio)
    mask = 15 if free_mu else 13
    cuts = _cuts(g)
    assert 16 <= cuts[0] <= 80 and cuts[0] < cuts[1] < cuts[2] == M.shape[0] - 1, cuts
    floor_ = np.sqrt(abs(S) * n)
    sc = lambda v: max(abs(v), floor_)
    want = [S, S1, S3] + list(su)
    for K in cuts:
        f = capi.lagforms_host(M, s, n, theta, DT, K, mask=mask, model=model, ref=ref)
        taps, raw, acc = f["taps"], f["raw"], f["acc"]
        assert taps.shape == (3, M.shape[0]) and np.all(taps[:, K + 1:] == 0.0) and taps[0, 0] == 1.0 and taps[1, 0] == 0.0 and taps[1, 1] == 1.0
        if model == "BM_SSM":
            assert np.all(taps[2] == 0.0) and raw[0, 2] == 0.0 and raw[1, 2] == 0.0
        else:
            assert taps[2, 1] == 0.0 and taps[2, 2] != 0.0
        for j in range(3 + d):
            err = float(abs(LD(raw[0, j]) - want[j]) / sc(want[j]))
            print("%s d=%d ratio=%g K=%d sum %d: %.3e" % (model, d, ratio, K, j, err))
            assert err <= TOL, (K, j, err, raw[0, j], float(want[j]))
        if d == 1:
            assert raw[0, 4] == 0.0 and raw[1, 4] == 0.0
        # the accumulators, on the scale the same combination gives
        ref_acc = _finish(g, d, mask, S, S1, S3, macc)
        g_abs = dict(g, iF=abs(g["iF"]), hd=np.abs(g["hd"]), dk=np.abs(g["dk"]))
        mxs = abs(g["b"] / (1 - g["c"]))
        scale = _finish(g_abs, d, mask, sc(S), -sc(S1), -sc(S3), -mxs * np.array([sc(v) for v in su]))
        assert acc.shape == (4 + d,)
        for k in range(4 + d):
            if ref_acc[k] == 0.0:
                assert acc[k] == 0.0, (k, acc)
                continue
            err = float(abs(LD(acc[k]) - ref_acc[k]) / scale[k])
            print("%s d=%d ratio=%g K=%d acc %d: %.3e" % (model, d, ratio, K, k, err))
            assert err <= TOL, (K, k, err, acc[k], float(ref_acc[k]))
        assert acc[0] > 0.0 and acc[1] != 0.0 and acc[2 + d] != 0.0
        assert np.all(acc[2:2 + d] != 0.0) if free_mu else np.all(acc[2:2 + d] == 0.0)
        assert (acc[3 + d] != 0.0) == (model == "OU_SSM")
        # the two cuts differ by no more than the check value says, on its scale
        for j in range(3 + d):
            a, b = raw[0, j], raw[1, j]
            assert abs(a - b) <= f["chk"] * max(abs(a), abs(b), np.sqrt(abs(raw[0, 0]) * n)) * (1.0 + 1e-14), (j, a, b, f["chk"])
        assert np.isfinite(f["chk"]) and f["chk"] <= 1e-12


@pytest.mark.parametrize("model", ["OU_SSM", "BM_SSM"])
def test_taps_beyond_the_cut_are_never_read(model):
    theta, ref, M, s, n, g, _ = _case(model, 2, 0.5)
    for K in _cuts(g):
        f = capi.lagforms_host(M, s, n, theta, DT, K, model=model, ref=ref)
        h = capi.lagforms_host(M, s, n, theta, DT, K, model=model, ref=ref, taps=f["taps"])
        assert np.array_equal(f["raw"], h["raw"]) and np.array_equal(f["acc"], h["acc"]) and f["chk"] == h["chk"]
        junk = f["taps"].copy()
        junk[:, K + 1:] = 1e30 * (1.0 + np.random.default_rng(5).random(junk[:, K + 1:].shape))
        h = capi.lagforms_host(M, s, n, theta, DT, K, model=model, ref=ref, taps=junk)
        assert np.array_equal(f["raw"], h["raw"]) and np.array_equal(f["acc"], h["acc"]) and f["chk"] == h["chk"]


def test_arguments_out_of_range_are_refused():
    theta, ref, M, s, n, g, _ = _case("OU_SSM", 1, 0.1)
    for K in (15, M.shape[0]):
        with pytest.raises(ValueError):
            capi.lagforms_host(M, s, n, theta, DT, K, model="OU_SSM", ref=ref)
    with pytest.raises(ValueError):
        capi.lagforms_host(M, s, n, theta, DT, 40, model="OU_SSM")                  # levels need their ref
    with pytest.raises(ValueError):
        capi.lagforms_host(M, s, n, theta, 0.0, 40, model="OU_SSM", ref=ref)
    with pytest.raises(ValueError):
        capi.lagforms_host(M, s, n, theta, DT, 40, model="OU", ref=ref)   # a model outside the three
    capi.lagforms_host(M, s, n, theta, DT, 40, model="OU_SSM", ref=ref)


@pytest.mark.parametrize("d", [1, 2])
def test_ctcrw_through_the_new_entry_is_bitwise_the_existing_one(d):
    tracks = _tracks("BM_SSM", d, 9)
    M, s, n, _ = capi.lagstats_host(tracks)
    theta = np.array([np.log(0.1)] + [0.25] * d + [np.log(2.0), 0.0])
    for K in (16, 48, 191):
        f = capi.lagforms_host(M, s, n, theta, DT, K, mask=15)
        h = capi.lagforms_host(M, s, n, theta, DT, K, mask=15, model="CTCRW", ref=np.zeros(d))
        assert np.array_equal(f["raw"], h["raw"]) and np.array_equal(f["acc"], h["acc"]) and f["chk"] == h["chk"]
        assert np.array_equal(f["taps"], h["taps"])
