"""numpy restatement of ssde_simulate_rows (smoothsde_amd/csrc/k_sim_rows.hip, ssde_simrows.hpp) -- test infrastructure.

The definition in float64 or np.longdouble: the Philox4x32-10 block of tests/sim_ref.py with the counter (row position in the track,
track ordinal, replicate number, stream) -- the replicate number where ssde_simulate's track_hi went --, the same two 53-bit
uniforms (formed in float64, as the device does), Box-Muller, the exact transitions of the reference (R/sde.R:1434-1478, CTCRW_cov
of R/utility.R:188-196) with the parameters of the row before and dt = diff(time), in the forms of ssde_simrows.hpp (expm1 for
1 - e and 1 - e^2, the series of the CTCRW position variance below dt / tau = 1 / 4), and the per-track statistics of the written
observations.  Sums are numpy's (not the device's order): agreement is to rounding, not bitwise."""
import math

import numpy as np

from sim_ref import philox4x32_10

KIND = {"CTCRW": 0, "OU": 1, "OU_SSM": 1, "BM": 2, "BM_SSM": 2}
PI_LD = "3.14159265358979323846264338327950288"


def n_par(model, d):
    return d + (1 if KIND[model] == 2 else 2)


def normal_pair(seed, p, trk, rep, stream, dtype=np.float64):
    """two N(0, 1) deviates per entry of the broadcast (p, trk, rep, stream)"""
    o0, o1, o2, o3 = philox4x32_10(np.asarray(p, dtype=np.uint64), np.asarray(trk, dtype=np.uint64), np.asarray(rep, dtype=np.uint64),
                                   np.asarray(stream, dtype=np.uint64), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u1 = ((((o0 << np.uint64(32)) | o1) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = ((((o2 << np.uint64(32)) | o3) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    u1, u2 = u1.astype(dtype), u2.astype(dtype)
    pi = np.longdouble(PI_LD) if dtype is np.longdouble else np.pi
    r = np.sqrt(-2.0 * np.log(u1))
    a = (2.0 * pi) * u2
    return r * np.cos(a), r * np.sin(a)


def g_series(x, ome, ome2):
    """G(x) = x + (1 - e^(-2x)) / 2 - 2 (1 - e^(-x)); its series sum_{k = 3 .. 14} (-1)^(k + 1) (2^(k - 1) - 2) / k! x^k below 1 / 4"""
    dtype = x.dtype.type
    s = np.zeros_like(x)
    for k in range(14, 2, -1):
        ck = dtype((-1) ** (k + 1) * (2 ** (k - 1) - 2)) / dtype(math.factorial(k))
        s = s * x + ck
    return np.where(x < 0.25, s * x * x * x, x + 0.5 * ome2 - 2.0 * ome)


def factors(kind, dt, p1, p2):
    """what the columns of one transition share (SimrowsFac): arrays over the replicates"""
    F = {"dt": dt}
    if kind == 2:
        F["sd"] = p1 * np.sqrt(dt)
        return F
    x = dt / p1
    F["e"], F["ome"] = np.exp(-x), -np.expm1(-x)
    ome2 = -np.expm1(-2.0 * x)
    if kind == 1:
        F["sd"] = np.sqrt(p2 * ome2)
        return F
    pi = np.longdouble(PI_LD) if x.dtype.type is np.longdouble else np.pi
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        h = 2.0 * (p2 * p2) / pi
        F["a"] = p1 * F["ome"]
        F["l11"] = np.sqrt(h * ome2)
        F["l21"] = (h * p1) * (F["ome"] * F["ome"]) / F["l11"]
        qzz = (2.0 * h) * (p1 * p1) * g_series(x, F["ome"], ome2)
        F["l22"] = np.sqrt(np.maximum(qzz - F["l21"] * F["l21"], 0.0))
    return F


def step(kind, F, mu, na, nb, z, v):
    if kind == 2:
        return z + mu * F["dt"] + F["sd"] * na, v
    if kind == 1:
        return F["e"] * z + F["ome"] * mu + F["sd"] * na, v
    zn = z + mu * F["dt"] + (v - mu) * F["a"] + F["l21"] * na + F["l22"] * nb
    return zn, F["e"] * v + F["ome"] * mu + F["l11"] * na


def par_values(X_fe, X_re, link, coeff, n, dtype=np.float64):
    """par[j]: (n_coeff_rows, n) natural-scale values of parameter j at every row"""
    out, off = [], 0
    cf = np.asarray(coeff, dtype=np.float64).astype(dtype)
    for j in range(len(X_fe)):
        cols = [np.ones((n, 1)) if X_fe[j] is None else np.asarray(X_fe[j], dtype=np.float64)]
        if X_re[j] is not None:
            cols.append(np.asarray(X_re[j], dtype=np.float64))
        X = np.concatenate(cols, axis=1).astype(dtype)
        K = X.shape[1]
        lp = cf[:, off:off + K] @ X.T
        with np.errstate(over="ignore"):
            out.append(np.exp(lp) if link[j] == 1 else lp)
        off += K
    assert off == cf.shape[1]
    return out


def track_stats(y, thr):
    """y: (n_rep, T, d) written observations of one track -> (n_rep, 3 d + 2 + n_thr)"""
    R, T, d = y.shape
    out = np.full((R, 3 * d + 2 + len(thr)), np.nan, dtype=y.dtype)
    if T < 2:
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        D = np.diff(y, axis=1)
        L = np.sqrt(np.sum(D * D, axis=2))
        for c in range(d):
            out[:, 3 * c] = np.sum(D[:, :, c], axis=1)
            out[:, 3 * c + 1] = np.sum(D[:, :, c] ** 2, axis=1)
            out[:, 3 * c + 2] = np.sum(D[:, 1:, c] * D[:, :-1, c], axis=1)
        out[:, 3 * d] = np.sum(L, axis=1)
        out[:, 3 * d + 1] = np.max(L, axis=1)
        for r, th in enumerate(thr):
            out[:, 3 * d + 2 + r] = np.sum(L <= th, axis=1)
    out[~np.all(np.isfinite(y), axis=(1, 2))] = np.nan
    return out


def simrows_ref(model, n_dim, row0, times, X_fe, X_re, link, coeff, sigma_obs=None, z0=0.0, seed=0, rep0=0, n_rep=1, thr=(),
                dtype=np.float64, steps=False):
    """{"obs": (n_rep, n, d), "stats": (n_rep, n_tracks, 3 d + 2 + n_thr)}; with `steps` also "L": the step lengths of every
    (replicate, row), NaN on a track's first row"""
    kind, d = KIND[model], int(n_dim)
    row0 = np.asarray(row0, dtype=np.int64)
    times = np.asarray(times, dtype=np.float64)
    n, M, R = len(times), len(row0) - 1, int(n_rep)
    coeff = np.atleast_2d(np.asarray(coeff, dtype=np.float64))
    crow = np.zeros(R, dtype=int) if coeff.shape[0] == 1 else np.arange(R)
    par = [p[crow] for p in par_values(X_fe, X_re, link, coeff, n, dtype)]
    assert len(par) == n_par(model, d)
    so = np.zeros(R) if sigma_obs is None else np.broadcast_to(np.asarray(sigma_obs, dtype=np.float64), (coeff.shape[0],))[crow]
    so = so.astype(dtype)
    z0 = np.broadcast_to(np.asarray(z0, dtype=np.float64), (d,)).astype(dtype)
    thr = np.asarray(thr, dtype=np.float64)
    reps = np.arange(rep0, rep0 + R, dtype=np.uint64)
    obs = np.full((R, n, d), np.nan, dtype=dtype)
    stats = np.full((R, M, 3 * d + 2 + len(thr)), np.nan, dtype=dtype)
    Lall = np.full((R, n), np.nan, dtype=dtype)
    for t in range(M):
        r0, T = int(row0[t]), int(row0[t + 1] - row0[t])
        if T == 0:
            continue
        pos = np.arange(T, dtype=np.uint64)[:, None]
        y = np.zeros((R, T, d), dtype=dtype)
        bad = np.zeros(R, dtype=bool)
        dts = (times[r0 + 1:r0 + T] - times[r0:r0 + T - 1]).astype(dtype)
        for c in range(d):
            na, n2 = normal_pair(seed, pos, t, reps[None, :], 2 * c, dtype)             # (T, R)
            if kind == 0:
                nb, no = n2, normal_pair(seed, pos, t, reps[None, :], 2 * c + 1, dtype)[0]
            else:
                nb, no = None, n2
            z = np.full(R, z0[c], dtype=dtype)
            v = np.zeros(R, dtype=dtype)
            y[:, 0, c] = z + so * no[0]
            for p in range(1, T):
                i1 = r0 + p - 1
                p1 = par[d][:, i1]
                p2 = par[d + 1][:, i1] if len(par) > d + 1 else np.zeros(R, dtype=dtype)
                mu = par[c][:, i1]
                bad |= ~(np.isfinite(p1) & np.isfinite(p2) & np.isfinite(mu))
                with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                    F = factors(kind, dts[p - 1], p1, p2)
                    z, v = step(kind, F, mu, na[p], None if nb is None else nb[p], z, v)
                    y[:, p, c] = z + so * no[p]
        obs[:, r0:r0 + T, :] = y
        st = track_stats(y, thr)
        st[bad] = np.nan
        stats[:, t, :] = st
        if T >= 2:
            with np.errstate(invalid="ignore", over="ignore"):
                Lall[:, r0 + 1:r0 + T] = np.sqrt(np.sum(np.diff(y, axis=1) ** 2, axis=2))
    out = {"obs": obs, "stats": stats}
    if steps:
        out["L"] = Lall
    return out
