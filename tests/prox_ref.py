"""Reference of ssde_path_proximity in numpy alone: no twin, no csrc header.  From the array ssde_predict_draws
returns for the A queries followed by the B queries, the pair list, the weights and the radii it forms the statistics the call defines,
with Python integers for the quanta; `undecided` counts the items an exact comparison could not settle against another arithmetic."""
import math

import numpy as np


def position_columns(model, d):
    """the position columns of the state: DenseDims<MODEL, D>::z"""
    return [2 * c for c in range(d)] if model == "CTCRW" else list(range(d))


def quantum_exp(wmax, n_point):
    """occ_quantum_exp(wmax, n_point, 1): frexp(wmax) = (m, k), b the bit length of n_point, e = max(k + b - 52, -1074)"""
    k = math.frexp(float(wmax))[1]
    return max(k + int(n_point).bit_length() - 52, -1074)


def quantise(w, e):
    """nearbyint(ldexp(w, -e)), ties to even, as a Python integer; w finite and >= 0"""
    x = math.ldexp(float(w), -e)                # (exact unless it underflows, and then it rounds to 0 or 1 quantum as ldexp does)
    return int(round(x)) if x < 2.0 ** 53 else int(x)          # Python's round: ties to even


def distances(draws_at, model, d):
    """(n_draws, n_point) distances between the two halves of draws_at (n_draws, 2 n_point, sdim); NaN where a position of either side is
    not finite"""
    z = position_columns(model, d)
    n_point = draws_at.shape[1] // 2
    a, b = draws_at[:, :n_point][:, :, z], draws_at[:, n_point:][:, :, z]
    ok = np.isfinite(a).all(axis=2) & np.isfinite(b).all(axis=2)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = a - b
        dist = np.abs(diff[:, :, 0]) if d == 1 else np.sqrt((diff * diff).sum(axis=2))
    return np.where(ok, dist, np.nan)


def proximity(draws_at, model, d, pair_ptr, radii=(), weight=None):
    """(n_draws, n_pairs, 2 + n_radii): min distance, index of its first point, the fixed-point sums"""
    pair_ptr = np.asarray(pair_ptr, dtype=np.int64)
    radii = np.asarray(radii, dtype=np.float64).ravel()
    n_draws, n_point, n_pairs = draws_at.shape[0], draws_at.shape[1] // 2, len(pair_ptr) - 1
    assert pair_ptr[-1] == n_point
    dist = distances(draws_at, model, d)
    wmax = 1.0 if weight is None else float(np.max(weight, initial=0.0))
    e = quantum_exp(wmax, n_point)
    wq = [quantise(1.0 if weight is None else weight[i], e) for i in range(n_point)]
    out = np.full((n_draws, n_pairs, 2 + len(radii)), np.nan)
    for p in range(n_pairs):
        lo, hi = int(pair_ptr[p]), int(pair_ptr[p + 1])
        if hi == lo:
            continue
        for q in range(n_draws):
            dd = dist[q, lo:hi]
            if np.isnan(dd).any():
                continue
            k = int(np.argmin(dd))                                   # the first of equal minima
            out[q, p, 0], out[q, p, 1] = dd[k], k
            for r, rad in enumerate(radii):
                total = sum(wq[lo + i] for i in np.flatnonzero(dd <= rad))
                out[q, p, 2 + r] = math.ldexp(float(total), e)       # total < 2^53: float() is exact
    return out


def proximity_fast(draws_at, model, d, pair_ptr, radii=(), weight=None):
    """the same numbers vectorised over draws (np.minimum.reduceat and integer sums in int64): the host route a caller had before the
    call existed, timed by tools/bench_prox.py.  Pairs must not be empty."""
    pair_ptr = np.asarray(pair_ptr, dtype=np.int64)
    radii = np.asarray(radii, dtype=np.float64).ravel()
    n_draws, n_point = draws_at.shape[0], draws_at.shape[1] // 2
    dist = distances(draws_at, model, d)
    wmax = 1.0 if weight is None else float(np.max(weight, initial=0.0))
    e = quantum_exp(wmax, n_point)
    w = np.ones(n_point) if weight is None else np.asarray(weight, dtype=np.float64)
    wq = np.rint(np.ldexp(w, -e)).astype(np.int64)
    starts = pair_ptr[:-1]
    out = np.empty((n_draws, len(starts), 2 + len(radii)))
    bad = np.add.reduceat(np.isnan(dist).astype(np.int64), starts, axis=1) > 0
    dmin = np.minimum.reduceat(np.where(np.isnan(dist), np.inf, dist), starts, axis=1)
    out[:, :, 0] = dmin
    first = np.where(dist == np.repeat(dmin, np.diff(pair_ptr), axis=1), np.arange(n_point)[None, :], n_point)
    out[:, :, 1] = np.minimum.reduceat(first, starts, axis=1) - starts[None, :]
    for r, rad in enumerate(radii):
        out[:, :, 2 + r] = np.ldexp(np.add.reduceat(np.where(dist <= rad, wq[None, :], 0), starts, axis=1).astype(np.float64), e)
    out[bad] = np.nan
    return out


def undecided(draws_at, model, d, pair_ptr, radii=(), tol=1e-12):
    """How many items an exact comparison cannot settle when the other side's distances differ from these by up to `tol` relative:
    distances within tol * (1 + r) of a radius r (a finite one), plus (pair, draw)s whose two smallest distances differ by less than
    tol relative (the index of the minimum could move).  NaN (pair, draw)s and empty pairs are decided: NaN either way."""
    pair_ptr = np.asarray(pair_ptr, dtype=np.int64)
    dist = distances(draws_at, model, d)
    count = 0
    for rad in np.asarray(radii, dtype=np.float64).ravel():
        if np.isfinite(rad):
            with np.errstate(invalid="ignore"):
                count += int(np.sum(np.abs(dist - rad) <= tol * (1.0 + rad)))
    for p in range(len(pair_ptr) - 1):
        lo, hi = int(pair_ptr[p]), int(pair_ptr[p + 1])
        if hi - lo < 2:
            continue
        dd = np.sort(dist[:, lo:hi], axis=1)
        ok = ~np.isnan(dd).any(axis=1)
        count += int(np.sum(ok & (dd[:, 1] - dd[:, 0] < tol * np.maximum(dd[:, 1], np.finfo(float).tiny))))
    return count


def compare(got, ref, tag, rel=1e-12, scale_abs=False):
    """got vs ref (n_draws, n_pairs, n_stat): identical NaN patterns, the index and the sums bitwise, the minimum within rel relative
    (scale_abs: within rel * (1 + the largest reference minimum))"""
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{tag}: NaN patterns differ"
    ok = ~np.isnan(ref[:, :, 0])
    g, r = got[:, :, 0][ok], ref[:, :, 0][ok]
    if g.size:
        bound = rel * (1.0 + np.max(r)) if scale_abs else rel * np.abs(r)
        worst = float(np.max(np.abs(g - r) - bound))
        print(f"{tag}: min distance worst excess over the bound {worst:.3e} (largest difference {float(np.max(np.abs(g - r))):.3e})")
        assert np.all(np.abs(g - r) <= bound), f"{tag}: minimum distance off by {float(np.max(np.abs(g - r))):.3e}"
    assert np.array_equal(got[:, :, 1:], ref[:, :, 1:], equal_nan=True), f"{tag}: index or sums differ"
