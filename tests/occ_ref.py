"""numpy restatement of ssde_path_occupancy for the tests (test infrastructure): the definition and nothing else,
on an array of draws -- those of tests/draws_ref.py, of the host twin, or a GPU's own.  The quantum rule and the quantisation are
part of the definition, so the result is comparable BITWISE.

* A track's state rows are rows first + 1 .. last of `seg_start`'s segments; position columns as path_ref.position_columns.
* The cell of a position is ix = floor((p_1 - x0) / dx), iy = floor((p_2 - y0) / dy) (IEEE divisions); inside when 0 <= ix < nx and
  0 <= iy < ny; d = 1 has ny = 1 and reads neither y0 nor dy; a non-finite coordinate is outside.
* occ[g, iy, ix] is the sum of w_j over the draws, the tracks with group[t] == g and their state rows in the cell; outside[g] the same
  sum over the state rows in no cell.  group -1: the track takes part in nothing; group None: one group.
* Fixed point: wmax the largest weight (1 for None), frexp(wmax) = (m, k), b the bit length of n_rows * n_draws,
  e = max(k + b - 52, -1074); w_j enters as the integer nearbyint(ldexp(w_j, -e)) (ties to even), the integers are summed exactly and
  an output is ldexp(float(sum), e).  n_rows is the row count of the caller's data (draws.shape[1] unless given).
"""
from __future__ import annotations

import math

import numpy as np

from path_ref import position_columns


def grid_of(x0, dx, nx, y0=0.0, dy=1.0, ny=1):
    return {"x0": float(x0), "dx": float(dx), "nx": int(nx), "y0": float(y0), "dy": float(dy), "ny": int(ny)}


def quantum_exp(wmax, n_rows, n_draws):
    k = math.frexp(float(wmax))[1]
    b = (int(n_rows) * int(n_draws)).bit_length()
    return max(k + b - 52, -1074)


def quantise(w, e):
    """the weights as whole numbers of 2^e (np.rint rounds half to even); object-free uint64"""
    return np.rint(np.ldexp(np.asarray(w, dtype=np.float64), -e)).astype(np.uint64)


def cells_of(p, grid, d):
    """the cell ix + nx * iy of positions p (..., d), -1 outside"""
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((p[..., 0] - grid["x0"]) / grid["dx"])
        ok = (fx >= 0) & (fx < grid["nx"])
        cell = np.where(ok, fx, 0.0)
        if d == 2:
            fy = np.floor((p[..., 1] - grid["y0"]) / grid["dy"])
            ok &= (fy >= 0) & (fy < grid["ny"])
            cell = cell + grid["nx"] * np.where((fy >= 0) & (fy < grid["ny"]), fy, 0.0)
    return np.where(ok, cell, -1.0).astype(np.int64)


def occ_counts(draws, seg_start, model, d, grid, weight=None, group=None, n_groups=1, n_rows=None):
    """(counts (n_groups, ny, nx) uint64, outside counts (n_groups,) uint64, e)"""
    draws = np.asarray(draws, dtype=np.float64)
    nd, n, _ = draws.shape
    n_rows = n if n_rows is None else n_rows
    cols = position_columns(model, d)
    nx, ny = grid["nx"], (grid["ny"] if d == 2 else 1)
    w = np.ones(n) if weight is None else np.asarray(weight, dtype=np.float64)
    e = quantum_exp(1.0 if weight is None else np.max(w, initial=0.0), n_rows, nd)
    wq = quantise(w, e)
    bounds = np.r_[np.asarray(seg_start, dtype=np.int64), n]
    occ = np.zeros((n_groups, nx * ny), dtype=np.uint64)
    out = np.zeros(n_groups, dtype=np.uint64)
    for t in range(len(bounds) - 1):
        g = 0 if group is None else int(group[t])
        rows = np.arange(bounds[t] + 1, bounds[t + 1])
        if g < 0 or len(rows) == 0:
            continue
        cell = cells_of(draws[:, rows][:, :, cols], grid, d)                # n_draws x m
        wt = np.broadcast_to(wq[rows][None, :], cell.shape)
        inside = cell >= 0
        np.add.at(occ[g], cell[inside], wt[inside])
        out[g] += wt[~inside].sum(dtype=np.uint64)
    return occ.reshape(n_groups, ny, nx), out, e


def occ_ref(draws, seg_start, model, d, grid, weight=None, group=None, n_groups=1, n_rows=None):
    """(occ (n_groups, ny, nx), outside (n_groups,)) as ssde_path_occupancy returns them"""
    occ, out, e = occ_counts(draws, seg_start, model, d, grid, weight=weight, group=group, n_groups=n_groups, n_rows=n_rows)
    assert max(int(occ.max(initial=0)), int(out.max(initial=0))) < 2 ** 52
    return np.ldexp(occ.astype(np.float64), e), np.ldexp(out.astype(np.float64), e)
