"""Grids shared by the tests of ssde_path_occupancy (test infrastructure).

A cell line must not sit on a drawn position, or a 1e-15 difference between two implementations would flip a cell.  Per position
column: lo, hi = quantile(obs, [.02, .98]), dx = round((hi - lo) / nc, 3), x0 = round(lo, 3) + s * 1e-3 * dx for the first shift
s = 0, 1, ... <= 15 at which every finite reference-drawn coordinate is more than 1e-6 from every cell line of the grid (the lines
x0 + i dx, i = 0 .. nc); clear_of_lines() is the precondition every comparison asserts on its reference draws."""
import numpy as np

from occ_ref import grid_of
from path_ref import position_columns

CLEARANCE = 1e-6


def line_distance(draws, model, d, grid):
    """the smallest distance of a finite drawn position coordinate to a cell line of its column"""
    best = np.inf
    for c, col in enumerate(position_columns(model, d)):
        lo, step, nc = (grid["x0"], grid["dx"], grid["nx"]) if c == 0 else (grid["y0"], grid["dy"], grid["ny"])
        p = draws[:, :, col]
        p = p[np.isfinite(p)]
        if p.size:
            u = (p - lo) / step
            near = np.clip(np.rint(u), 0, nc)                           # the nearest of the lines 0 .. nc
            best = min(best, float(np.min(np.abs(u - near)) * step))
    return best


def clear_of_lines(draws, model, d, grid):
    return line_distance(draws, model, d, grid) > CLEARANCE


def make_grid(obs, draws, model, d, cells=(16, 12)):
    """the grid of the module's rule: (grid, shift used)"""
    obs = np.asarray(obs, dtype=np.float64)
    lo, step = [], []
    for a in range(d):
        col = obs[:, a]
        q = np.quantile(col[~np.isnan(col)], [.02, .98])
        step.append(round(float(q[1] - q[0]) / cells[a], 3))
        lo.append(round(float(q[0]), 3))
    for s in range(16):
        g = grid_of(lo[0] + s * 1e-3 * step[0], step[0], cells[0]) if d == 1 else \
            grid_of(lo[0] + s * 1e-3 * step[0], step[0], cells[0], lo[1] + s * 1e-3 * step[1], step[1], cells[1])
        if clear_of_lines(draws, model, d, g):
            return g, s
    raise AssertionError("no shift <= 15 clears the cell lines")
