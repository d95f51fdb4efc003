"""CPU suite: the numpy statement of ssde_path_occupancy (tests/occ_ref.py) on the draws of tests/draws_ref.py,
against a per-track, per-draw, per-row loop written here from the definition, and the rules the definition implies.  Both sides sum
integers, so every comparison is exact."""
import math

import numpy as np
import pytest

from cases import make_spec, problem_from_spec
from draws_ref import draws_ref
from occ_cases import clear_of_lines, make_grid
from occ_ref import occ_counts, occ_ref, quantise, quantum_exp
from path_cases import dt_weights
from path_ref import position_columns

MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS = [9, 1, 2, 7]                           # rows 0-8 | 9 | 10-11 | 12-18
NA_ROWS = (3, 15)
CELLS = (5, 4)
_CASE = {}


def _case(model, d):
    """problem, eight reference draws, grid and dt weights of a (model, d), computed once"""
    if (model, d) not in _CASE:
        spec = make_spec(f"oh_{model}_{d}", model, d, seed=71 + d, lengths=LENGTHS, na_rows=NA_ROWS)
        pb = problem_from_spec(spec)
        draws = draws_ref(pb, spec["par"], seed=13, n_draws=8)
        draws.setflags(write=False)
        grid, _ = make_grid(spec["obs"], draws, model, d, cells=CELLS)
        _CASE[(model, d)] = (spec, pb, draws, grid, dt_weights(pb.seg_start, pb.times))
    return _CASE[(model, d)]


def _brute(draws, seg_start, model, d, grid, weight, group, n_groups):
    """the definition, one (draw, track, row) at a time, in Python integers"""
    nd, n, _ = draws.shape
    cols = position_columns(model, d)
    nx, ny = grid["nx"], (grid["ny"] if d == 2 else 1)
    wmax = 1.0 if weight is None else max(float(v) for v in weight)
    k = math.frexp(wmax)[1]
    e = max(k + (n * nd).bit_length() - 52, -1074)
    bounds = list(seg_start) + [n]
    occ = [[[0] * nx for _ in range(ny)] for _ in range(n_groups)]
    out = [0] * n_groups
    for q in range(nd):
        for t in range(len(bounds) - 1):
            g = 0 if group is None else int(group[t])
            if g < 0:
                continue
            for j in range(bounds[t] + 1, bounds[t + 1]):
                w = 1.0 if weight is None else float(weight[j])
                scaled = math.ldexp(w, -e)
                wq = round(scaled)                                   # Python rounds halves to even, as nearbyint does
                assert wq == scaled or abs(wq - scaled) <= 0.5
                p = [float(draws[q, j, c]) for c in cols]
                ok = all(math.isfinite(v) for v in p)
                if ok:
                    ix = math.floor((p[0] - grid["x0"]) / grid["dx"])
                    iy = math.floor((p[1] - grid["y0"]) / grid["dy"]) if d == 2 else 0
                    ok = 0 <= ix < nx and 0 <= iy < ny
                if ok:
                    occ[g][iy][ix] += wq
                else:
                    out[g] += wq
    return (np.array([[[math.ldexp(float(v), e) for v in r] for r in gg] for gg in occ]).reshape(n_groups, ny, nx),
            np.array([math.ldexp(float(v), e) for v in out]))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_occ_ref_is_the_definition(model, d):
    spec, pb, draws, grid, w = _case(model, d)
    assert clear_of_lines(draws, model, d, grid)
    for group, ng in ((None, 1), ([1, 0, -1, 1], 2), ([0, 1, 2, 3], 4)):
        occ, out = occ_ref(draws, pb.seg_start, model, d, grid, weight=w, group=group, n_groups=ng)
        rocc, rout = _brute(draws, pb.seg_start, model, d, grid, w, group, ng)
        assert occ.shape == (ng, CELLS[1] if d == 2 else 1, CELLS[0])
        assert np.array_equal(occ, rocc) and np.array_equal(out, rout)
    occ, out = occ_ref(draws, pb.seg_start, model, d, grid, weight=w)
    assert np.any(occ > 0) and np.any(occ == 0) and out[0] > 0      # both branches: the grid spans the 2 % - 98 % quantiles


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_conservation_one_row_tracks_and_left_out_tracks(model, d):
    spec, pb, draws, grid, w = _case(model, d)
    state = np.ones(pb.n, dtype=bool)
    state[pb.seg_start] = False
    occ, out, e = occ_counts(draws, pb.seg_start, model, d, grid, weight=w)
    wq = quantise(w, e)
    assert int(occ.sum()) + int(out.sum()) == 8 * int(wq[state].sum())                      # exact, in quanta
    per, pout = occ_ref(draws, pb.seg_start, model, d, grid, weight=w, group=[0, 1, 2, 3], n_groups=4)
    assert np.all(per[1] == 0) and pout[1] == 0                                             # the one-row track adds nothing
    pooled = occ_ref(draws, pb.seg_start, model, d, grid, weight=w)
    assert np.array_equal(per.sum(axis=0), pooled[0][0]) and pout.sum() == pooled[1][0]     # (sums of < 2^52 quanta: exact)
    left, lout = occ_ref(draws, pb.seg_start, model, d, grid, weight=w, group=[0, 0, 0, -1], n_groups=1)
    assert np.array_equal(left[0], per[0] + per[1] + per[2]) and lout[0] == pout[:3].sum()  # group -1 adds nothing
    none = occ_ref(draws, pb.seg_start, model, d, grid, weight=None)
    ones = occ_ref(draws, pb.seg_start, model, d, grid, weight=np.ones(pb.n))
    assert np.array_equal(none[0], ones[0]) and np.array_equal(none[1], ones[1])
    assert none[0].sum() + none[1].sum() == 8 * state.sum()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_non_finite_positions_are_outside(model, d):
    spec, pb, draws, grid, w = _case(model, d)
    occ, out, e = occ_counts(draws, pb.seg_start, model, d, grid, weight=w)
    wq = quantise(w, e)
    cols = position_columns(model, d)
    for value, (q, j, c) in ((np.nan, (1, 14, cols[-1])), (np.inf, (2, 5, cols[0])), (-np.inf, (0, 6, cols[0]))):
        bad = np.array(draws)
        bad[q, j, c] = value
        occ2, out2, e2 = occ_counts(bad, pb.seg_start, model, d, grid, weight=w)
        assert e2 == e and int(occ2.sum()) + int(out2.sum()) == int(occ.sum()) + int(out.sum())
        moved = int(out2[0]) - int(out[0])
        assert moved in (0, int(wq[j])) and int(occ.sum()) - int(occ2.sum()) == moved      # exactly its weight, if it was inside
        assert (np.asarray(occ2) != np.asarray(occ)).sum() == (1 if moved else 0)
    if model == "CTCRW":                                             # a velocity column is no position
        vel = np.array(draws)
        vel[:, :, 1] = np.nan
        occ3, out3, _ = occ_counts(vel, pb.seg_start, model, d, grid, weight=w)
        assert np.array_equal(occ3, occ) and np.array_equal(out3, out)


def test_the_quantum_rule_spelled_out():
    # w = 1: frexp(1) = (0.5, 1); 19 rows x 8 draws = 152 has 8 bits: e = 1 + 8 - 52
    assert quantum_exp(1.0, 19, 8) == -43 and int(quantise([1.0], -43)[0]) == 2 ** 43
    # a dyadic dt = 0.375 = 0.75 * 2^-1: k = -1; 1000 rows x 32 draws = 32000 has 15 bits
    assert quantum_exp(0.375, 1000, 32) == -1 + 15 - 52 and int(quantise([0.375], -38)[0]) == 3 * 2 ** 35
    assert quantum_exp(0.0, 19, 8) == 8 - 52 and int(quantise([0.0], -44)[0]) == 0           # wmax = 0: every output is 0
    assert quantum_exp(5e-324, 1, 1) == -1074 and int(quantise([5e-324], -1074)[0]) == 1     # the floor of the exponent
    assert quantum_exp(2.0 ** 60, 1 << 20, 1 << 10) == 61 + 31 - 52
    # ties go to even
    assert [int(v) for v in quantise([0.5, 1.5, 2.5, 2.5000001], 0)] == [0, 2, 2, 3]
    # every possible sum stays below 2^52
    for wmax, n, nd in ((1.0, 19, 8), (0.999, 10 ** 7, 32), (123.456, 4095, 4097)):
        e = quantum_exp(wmax, n, nd)
        assert int(quantise([wmax], e)[0]) * n * nd < 2 ** 52
    spec, pb, draws, grid, w = _case("CTCRW", 2)
    occ, out = occ_ref(draws, pb.seg_start, "CTCRW", 2, grid, weight=np.zeros(pb.n))
    assert np.all(occ == 0) and np.all(out == 0)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_draw_ranges_add_up(model, d):
    spec, pb, draws, grid, w = _case(model, d)
    halves = [draws_ref(pb, spec["par"], seed=13, draw0=k, n_draws=4) for k in (0, 4)]
    assert np.array_equal(np.concatenate(halves), draws, equal_nan=True)
    dyadic = np.round(w * 8) / 8                                       # eighths: whole quanta at both exponents
    for weight in (None, dyadic):
        whole = occ_ref(draws, pb.seg_start, model, d, grid, weight=weight)
        a, b = (occ_ref(h, pb.seg_start, model, d, grid, weight=weight) for h in halves)
        assert np.array_equal(whole[0], a[0] + b[0]) and np.array_equal(whole[1], a[1] + b[1])     # bitwise
    # irregular dt: within hits * 2^(e - 1) per cell, e the exponent of the eight-draw call (the coarser one)
    irr = w * (1.0 + 0.1 * np.sin(np.arange(pb.n)))
    whole = occ_ref(draws, pb.seg_start, model, d, grid, weight=irr)
    a, b = (occ_ref(h, pb.seg_start, model, d, grid, weight=irr) for h in halves)
    hits = occ_ref(draws, pb.seg_start, model, d, grid, weight=None)
    e8, e4 = quantum_exp(irr.max(), pb.n, 8), quantum_exp(irr.max(), pb.n, 4)
    assert e8 == e4 + 1
    assert np.all(np.abs(whole[0] - (a[0] + b[0])) <= hits[0] * 2.0 ** (e8 - 1))
    assert np.all(np.abs(whole[1] - (a[1] + b[1])) <= hits[1] * 2.0 ** (e8 - 1))
    assert not np.array_equal(whole[0], a[0] + b[0])                   # ... and the bound is not idle
