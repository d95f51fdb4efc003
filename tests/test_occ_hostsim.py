"""CPU suite: the lane math of ssde_path_occupancy (csrc/ssde_occ.hpp over csrc/ssde_draws.hpp), built with g++
(tests/hostsim/hostsim_occ.cpp through tests/occsim_lib.py), against the definition (tests/occ_ref.py) on the reference draws
(tests/draws_ref.py): BITWISE.  The two sides draw the paths independently (they agree to ~1e-13), so every comparison first asserts
that no reference position is within 1e-6 of a cell line (occ_cases.py): then both put every position in the same cell and add the
same integers."""
import numpy as np
import pytest

import occsim_lib
from cases import make_spec, problem_from_spec
from draws_ref import draws_ref
from occ_cases import clear_of_lines, make_grid
from occ_ref import occ_ref
from path_cases import dt_weights

MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS = [12, 25, 1, 40, 2, 7]
NA_ROWS = (4, 5, 11, 20, 60)                    # row 11 ends the first track
GROUPS = [1, 0, 1, -1, 0, 1]


def _check(pb, par, obs, tag, seed, draw0=0, n_draws=5):
    model, d = pb.model, pb.n_dim
    with np.errstate(invalid="ignore"):
        draws = draws_ref(pb, par, seed=seed, draw0=draw0, n_draws=n_draws)
    grid, shift = make_grid(obs, draws, model, d, cells=(7, 5))
    assert clear_of_lines(draws, model, d, grid), tag
    w = dt_weights(pb.seg_start, pb.times)
    out = None
    for group, ng in ((None, 1), (GROUPS[:pb.n_seg], 2)):
        ref = occ_ref(draws, pb.seg_start, model, d, grid, weight=w, group=group, n_groups=ng)
        got = occsim_lib.path_occupancy(pb, par, grid, seed=seed, draw0=draw0, n_draws=n_draws, weight=w, group=group, n_groups=ng)
        print(f"OCC {tag} groups={ng} shift={shift} inside={got[0].sum():.6g} outside={got[1].sum():.6g}")
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), tag
        out = out or got
    return out


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_constant_coefficients_with_na_rows(model, d):
    spec = make_spec(f"dh_{model}_{d}", model, d, seed=31 + d, lengths=LENGTHS, na_rows=NA_ROWS)
    pb = problem_from_spec(spec)
    occ, out = _check(pb, spec["par"], spec["obs"], f"const {model} d={d}", seed=5, draw0=2)
    assert np.any(occ > 0) and out[0] > 0
    # the twin's own invariances, bitwise: draw ranges with unit weights, weight = None as ones
    grid, _ = make_grid(spec["obs"], draws_ref(pb, spec["par"], seed=5, n_draws=8), model, d, cells=(7, 5))
    whole = occsim_lib.path_occupancy(pb, spec["par"], grid, seed=5, draw0=0, n_draws=8)
    a = occsim_lib.path_occupancy(pb, spec["par"], grid, seed=5, draw0=0, n_draws=4)
    b = occsim_lib.path_occupancy(pb, spec["par"], grid, seed=5, draw0=4, n_draws=4)
    ones = occsim_lib.path_occupancy(pb, spec["par"], grid, seed=5, draw0=4, n_draws=4, weight=np.ones(pb.n))
    assert np.array_equal(whole[0], a[0] + b[0]) and np.array_equal(whole[1], a[1] + b[1])
    assert np.array_equal(b[0], ones[0]) and np.array_equal(b[1], ones[1])
    assert whole[0].sum() + whole[1].sum() == 8 * (pb.n - pb.n_seg)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(model, d):
    spec = make_spec(f"dh_hp_{model}_{d}", model, d, seed=41 + d, lengths=LENGTHS, with_H=True, with_P0=True, na_rows=NA_ROWS)
    pb = problem_from_spec(spec)
    _check(pb, spec["par"], spec["obs"], f"H P0 {model} d={d}", seed=9)


@pytest.mark.parametrize("model", MODELS)
def test_row_varying_parameters(model):
    spec = make_spec(f"dh_tv_{model}", model, 2, seed=51, lengths=[30, 18, 1, 44], variant="tv", na_rows=(3, 29, 50))
    pb = problem_from_spec(spec)
    _check(pb, spec["par"], spec["obs"], f"tv {model}", seed=3)


def test_negative_p0_follows_the_reference():
    # the det F <= 0 corner of §3.9, d = 1: whatever pivots fail, fail alike; the rows without a finite position land outside
    from smoothsde_amd import capi
    from smoothsde_amd.synth import simulate
    seen = 0
    for model in MODELS:
        ID, times, obs = simulate(model, 5, 12, 1, seed=4)
        sdim = 2 if model == "CTCRW" else 1
        P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
        par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
        pb = capi.Problem(model, ID, times, obs, P0=P0)
        with np.errstate(invalid="ignore"):
            draws = draws_ref(pb, par, seed=2, n_draws=4)
        occ, out = _check(pb, par, obs, f"negative P0 {model}", seed=2, n_draws=4)
        w = dt_weights(pb.seg_start, pb.times)
        state = np.ones(pb.n, dtype=bool)
        state[pb.seg_start] = False
        col = 0
        lost = sum(w[j] for q in range(4) for j in np.flatnonzero(state) if not np.isfinite(draws[q, j, col]))
        assert out[0] >= lost > 0 or lost == 0
        assert abs(occ.sum() + out[0] - 4 * w[state].sum()) <= 1e-9      # conservation (exact in quanta; dt is not dyadic)
        seen += int(lost > 0)
    assert seen > 0                                                      # the corner is met


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_rows_that_are_not_the_callers_take_part_in_nothing(model, d):
    """A lattice-padded handle walks its padded rows too: the twin runs the written-out tracks with those rows flagged, the reference
    is the definition on the caller's rows of the same draws, with the weights indexed by the caller's rows and the quantum set by
    the caller's row count."""
    from smoothsde_amd import capi
    from test_gpu_draws import _written_out
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks(model, d, [40, 25, 1, 33, 2, 18], 0.5, 0.2, seed=8, na_frac=0.05)
    pb = capi.Problem(model, ID, times, obs)
    par = _par(model, d, np.random.default_rng(2))
    ID2, t2, obs2, rows = _written_out(ID, times, obs, 0.5)
    pb2 = capi.Problem(model, ID2, t2, obs2)
    assert pb2.n > pb.n and pb2.n_seg == pb.n_seg
    draws = draws_ref(pb2, par, seed=11, n_draws=5)
    own = draws[:, rows, :]
    grid, _ = make_grid(obs, own, model, d, cells=(7, 5))
    assert clear_of_lines(own, model, d, grid)
    w = dt_weights(pb.seg_start, pb.times)
    ref = occ_ref(own, pb.seg_start, model, d, grid, weight=w)
    is_row = np.zeros(pb2.n, dtype=bool)
    is_row[rows] = True
    w2 = np.full(pb2.n, 1e300)                                       # a padded row's weight is never read into a sum
    w2[rows] = w
    got = occsim_lib.path_occupancy(pb2, par, grid, seed=11, n_draws=5, weight=w2, is_row=is_row, n_rows=pb.n)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    # ... and they do change the numbers: every written-out row taken as a row of the data counts more rows
    every = occsim_lib.path_occupancy(pb2, par, grid, seed=11, n_draws=5)
    fewer = occsim_lib.path_occupancy(pb2, par, grid, seed=11, n_draws=5, is_row=is_row)
    assert every[0].sum() + every[1].sum() > fewer[0].sum() + fewer[1].sum()
