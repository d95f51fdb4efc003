"""CPU suite: the lane math of ssde_path_occupancy_fine end to end with g++ (tests/hostsim/hostsim_occ_fine.cpp through
tests/occfinesim_lib.py: records -> draws' walk -> ends / side packets by the walk's store rule -> bridge_slot_walk with the kernel's
offsets -> occ_cell -> integer add, over the real plan_all_slots / plan_fine_weights), against the definition (tests/occ_fine_ref.py)
on the reference draws: BITWISE.  The two sides draw the paths independently, so every comparison first asserts that no reference
point -- at a row or inside an interval -- is within 1e-6 of a cell line (occ_cases.py)."""
import numpy as np
import pytest

import occfinesim_lib
from cases import make_spec, problem_from_spec
from occ_cases import clear_of_lines, make_grid
from occ_fine_ref import all_points, fine_plan, occ_fine_counts, reference_draws, to_float
from path_cases import dt_weights

MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
LENGTHS = [12, 25, 1, 40, 2, 7]
NA_ROWS = (4, 5, 11, 20, 60)                    # row 11 ends the first track
GROUPS = [1, 0, 1, -1, 0, 1]


def _max_step(pb, factor=0.4):
    b = np.r_[pb.seg_start, pb.n]
    inner = np.concatenate([np.arange(b[t] + 1, b[t + 1] - 1) for t in range(len(b) - 1)])
    return factor * float(np.median(np.diff(pb.times)[inner]))


def _check(pb, par, obs, tag, seed, draw0=0, n_draws=5, max_step=None, cells=(7, 5)):
    model, d = pb.model, pb.n_dim
    max_step = _max_step(pb) if max_step is None else max_step
    plan = fine_plan(pb.times, pb.seg_start, max_step)
    rows, inner = reference_draws(pb, par, plan, seed=seed, draw0=draw0, n_draws=n_draws)
    pts = all_points(rows, inner)
    grid, shift = make_grid(obs, pts, model, d, cells=cells)
    assert clear_of_lines(pts, model, d, grid), tag
    w = dt_weights(pb.seg_start, pb.times)
    out = None
    for group, ng in ((None, 1), (GROUPS[:pb.n_seg], 2)):
        ref = to_float(*occ_fine_counts(rows, inner, plan, pb.seg_start, model, d, grid, weight=w, group=group, n_groups=ng))
        got = occfinesim_lib.path_occupancy_fine(pb, par, grid, max_step, seed=seed, draw0=draw0, n_draws=n_draws, weight=w, group=group,
                                                 n_groups=ng, with_points=True)
        gplan = fine_plan(pb.times, pb.seg_start, max_step, group=group)
        print(f"OCCFINE {tag} groups={ng} shift={shift} max m={plan['m'].max()} inside={got[0].sum():.6g} outside={got[1].sum():.6g}")
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), tag
        assert got[2] == (gplan["n_points"], gplan["n_capped"]), tag
        out = out or got
    return out, plan


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_constant_coefficients_with_na_rows(model, d):
    spec = make_spec(f"fh_{model}_{d}", model, d, seed=31 + d, lengths=LENGTHS, na_rows=NA_ROWS)
    pb = problem_from_spec(spec)
    (occ, out, _), plan = _check(pb, spec["par"], spec["obs"], f"const {model} d={d}", seed=5, draw0=2)
    assert np.any(occ > 0) and plan["m"].max() >= 4
    # every m = 1 is the twin of ssde_path_occupancy, bit for bit
    import occsim_lib
    w = dt_weights(pb.seg_start, pb.times)
    grid, _ = make_grid(spec["obs"], reference_draws(pb, spec["par"], fine_plan(pb.times, pb.seg_start, np.inf), seed=5, n_draws=4)[0],
                        model, d, cells=(7, 5))
    a = occfinesim_lib.path_occupancy_fine(pb, spec["par"], grid, np.inf, seed=5, n_draws=4, weight=w, group=GROUPS, n_groups=2)
    b = occsim_lib.path_occupancy(pb, spec["par"], grid, seed=5, n_draws=4, weight=w, group=GROUPS, n_groups=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(model, d):
    spec = make_spec(f"fh_hp_{model}_{d}", model, d, seed=41 + d, lengths=LENGTHS, with_H=True, with_P0=True, na_rows=NA_ROWS)
    pb = problem_from_spec(spec)
    _check(pb, spec["par"], spec["obs"], f"H P0 {model} d={d}", seed=9)


@pytest.mark.parametrize("model", MODELS)
def test_row_varying_parameters(model):
    spec = make_spec(f"fh_tv_{model}", model, 2, seed=51, lengths=[30, 18, 1, 44], variant="tv", na_rows=(3, 29, 50))
    pb = problem_from_spec(spec)
    _check(pb, spec["par"], spec["obs"], f"tv {model}", seed=3)


def test_one_interval_at_the_cap():
    spec = make_spec("fh_cap", "OU_SSM", 2, seed=61, lengths=[9, 7], irregular=False)
    t = np.array(spec["times"]); t[5:] += 99.0
    spec["times"] = t
    pb = problem_from_spec(spec)
    (occ, out, pts), plan = _check(pb, spec["par"], spec["obs"], "the cap", seed=4, max_step=1.0)
    assert plan["m"].max() == 64 and pts[1] == 1


def test_negative_p0_follows_the_reference():
    # the det F <= 0 corner of §3.9, d = 1: whatever pivots fail, fail alike; the points without a finite position land outside
    from smoothsde_amd import capi
    from smoothsde_amd.synth import simulate
    seen = 0
    for model in MODELS:
        ID, times, obs = simulate(model, 5, 12, 1, seed=4)
        sdim = 2 if model == "CTCRW" else 1
        P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
        par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
        pb = capi.Problem(model, ID, times, obs, P0=P0)
        (occ, out, _), plan = _check(pb, par, obs, f"negative P0 {model}", seed=2, n_draws=4)
        rows, inner = reference_draws(pb, par, plan, seed=2, n_draws=4)
        lost = np.count_nonzero(~np.isfinite(inner[:, :, 0]))
        assert out[0] > 0 or lost == 0
        seen += int(lost > 0)
    assert seen > 0                                                      # the corner is met


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_written_out_lattice_tracks_spread_a_gap_over_its_slots(model, d):
    """A lattice-padded handle's slots are its lattice rows: the twin runs the written-out tracks with the padded rows flagged, and a
    caller's row shares its weight among the points of every lattice slot up to the next caller's row, padded rows' own points
    included.  The weights are indexed by the caller's rows and the quantum is set by the caller's row count."""
    from smoothsde_amd import capi
    from test_gpu_draws import _written_out
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks(model, d, [40, 25, 1, 33, 2, 18], 0.5, 0.2, seed=8, na_frac=0.05)
    pb = capi.Problem(model, ID, times, obs)
    par = _par(model, d, np.random.default_rng(2))
    ID2, t2, obs2, rows = _written_out(ID, times, obs, 0.5)
    pb2 = capi.Problem(model, ID2, t2, obs2)
    assert pb2.n > pb.n and pb2.n_seg == pb.n_seg
    is_row = np.zeros(pb2.n, dtype=bool)
    is_row[rows] = True
    w2 = np.full(pb2.n, 1e300)                                       # a padded row's weight is never read
    w2[rows] = dt_weights(pb.seg_start, pb.times)
    for max_step in (0.2, 10.0):
        plan = fine_plan(pb2.times, pb2.seg_start, max_step, is_row=is_row)
        prow, inner = reference_draws(pb2, par, plan, seed=11, n_draws=5)
        pts = all_points(prow, inner)
        grid, _ = make_grid(obs, pts, model, d, cells=(7, 5))
        assert clear_of_lines(pts, model, d, grid)
        wr = np.where(is_row, w2, 0.0)
        ref = to_float(*occ_fine_counts(prow, inner, plan, pb2.seg_start, model, d, grid, weight=wr, n_rows=pb.n))
        got = occfinesim_lib.path_occupancy_fine(pb2, par, grid, max_step, seed=11, n_draws=5, weight=w2, is_row=is_row, n_rows=pb.n,
                                                 with_points=True)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        assert got[2] == (plan["n_points"], 0) and plan["m"].max() == (3 if max_step == 0.2 else 1)
        # the padded rows' points carry weight: more points than the caller's rows have
        own_only = fine_plan(pb.times, pb.seg_start, np.inf)["n_points"]
        assert plan["n_points"] > own_only
