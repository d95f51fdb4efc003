"""CPU suite: the numpy reference of ssde_predict_draws (tests/bridge_ref.py) is exact, not merely plausible.

The queried states and the row states of a draw are an affine map of its deviates, row deviates and bridge deviates alike.  Injecting
unit deviates one at a time recovers the map A column by column; A A' must be the posterior covariance of those states, cross blocks
between queries and rows included -- draws_ref.joint_full on the problem with NA rows at the query times (predict_ref.augment) -- and
the zero-deviate answer its mean (= predict_ref's mean at the queries).  Limits: §3.10's -- covariance 1e-9 max|cov|, mean
1e-10 (1 + max|mean|); 1e-7 for the covariance at log sigma_obs = -6.  Measured gaps: DESIGN.md §3.14."""
import numpy as np
import pytest

from bridge_ref import bridge_queries, predict_draws_ref
from draws_ref import draws_ref, joint_full
from predict_cases import MODELS, expected_nan, small_problem
from predict_ref import augment, predict_ref

GAPS = {}


def _exact(pb, par, rows, offs, tag, cov_tol):
    sd, n, m = pb.sdim, pb.n, len(rows)
    aug, index = augment(pb, rows, offs)
    bounds = list(pb.seg_start) + [n]
    ab = list(aug.seg_start) + [aug.n]
    old_pos = np.flatnonzero(~np.isin(np.arange(aug.n), index[index >= 0]))          # the new row of every old row
    assert len(old_pos) == n
    pref = predict_ref(pb, par, rows, offs)["mean"]
    worst_c = worst_m = 0.0
    for k in range(pb.n_seg):
        r0, r1 = bounds[k], bounds[k + 1]
        if r1 - r0 < 2:
            continue
        srow = np.arange(r0 + 1, r1)
        qs = np.flatnonzero((rows > r0) & (rows < r1) & (index >= 0))
        nz = (len(srow) + len(qs)) * sd
        nrm_r = np.zeros((1 + nz, n, sd)); nrm_b = np.zeros((1 + nz, m, sd))
        col = 1
        for j in srow:
            for c in range(sd):
                nrm_r[col, j, c] = 1.0; col += 1
        for q in qs:
            for c in range(sd):
                nrm_b[col, q, c] = 1.0; col += 1
        got_q = predict_draws_ref(pb, par, rows, offs, n_draws=1 + nz, normals=(nrm_r, nrm_b))[:, qs, :]
        got_r = draws_ref(pb, par, n_draws=1 + nz, normals=nrm_r)[:, srow, :]
        stack = np.concatenate([got_q.reshape(1 + nz, -1), got_r.reshape(1 + nz, -1)], axis=1)
        A = (stack[1:] - stack[0]).T
        jm, jcov = joint_full(aug, par, k)
        pos = np.r_[index[qs], old_pos[srow]] - (ab[k] + 1)                          # state-row positions in the augmented track
        sel = (pos[:, None] * sd + np.arange(sd)[None, :]).ravel()
        want_c, want_m = jcov[np.ix_(sel, sel)], jm.reshape(-1)[sel]
        gap_c = np.max(np.abs(A @ A.T - want_c)) / np.max(np.abs(want_c))
        gap_m = np.max(np.abs(stack[0] - want_m)) / (1.0 + np.max(np.abs(want_m)))
        gap_p = np.max(np.abs(got_q[0] - pref[qs]), initial=0.0) / (1.0 + np.max(np.abs(pref[qs]), initial=0.0))
        worst_c, worst_m = max(worst_c, gap_c), max(worst_m, gap_m, gap_p)
        assert gap_c <= cov_tol, (tag, k, gap_c)
        assert gap_m <= 1e-10 and gap_p <= 1e-10, (tag, k, gap_m, gap_p)
    print(f"GAP {tag}: cov {worst_c:.2e} mean {worst_m:.2e}")
    GAPS[tag] = (worst_c, worst_m)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("irregular", [False, True])
@pytest.mark.parametrize("log_sigma_obs,cov_tol", [(-1.0, 1e-9), (-6.0, 1e-7)])
def test_bridges_have_the_joint_posterior_moments(model, d, irregular, log_sigma_obs, cov_tol):
    pb, par = small_problem(model, d, irregular)
    par = par.copy(); par[0] = log_sigma_obs
    rows, offs = bridge_queries(pb, seed=3)
    _exact(pb, par, rows, offs, f"{model} d={d} irregular={irregular} lso={log_sigma_obs}", cov_tol)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_per_row_h_and_a_general_p0(model, d):
    pb, par = small_problem(model, d, with_HP=True)
    rows, offs = bridge_queries(pb, seed=4)
    _exact(pb, par, rows, offs, f"H P0 {model} d={d}", 1e-9)


@pytest.mark.parametrize("model", MODELS)
def test_row_varying_parameters(model):
    pb, par = small_problem(model, 2, variant="tv")
    rows, offs = bridge_queries(pb, seed=5)
    _exact(pb, par, rows, offs, f"tv {model}", 1e-9)


@pytest.mark.parametrize("model", MODELS)
def test_the_rules_of_the_definition(model):
    from predict_cases import intervals
    pb, par = small_problem(model, 2)
    rows, offs = bridge_queries(pb, seed=6)
    first, last, dt = intervals(pb)
    whole = predict_draws_ref(pb, par, rows, offs, seed=7, draw0=0, n_draws=8)
    paths = draws_ref(pb, par, seed=7, draw0=0, n_draws=8)
    # NaN exactly where ssde_predict's rules say
    assert np.array_equal(np.isnan(whole[0, :, 0]), expected_nan(pb, rows, offs))
    assert np.array_equal(np.isnan(whole).all(axis=(0, 2)), np.isnan(whole).any(axis=(0, 2)))
    # delta = 0 is the row's draw and delta = Delta the next row's, bitwise
    z = np.flatnonzero((offs == 0.0) & ~first[rows])
    e = np.flatnonzero((offs == dt[rows]) & ~first[rows] & ~last[rows])
    assert len(z) and len(e)
    assert np.array_equal(whole[:, z], paths[:, rows[z]]) and np.array_equal(whole[:, e], paths[:, rows[e] + 1])
    # a draw is a pure function of its number
    assert np.array_equal(whole[:4], predict_draws_ref(pb, par, rows, offs, seed=7, draw0=0, n_draws=4), equal_nan=True)
    assert np.array_equal(whole[4:], predict_draws_ref(pb, par, rows, offs, seed=7, draw0=4, n_draws=4), equal_nan=True)
    # the order of the queries does not matter
    p = np.lexsort((offs, rows))
    assert np.array_equal(whole[:, p], predict_draws_ref(pb, par, rows[p], offs[p], seed=7, n_draws=8), equal_nan=True)
    # queries in ANOTHER interval change nothing
    j = int(np.flatnonzero(~first & ~last)[0])
    keep = rows != j
    more = predict_draws_ref(pb, par, np.r_[rows[keep], j, j], np.r_[offs[keep], 0.2 * dt[j], 0.7 * dt[j]], seed=7, n_draws=8)
    assert np.array_equal(more[:, :keep.sum()], whole[:, keep], equal_nan=True)
    # interior answers differ between draws and from the ends
    inner = np.flatnonzero((offs > 0) & (offs < dt[rows]) & ~first[rows] & ~last[rows])
    assert np.all(whole[0, inner] != whole[1, inner]) and np.all(whole[:, inner] != paths[:, rows[inner]])


def test_bridge_deviates_never_equal_a_row_deviate_counter():
    from bridge_ref import bridge_normals
    from draws_ref import philox_normals
    zb = bridge_normals(3, 0, 4, 5, 2, 0, 4)
    zr = philox_normals(3, 0, 4, 5, 3, 4)[:, 2, :]
    assert not np.any(zb == zr)
    assert not np.array_equal(zb, bridge_normals(3, 0, 4, 5, 2, 1, 4))
    big = bridge_normals(3, 0, 20000, 5, 2, 7, 2)
    assert abs(big.mean()) < 0.02 and abs(big.std() - 1.0) < 0.02
