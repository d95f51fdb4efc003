"""CPU suite: the lane math of ssde_path_proximity (csrc/ssde_prox.hpp: the point step, the wave butterfly, the combine, the fold over
the tile plan and the finish, as k_path_prox.hip runs them), built with g++ (tests/hostsim/hostsim_prox.cpp through
tests/proxsim_lib.py), against the numpy reference written from the definition (tests/prox_ref.py).  The positions are the host twin's
ssde_predict_draws (tests/predictdrawsim_lib.py).  The sums and the index are compared bitwise after prox_ref.undecided (tol 1e-12) is
asserted 0 on the reference; the minimum distance within 1e-12 relative."""
import subprocess

import numpy as np
import pytest

import predictdrawsim_lib as drawsim
import prox_ref
import proxsim_lib as twin
from predict_cases import MODELS, small_problem
from prox_cases import EDGE_SIZES, RADII, RADII8, STAT_DRAWS, STAT_SEED, concat, points, stat_problem, stat_ratio

ND, TOL = 5, 1e-12
_POS = {}


def _positions(model, d, seed=3, forecast=0.1):
    """the twin's predict_draws of one call of the edge sizes on the small problem, computed once per (model, d)"""
    key = (model, d, seed, forecast)
    if key not in _POS:
        pb, par = small_problem(model, d)
        ra, oa, rb, ob, pp = points(pb, EDGE_SIZES, seed=seed + d, forecast=forecast)
        rows, offs = concat(ra, oa, rb, ob)
        at = drawsim.predict_draws(pb, par, rows, offs, seed=11, draw0=2, n_draws=ND)
        at.setflags(write=False)
        _POS[key] = (at, pp)
    return _POS[key]


def _both(at, model, d, pp, radii, weight=None, tag=""):
    assert prox_ref.undecided(at, model, d, pp, radii, tol=TOL) == 0, tag
    got, ref = twin.proximity(at, model, d, pp, radii, weight), prox_ref.proximity(at, model, d, pp, radii, weight)
    prox_ref.compare(got, ref, tag, rel=TOL)
    return got


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
def test_the_edge_sizes_against_the_reference(model, d):
    at, pp = _positions(model, d)
    w = np.random.default_rng(5).uniform(0.0, 2.0, int(pp[-1]))
    got = _both(at, model, d, pp, RADII, w, f"twin vs prox_ref: {model} d={d} weights")
    assert np.all(np.isnan(got[:, 0])) and np.all(np.isfinite(got[:, 1:]))               # the empty pair, and no other
    assert np.all(got[:, 1:, 1] < np.array(EDGE_SIZES[1:])[None, :]) and np.all(got[:, 5, 1] >= 0)
    none = _both(at, model, d, pp, RADII, None, f"twin vs prox_ref: {model} d={d} no weights")
    assert np.array_equal(none[:, 1:, 4], np.broadcast_to(np.array(EDGE_SIZES[1:], dtype=float), (ND, 5)))      # r = inf counts every point
    assert np.array_equal(none, twin.proximity(at, model, d, pp, RADII, np.ones(int(pp[-1]))), equal_nan=True)
    _both(at, model, d, pp, RADII8, w, f"twin vs prox_ref: {model} d={d} 8 radii")
    _both(at, model, d, pp, [], w, f"twin vs prox_ref: {model} d={d} no radius")


def test_the_vectorised_reference_agrees_with_the_plain_one():
    at, pp = _positions("CTCRW", 2)
    w = np.random.default_rng(6).uniform(0.0, 2.0, int(pp[-1]))
    a = prox_ref.proximity(at, "CTCRW", 2, pp, RADII, w)[:, 1:]
    b = prox_ref.proximity_fast(at, "CTCRW", 2, pp[1:], RADII, w)                         # (the fast form takes no empty pair)
    assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("model,d", [("CTCRW", 2), ("OU_SSM", 1)])
def test_identical_sides_a_duplicated_point_and_zero_weights(model, d):
    pb, par = small_problem(model, d)
    ra, oa, _, _, pp = points(pb, [7, 300], seed=21)
    rows, offs = concat(ra, oa, ra, oa)                                                  # both sides identical
    at = drawsim.predict_draws(pb, par, rows, offs, seed=4, n_draws=ND)
    w = np.random.default_rng(7).uniform(0.5, 2.0, 307)
    radii = [0.0, 0.37, np.inf]
    got = twin.proximity(at, model, d, pp, radii, w)
    ref = prox_ref.proximity(at, model, d, pp, radii, w)
    assert np.array_equal(got, ref)
    assert np.all(got[:, :, 0] == 0.0) and np.all(got[:, :, 1] == 0.0)                    # minimum 0 at index 0
    assert np.all(got[:, :, 2] == got[:, :, 4]) and np.all(got[:, :, 3] == got[:, :, 4])   # every radius, 0 included: the whole weight
    e = prox_ref.quantum_exp(w.max(), 307)
    whole = [float(np.ldexp(float(sum(prox_ref.quantise(x, e) for x in w[a:b])), e)) for a, b in ((0, 7), (7, 307))]
    assert np.array_equal(got[:, :, 4], np.broadcast_to(whole, (ND, 2)))
    zero = twin.proximity(at, model, d, pp, radii, np.zeros(307))
    assert np.all(zero[:, :, 2:] == 0.0) and np.array_equal(zero[:, :, :2], got[:, :, :2])
    # a duplicated point: the pair's points 3 and 150 repeat the point that is closest in draw 0; the smaller index is reported
    ra, oa, rb, ob, pp = points(pb, [300], seed=22)
    at = drawsim.predict_draws(pb, par, *concat(ra, oa, rb, ob), seed=4, n_draws=1)
    k = int(prox_ref.proximity(at, model, d, pp)[0, 0, 1])
    for arr in (ra, oa, rb, ob):
        arr[150] = arr[k]; arr[3 if k != 3 else 4] = arr[k]
    at = drawsim.predict_draws(pb, par, *concat(ra, oa, rb, ob), seed=4, n_draws=1)
    got = twin.proximity(at, model, d, pp, [1.3])
    assert got[0, 0, 1] == min(k, 3 if k != 3 else 4) and np.array_equal(got, prox_ref.proximity(at, model, d, pp, [1.3]))


def test_a_first_row_query_makes_its_pair_nan_and_leaves_the_others():
    pb, par = small_problem("CTCRW", 2)
    ra, oa, rb, ob, pp = points(pb, [257, 40, 300], seed=23)
    clean = drawsim.predict_draws(pb, par, *concat(ra, oa, rb, ob), seed=4, n_draws=ND)
    # one more point in the first pair (its 258th: a second tile of one point) whose side B is a first row; such a query has no state
    # and enters no plan, so every other state of the call is what it was
    ra, oa = np.insert(ra, 257, ra[0]), np.insert(oa, 257, oa[0])
    rb, ob = np.insert(rb, 257, int(pb.seg_start[3])), np.insert(ob, 257, 0.1)
    pp2 = pp.copy(); pp2[1:] += 1
    at = drawsim.predict_draws(pb, par, *concat(ra, oa, rb, ob), seed=4, n_draws=ND)
    got = _both(at, "CTCRW", 2, pp2, RADII, None, "twin vs prox_ref: a first row")
    assert np.all(np.isnan(got[:, 0])) and np.all(np.isfinite(got[:, 1:]))
    was = twin.proximity(clean, "CTCRW", 2, pp, RADII)
    assert np.array_equal(got[:, 1:], was[:, 1:]) and np.all(np.isfinite(was))


def test_weights_of_1e_300_and_1e300_in_one_call():
    at, pp = _positions("OU_SSM", 2)
    w = np.where(np.arange(int(pp[-1])) % 2 == 0, 1e-300, 1e300)
    got = _both(at, "OU_SSM", 2, pp, RADII, w, "twin vs prox_ref: 1e-300 and 1e300")
    n_big = np.array([int(np.sum(w[a:b] == 1e300)) for a, b in zip(pp[1:-1], pp[2:])])
    e = prox_ref.quantum_exp(1e300, int(pp[-1]))
    assert np.array_equal(got[0, 1:, 4], [float(np.ldexp(float(n * prox_ref.quantise(1e300, e)), e)) for n in n_big])   # the small ones: 0 quanta
    tiny = _both(at, "OU_SSM", 2, pp, RADII, np.full(int(pp[-1]), 1e-300), "twin vs prox_ref: 1e-300 alone")
    assert np.all(tiny[:, 1:, 4] > 0.0)


def test_the_sanitizer_program_runs_clean():
    """tests/hostsim/prox_san: the plan and the twin's walk over the edge sizes, built with -fsanitize=address,undefined, run as a program"""
    twin.load()
    r = subprocess.run([twin.SAN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "prox_san ok" in r.stdout, (r.stdout, r.stderr)


def test_the_statistical_seed_passes_on_the_twin():
    """E dist^2 = |m_a - m_b|^2 + tr(V_a + V_b) on the position columns (the tracks are independent): the GPU suite's check, with the
    seed it uses, confirmed here first; the mean and covariance are the host twin's ssde_predict"""
    import predictsim_lib
    pb, par, rows, offs = stat_problem()
    at = drawsim.predict_draws(pb, par, rows, offs, seed=STAT_SEED, n_draws=STAT_DRAWS)
    got = twin.proximity(at, "CTCRW", 2, [0, 1])
    pred = predictsim_lib.predict(pb, par, rows, offs)
    ratio = stat_ratio(got[:, 0, 0], pred["mean"], pred["cov"])
    print(f"STAT proximity ratio {ratio:.3f}")
    assert np.all(got[:, 0, 1] == 0.0) and ratio <= 5.0
