"""GPU suite: ssde_simulate_rows (csrc/k_sim_rows.hip; include/ssde.h) against its numpy definition
(tests/simrows_ref.py) on the cases of tests/simrows_cases.py, its bitwise invariances, ssde_simulate's batch at replicate 0, a
blown-up parameter, and SDE.simulate / SDE.check_post on two small fits.

Limits (simrows_cases.compare): obs within 1e-9 (1 + max|ref|) -- the bound tests/sim_ref.py records for device against numpy
log / sincos on tracks of this length; every case keeps |y| <= 1e3 --, the sums of stats within that bound times the track's rows,
max L within the obs bound, counts exact (no reference step length lies within 1e-6 (1 + thr) of a threshold), NaN patterns
identical.  Every comparison prints its largest gap over its limit."""
from fractions import Fraction

import numpy as np
import pytest

from simrows_cases import CASES, case, compare, limits, reference
from simrows_ref import n_par
from smoothsde_amd import capi

pytestmark = pytest.mark.gpu


def _gpu(c, **over):
    kw = dict(sigma_obs=c["sigma_obs"], z0=c["z0"], seed=c["seed"], rep0=c["rep0"], n_rep=c["n_rep"], thresholds=c["thr"])
    kw.update(over)
    coeff = kw.pop("coeff", c["coeff"])
    return capi.simulate_rows(c["model"], c["n_dim"], kw.pop("row0", c["row0"]), kw.pop("times", c["times"]), kw.pop("X_fe", c["X_fe"]),
                              kw.pop("X_re", c["X_re"]), c["link"], coeff, **kw)


def _same(a, b, names=None):
    for k in (names or a.keys()):
        x, y = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (a[k], b[k]))
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_definition(name):
    c = case(name)
    compare(_gpu(c), reference(name), c, name)


# ---- bitwise invariances: one larger problem, simulated once ------------------------------------------------------------------------
def _wide_case():
    """CTCRW, two columns, tracks of 2000, 0 and 3000 rows, 70 replicates with a coefficient row each, tau smooth, nu linear: 80 kB of
    obs per replicate, so a budget of 1 MiB makes batches of 12 replicates"""
    from smoothsde_amd.synth import bspline_basis
    rng = np.random.default_rng(70)
    n, R = 5000, 70
    times = np.cumsum(rng.uniform(0.1, 1.5, size=n))
    X_fe = [None, None, None, np.column_stack([np.ones(n), np.sin(0.01 * np.arange(n))])]
    X_re = [None, None, bspline_basis((np.sin(0.003 * np.arange(n)) + 1) / 2, 9), None]
    chat = np.concatenate([[0.05, -0.03], [0.3], rng.uniform(-0.5, 0.5, 9), [-0.2, 0.3]])
    coeff = chat[None, :] + 0.1 * rng.standard_normal((R, len(chat)))
    return dict(model="CTCRW", n_dim=2, row0=np.array([0, 2000, 2000, 5000]), times=times, X_fe=X_fe, X_re=X_re,
                link=np.array([0, 0, 1, 1], dtype=np.uint8), coeff=coeff, sigma_obs=np.linspace(0.0, 0.2, R), z0=np.array([1.0, -1.0]),
                seed=99, rep0=3, n_rep=R, thr=np.array([0.5, 2.0]))


@pytest.fixture(scope="module")
def wide():
    c = _wide_case()
    return c, _gpu(c)


def test_bitwise_small_budget(wide):
    c, whole = wide
    _same(whole, _gpu(c, budget_mb=1))


def test_bitwise_each_output_alone(wide):
    c, whole = wide
    _same(_gpu(c, want=("stats",)), whole, ("stats",))
    _same(_gpu(c, want=("obs",)), whole, ("obs",))


def test_bitwise_a_replicate_range_cut_over_two_calls(wide):
    c, whole = wide
    a = _gpu(c, coeff=c["coeff"][:41], sigma_obs=c["sigma_obs"][:41], n_rep=41)
    b = _gpu(c, coeff=c["coeff"][41:], sigma_obs=c["sigma_obs"][41:], rep0=c["rep0"] + 41, n_rep=29)
    for k in ("obs", "stats"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k], equal_nan=True), k


def test_bitwise_a_track_alone_with_its_ordinal(wide):
    """track 2 without the others: rows 2000 .. 4999 of the times and the blocks, behind two empty tracks that keep its ordinal"""
    c, whole = wide
    rows = slice(2000, 5000)
    alone = _gpu(c, row0=np.array([0, 0, 0, 3000]), times=c["times"][rows], X_fe=[None if b is None else b[rows] for b in c["X_fe"]],
                 X_re=[None if b is None else b[rows] for b in c["X_re"]])
    assert np.array_equal(alone["obs"], whole["obs"][:, rows, :])
    assert np.array_equal(alone["stats"][:, 2, :], whole["stats"][:, 2, :]) and np.isnan(alone["stats"][:, :2, :]).all()


def test_bitwise_device_out_and_device_data(wide):
    import torch
    c, whole = wide
    dev = _gpu(c, device_out=True)
    assert dev["obs"].is_cuda and not hasattr(dev["stats"], "is_cuda")
    _same(dev, whole)
    t = lambda b: None if b is None else torch.as_tensor(b, device="cuda")
    _same(_gpu(c, X_fe=[t(b) for b in c["X_fe"]], X_re=[t(b) for b in c["X_re"]]), whole)


def _fma_sq(d, acc):
    """fma(d, d, acc) rounded once"""
    return float(Fraction(d) * Fraction(d) + Fraction(acc))


@pytest.mark.parametrize("name", ["ctcrw_smooth_d2", "bm_d3", "ou_const_d1"])
def test_stats_are_those_of_the_calls_own_obs(name):
    """the statistics recomputed from the same call's obs_rep: L by the definition's fma chain (exact rational arithmetic, rounded
    once per fma), so max L and the counts must be exact; the sums in numpy's order, held to the bound of the comparison"""
    c = case(name)
    got = _gpu(c)
    d, thr = c["n_dim"], c["thr"]
    lim, lim_t = limits(c, reference(name))
    for t in range(len(c["row0"]) - 1):
        r0, r1 = int(c["row0"][t]), int(c["row0"][t + 1])
        if r1 - r0 < 2:
            assert np.isnan(got["stats"][:, t, :]).all()
            continue
        D = np.diff(got["obs"][:, r0:r1, :], axis=1)
        L = np.empty(D.shape[:2])
        for k in range(D.shape[0]):
            for i in range(D.shape[1]):
                q = D[k, i, 0] * D[k, i, 0]
                for cc in range(1, d):
                    q = _fma_sq(D[k, i, cc], q)
                L[k, i] = np.sqrt(q)
        st = got["stats"][:, t, :]
        assert np.array_equal(st[:, 3 * d + 1], L.max(axis=1)), (name, t)
        for r, th in enumerate(thr):
            assert np.array_equal(st[:, 3 * d + 2 + r], np.sum(L <= th, axis=1)), (name, t, r)
        assert np.max(np.abs(st[:, 3 * d] - L.sum(axis=1))) <= lim_t[t]
        for cc in range(d):
            assert np.max(np.abs(st[:, 3 * cc] - D[:, :, cc].sum(axis=1))) <= lim_t[t]
            assert np.max(np.abs(st[:, 3 * cc + 1] - (D[:, :, cc] ** 2).sum(axis=1))) <= lim_t[t]
            assert np.max(np.abs(st[:, 3 * cc + 2] - (D[:, 1:, cc] * D[:, :-1, cc]).sum(axis=1))) <= lim_t[t]


# ---- the other simulator, a blown-up parameter --------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["CTCRW", "OU", "OU_SSM", "BM", "BM_SSM"])
def test_replicate_zero_is_ssde_simulates_batch(model):
    """intercept-only blocks, a regular grid, replicate number 0, 70 tracks of 64 rows: ssde_simulate's batch for the seed to
    1e-10 (1 + max|y|) -- the factors are formed per row with expm1 here, once with 1 - exp there; a wrong stream or counter
    assignment is off by O(1)"""
    M, T, d, dt = 70, 64, 2, 0.7
    p = dict(mu=[0.3, -0.2], tau=1.5, nu=0.8, kappa=0.6, sigma=0.9, sigma_obs=0.1)
    _, _, obs = capi.simulate_device(model, M, T, d, dt=dt, z0=[0.5, -1.0], seed=4242, **p)
    obs = obs.cpu().numpy()
    q = n_par(model, d)
    p1, p2 = (p["sigma"], None) if q == d + 1 else (p["tau"], p["nu"] if model == "CTCRW" else p["kappa"])
    coeff = np.array([p["mu"] + [np.log(p1)] + ([np.log(p2)] if p2 else [])])
    with_error = model in ("CTCRW", "OU_SSM", "BM_SSM")
    got = capi.simulate_rows(model, d, np.arange(M + 1) * T, np.tile(dt * np.arange(1, T + 1), M), [None] * q, [None] * q,
                             [0] * d + [1] * (q - d), coeff, sigma_obs=0.1 if with_error else None, z0=[0.5, -1.0], seed=4242)["obs"][0]
    gap, big = np.max(np.abs(got - obs)), np.max(np.abs(obs))
    print(f"simrows against ssde_simulate, {model}: gap {gap:.3g}, limit {1e-10 * (1 + big):.3g}")
    assert gap <= 1e-10 * (1.0 + big)


@pytest.mark.parametrize("name", ["bm_d3", "ctcrw_smooth_d2", "ou_ssm_smooth"])
def test_a_blown_up_parameter_is_nan_in_its_replicate_alone(name):
    """a log-link linear predictor of 800 in replicate 5's coefficient row (the intercept of the last parameter): exp overflows, and
    every statistic of every track of two or more rows is NaN for that replicate; the others are bitwise what they were"""
    c = case(name)
    clean = _gpu(c)
    coeff = c["coeff"].copy()
    K_last = (1 if c["X_fe"][-1] is None else c["X_fe"][-1].shape[1]) + (0 if c["X_re"][-1] is None else c["X_re"][-1].shape[1])
    coeff[5, coeff.shape[1] - K_last] = 800.0
    got = _gpu(c, coeff=coeff)
    assert np.isnan(got["stats"][5]).all()
    keep = [k for k in range(c["n_rep"]) if k != 5]
    assert np.array_equal(got["stats"][keep], clean["stats"][keep], equal_nan=True)
    assert np.array_equal(got["obs"][keep], clean["obs"][keep])


# ---- SDE.simulate / SDE.check_post ----------------------------------------------------------------------------------------------------
def _fit(model):
    from smoothsde_amd.sde import SDE
    from smoothsde_amd.synth import simulate
    if model == "CTCRW":
        ID, times, obs = simulate("CTCRW", 3, 120, 2, tau=2.0, nu=1.5, sigma_obs=0.1, seed=21)
        data = dict(ID=ID, time=times, z0=obs[:, 0], z1=obs[:, 1])
        sde = SDE(formulas={"mu1": "~1", "mu2": "~1", "tau": "~1", "nu": "~1"}, data=data, type="CTCRW", response=["z0", "z1"],
                  par0=[0, 0, 1, 1], fixpar=["mu1", "mu2"])
    else:
        ID, times, obs = simulate("OU", 3, 120, 1, mu=1.0, tau=2.0, kappa=1.0, seed=22)
        data = dict(ID=ID, time=times, z=obs[:, 0])
        sde = SDE(formulas={"mu": "~1", "tau": "~1", "kappa": "~1"}, data=data, type="OU", response="z", par0=[0.5, 1, 1])
    sde.fit(maxiter=60)
    return sde


@pytest.fixture(scope="module", params=["CTCRW", "OU"])
def fitted(request):
    return _fit(request.param)


def test_sde_simulate(fitted):
    sde = fitted
    n, d = sde.n_, len(sde.response())
    a, b, c = sde.simulate(seed=5), sde.simulate(seed=5), sde.simulate(seed=6)
    assert a.shape == (n, d) and np.isfinite(a).all() and np.array_equal(a, b) and not np.array_equal(a, c)
    p = sde.simulate(seed=5, posterior=True)
    assert p.shape == (n, d) and np.array_equal(p, sde.simulate(seed=5, posterior=True)) and not np.array_equal(p, a)
    # new rows: one track of 50 rows on another grid
    from smoothsde_amd.sde import Design
    new = sde.simulate(z0=2.0, seed=5, designs=[Design() for _ in sde.names_], ID=np.zeros(50), time=np.cumsum(np.full(50, 0.5)))
    assert new.shape == (50, d) and np.isfinite(new).all()
    if sde.type() == "OU":
        assert np.all(new[0] == 2.0)                         # no observation error: the first row is z0


def test_sde_check_post(fitted):
    sde = fitted
    d = len(sde.response())
    out = sde.check_post(n_sims=200, seed=3, thresholds=[1.0])
    n_stat = 3 * d + 2 + 1
    assert out["stats"].shape == (n_stat, 200) and out["obs_stat"].shape == (n_stat,) and len(out["names"]) == n_stat
    assert np.isfinite(out["stats"]).all() and np.isfinite(out["obs_stat"]).all()
    again = sde.check_post(n_sims=200, seed=3, thresholds=[1.0])
    assert np.array_equal(again["stats"], out["stats"]) and np.array_equal(again["obs_stat"], out["obs_stat"])
    lo, hi = out["stats"].min(axis=1), out["stats"].max(axis=1)
    for k, nm in enumerate(out["names"]):
        print(f"check_post {sde.type()} {nm}: obs {out['obs_stat'][k]:.4g}, replicates {lo[k]:.4g} .. {hi[k]:.4g}")
    inside = (out["obs_stat"] >= lo) & (out["obs_stat"] <= hi)
    assert inside.all(), [nm for nm, ok in zip(out["names"], inside) if not ok]
    # a callable sees (ID, time, obs) of every replicate: the built-in mean step length, recomputed from the replicates
    row0 = np.r_[0, np.arange(120, 361, 120)]

    def fn(ID, time, obs):
        L = np.concatenate([np.sqrt(np.sum(np.diff(obs[row0[t]:row0[t + 1]], axis=0) ** 2, axis=1)) for t in range(3)])
        return [L.mean(), L.max()]
    mine = sde.check_post(check_fn=fn, n_sims=200, seed=3, budget_mb=1)            # (1 MiB: two batches of replicates)
    assert mine["stats"].shape == (2, 200)
    assert np.allclose(mine["stats"], out["stats"][3 * d:3 * d + 2], rtol=1e-12, atol=0)
    assert np.allclose(mine["obs_stat"], out["obs_stat"][3 * d:3 * d + 2], rtol=1e-12, atol=0)
