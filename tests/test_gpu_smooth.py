"""GPU suite (-m gpu): ssde_smooth, the fixed-interval smoother of the Kalman families, against the numpy
reference smoother of tests/smooth_ref.py (itself checked against the joint Gaussian in test_smooth_host.py).

Tolerances: mean 1e-10 and covariance 1e-9 relative to the track's scale, whitened innovations 1e-10; NaN exactly where the
definitions put it."""
import ctypes as C

import numpy as np
import pytest

from cases import make_spec, problem_from_spec
from smooth_ref import smooth_ref
from smoothsde_amd import capi
from test_gpu_lattice import _par as _lat_par, lattice_tracks

pytestmark = pytest.mark.gpu

PATH_DENSE, PATH_TV = 2, 3


def _compare(got, ref, rows=None, cov=True):
    sel = slice(None) if rows is None else rows
    for key in (("mean", "cov", "resid") if cov else ("mean", "resid")):
        g, r = got[key][sel], ref[key][sel]
        assert np.array_equal(np.isnan(g), np.isnan(r)), key
        ok = ~np.isnan(r)
        if not ok.any():
            continue
        tol = {"mean": 1e-10 * (1.0 + np.max(np.abs(r[ok]))), "cov": 1e-9 * np.max(np.abs(r[ok])), "resid": 1e-10 * 10}[key]
        err = np.max(np.abs(g[ok] - r[ok]))
        assert err <= tol, (key, err, tol)


def _run(pb, par, **kw):
    eng = capi.Engine(pb, **kw)
    try:
        return eng.smooth(par), eng.info(), eng
    except Exception:
        eng.close()
        raise


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM", "BM_SSM"])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("grid", ["regular", "irregular"])
def test_parity_constant_coefficients(model, d, grid):
    irr = grid == "irregular"
    lengths = [40, 1, 33, 70, 12, 2] * 12
    n = sum(lengths)
    # NA rows, among them the last row of the first track
    spec = make_spec(f"gs_{model}_{d}_{grid}", model, d, seed=3 + d, lengths=lengths, irregular=irr, na_rows=(39, 45, 46, 300, n - 1))
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    _compare(got, smooth_ref(pb, spec["par"]))
    # consistency with the (verified) forward prediction: a track that ends in an NA row
    rep = eng.report(spec["par"])
    assert np.allclose(got["mean"][39], rep[38], rtol=0, atol=1e-10 * (1 + np.abs(rep[38]).max()))
    eng.close()
    ok = ~np.isnan(got["mean"][:, 0])
    pred = smooth_ref(pb, spec["par"])["pred_cov"]
    sdg, pdg = (np.diagonal(x[ok], axis1=1, axis2=2) for x in (got["cov"], pred))
    assert np.all(sdg <= pdg * (1 + 1e-9) + 1e-15) and np.all(sdg >= -1e-12)


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM", "BM_SSM"])
@pytest.mark.parametrize("d", [1, 2])
def test_parity_lattice_grid(model, d):
    # fixes missing from a regular schedule: the engine pads the tracks onto the lattice; outputs come back on the caller's rows
    ID, times, obs = lattice_tracks(model, d, [60, 45, 80, 33] * 20, 0.5, 0.15, seed=6 + d, na_frac=0.05)
    obs[59] = np.nan                                       # the first track ends in an NA row
    pb = capi.Problem(model, ID, times, obs)
    par = _lat_par(model, d, np.random.default_rng(d))
    got, info, eng = _run(pb, par)
    eng.close()
    assert info["n_rows_tiled"] > pb.n                     # laid out on the lattice
    _compare(got, smooth_ref(pb, par))


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM", "BM_SSM"])
@pytest.mark.parametrize("d", [1, 2])
def test_parity_per_row_H_and_general_P0(model, d):
    spec = make_spec(f"gsh_{model}_{d}", model, d, seed=21, lengths=[25, 60, 9, 1, 31] * 14, with_H=True, with_P0=True,
                     na_rows=(3, 24, 40, 41))
    pb = problem_from_spec(spec)
    got, _, eng = _run(pb, spec["par"])
    eng.close()
    _compare(got, smooth_ref(pb, spec["par"]))


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM", "BM_SSM"])
def test_parity_row_varying_dense_route(model):
    # row-varying tau / nu through streamed design columns, on the tiled dense_kernel route (SSDE_FLAG_FORCE_DENSE)
    spec = make_spec(f"gst_{model}", model, 2, seed=8, lengths=[30, 45, 17] * 30, variant="tv", na_rows=(5, 29, 77))
    pb = problem_from_spec(spec, flags=capi.FLAG_FORCE_DENSE)
    got, info, eng = _run(pb, spec["par"])
    eng.close()
    assert info["path"] == PATH_DENSE
    _compare(got, smooth_ref(pb, spec["par"]))


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM", "BM_SSM"])
def test_parity_row_varying_tv_route(model):
    # one long track with smooth parameters: the PATH_TV handle (the vignette's elephant-like case)
    spec = make_spec(f"gsv_{model}", model, 2, seed=9, lengths=[3000], variant="tv", na_rows=(10, 11, 2999))
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    eng.close()
    assert info["path"] == PATH_TV
    _compare(got, smooth_ref(pb, spec["par"]))


@pytest.mark.parametrize("d,coupled", [(3, False), (4, False), (3, True), (6, True)])
def test_parity_wide_responses(d, coupled):
    spec = make_spec(f"gsw_{d}_{coupled}", "CTCRW", d, seed=30 + d, lengths=[20, 35, 1, 14] * 5, with_H=coupled,
                     na_rows=(2, 19))
    pb = problem_from_spec(spec)
    got, _, eng = _run(pb, spec["par"])
    eng.close()
    _compare(got, smooth_ref(pb, spec["par"]))


def test_two_shard_parent():
    spec = make_spec("gs_shard", "CTCRW", 2, seed=41, lengths=[50, 31, 1, 64] * 40, na_rows=(49,))
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"], devices=[0, 0])
    eng.close()
    assert info["n_devices"] == 2
    _compare(got, smooth_ref(pb, spec["par"]))


def test_hygiene_and_errors():
    spec = make_spec("gs_hyg", "CTCRW", 2, seed=2, lengths=[80, 20, 40] * 30, na_rows=(7,))
    pb = problem_from_spec(spec)
    th, th2 = spec["par"], spec["par"] + 0.03
    eng = capi.Engine(pb)
    eng.eval(th, order=1)
    a = eng.smooth(th)
    b = eng.smooth(th)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    v, g = eng.eval(th2, order=1)
    fresh = capi.Engine(pb)
    vf, gf = fresh.eval(th2, order=1)
    fresh.close()
    assert v == vf and np.array_equal(g, gf)
    # smoothed variance never exceeds the predicted one
    ok = ~np.isnan(a["mean"][:, 0])
    assert np.all(np.diagonal(a["cov"][ok], axis1=1, axis2=2) <= np.diagonal(smooth_ref(pb, th)["pred_cov"][ok], axis1=1, axis2=2) * (1 + 1e-9))
    lib, h = eng.lib, eng._h
    p = np.ascontiguousarray(th)
    dp = p.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros(pb.n * pb.sdim)
    assert lib.ssde_smooth(h, dp, pb.n_par_full - 1, out.ctypes.data_as(C.POINTER(C.c_double)), None, None) == 1   # SSDE_ERR_ARG
    assert lib.ssde_smooth(h, dp, pb.n_par_full, None, None, None) == 1
    eng.close()
    for typ, d in (("OU", 1), ("BM", 2)):
        sp = make_spec(f"gs_direct_{typ}", typ, d, seed=4, lengths=[20, 30])
        pbd = problem_from_spec(sp)
        ed = capi.Engine(pbd)
        with pytest.raises(capi.EngineError) as ei:
            ed.smooth(sp["par"])
        assert ei.value.status == 2                                   # SSDE_ERR_MODEL
        ed.close()


def test_smoothed_variance_not_above_filter_prediction_and_report_tail():
    spec = make_spec("gs_tail", "OU_SSM", 2, seed=12, lengths=[30, 30], na_rows=(28, 29))
    pb = problem_from_spec(spec)
    got, _, eng = _run(pb, spec["par"])
    rep = eng.report(spec["par"])
    eng.close()
    # row 29: two NA rows at the end of the track; its state is the forward prediction from row 28's
    assert np.allclose(got["mean"][29], rep[28], rtol=0, atol=1e-10 * (1 + np.abs(rep[28]).max()))


def test_whitened_innovations_are_standard_normal():
    ID, times, obs = capi.simulate_device("CTCRW", 1000, 1000, 2, mu=0.0, tau=2.0, nu=1.0, sigma_obs=0.3, seed=17)
    pb = capi.Problem("CTCRW", ID.cpu().numpy(), times.cpu().numpy(), np.ascontiguousarray(obs.cpu().numpy()))
    par = np.array([np.log(0.3), 0.0, 0.0, np.log(2.0), np.log(1.0)])
    eng = capi.Engine(pb)
    e = eng.smooth(par, cov=False)["resid"]
    eng.close()
    e = e[~np.isnan(e[:, 0])]
    assert e.shape[0] >= 990_000
    assert np.all(np.abs(e.mean(axis=0)) < 5e-3), e.mean(axis=0)
    assert np.all(np.abs(e.var(axis=0) - 1.0) < 5e-3), e.var(axis=0)


def test_records_past_2_gib_and_chunking_is_bitwise():
    M, T = 1000, 10_000                                             # 10^7 rows: 2.48e9 bytes of CTCRW d = 2 records
    rng = np.random.default_rng(5)
    ID = np.repeat(np.arange(M, dtype=np.float64), T)
    times = np.tile(np.arange(T, dtype=np.float64), M)
    obs = np.cumsum(rng.standard_normal((M, T, 2)) * 0.5, axis=1).reshape(M * T, 2) + 3.0 * ID[:, None]
    par = np.array([np.log(0.2), 0.01, -0.02, np.log(3.0), np.log(0.8)])
    pb = capi.Problem("CTCRW", ID, times, np.ascontiguousarray(obs))
    eng = capi.Engine(pb)
    one = eng.smooth(par, cov=False)
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 400)                  # 16 groups of 159 MB each: 8 chunks
    many = eng.smooth(par, cov=False)
    eng.close()
    assert np.array_equal(one["mean"], many["mean"], equal_nan=True)
    assert np.array_equal(one["resid"], many["resid"], equal_nan=True)
    for k in (0, 1, 500, 937, M - 1):                               # first, middle and last wavefront groups
        r0, r1 = k * T, (k + 1) * T
        sub = capi.Problem("CTCRW", ID[r0:r1], times[r0:r1], np.ascontiguousarray(obs[r0:r1]))
        ref = smooth_ref(sub, par)
        _compare({"mean": one["mean"][r0:r1], "resid": one["resid"][r0:r1]}, ref, cov=False)
