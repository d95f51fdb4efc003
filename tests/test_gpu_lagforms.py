"""GPU suite: the bulk's forms computed on the host and handed BY VALUE to the reducing launch (DESIGN.md §3.3d;
ssde_lagforms.hpp).  Batches as in test_gpu_lagstats.py, the path forced with SSDE_LAGSTATS=2.

1. Nothing of the forms lives in a device buffer the evaluations of a handle share: four asynchronous evaluations at four thetas,
   in flight together on one stream, each give bitwise what a synchronous evaluation at their theta gives on a second engine.
2. The path's arithmetic is what ssde_lagforms_host exports: its accumulator for the engine's own statistics, added to the streamed
   head (the batch cut to the rows before the bulk) and the bulk rows' log-determinant term, reproduces the engine's value.
3. A theta near the slow-forgetting end of what the path still takes (a cut within 32 taps of the longest the statistics hold)
   agrees with the streamed evaluation."""
import numpy as np
import pytest

from smoothsde_amd import capi
from test_gpu_lagstats import _batch, _close, _engine, _theta

pytestmark = pytest.mark.gpu


def test_four_asynchronous_evaluations_in_flight_match_synchronous_ones_bitwise(monkeypatch):
    import torch
    host, dd = _batch(M=1000, T=4500, d=2, seed=12, free_mu=True)
    eng = _engine(dd, monkeypatch)
    ref = _engine(dd, monkeypatch)
    thetas = [_theta(eng.n_par_full, 2, k) for k in range(4)]
    for k in (1, 3):
        thetas[k][0] += 0.3 * k                    # (different cuts among the four, not only different taps)
    outs = [torch.zeros(2 + eng.n_par_full, dtype=torch.float64, device="cuda:0") for _ in thetas]
    st = torch.cuda.Stream()
    for th, o in zip(thetas, outs):
        eng.eval_device(th, o.data_ptr(), order=1, stream=st.cuda_stream)
    st.synchronize()
    assert eng.info()["lagstat_rows"] > 0
    for th, o in zip(thetas, outs):
        r = o.cpu().numpy()
        v, g = ref.eval(th)
        assert ref.info()["lagstat_rows"] > 0
        pv, pg = ref.penalty(th)
        assert r[0] + pv == v and np.array_equal(r[1:-1] + pg, g), (r, v, g)
        assert r[-1] == ref.info()["window_check"] <= capi.WINDOW_TOL


def _stationary_log_f(theta, d, dt):
    """log F of the stationary CTCRW filter (F = P11 + sigma_obs^2, P the predicted covariance): the covariance recursion of the model
    on a regular grid, iterated until it stops moving"""
    h = np.exp(theta[0]) ** 2
    tau, nu = np.exp(theta[1 + d]), np.exp(theta[2 + d])
    e = np.exp(-dt / tau)
    A = 4.0 * nu * nu / np.pi
    T = np.array([[1.0, (1.0 - e) * tau], [0.0, e]])
    Q = np.array([[A * tau * (dt - 2.0 * (1.0 - e) * tau + 0.5 * tau * (1.0 - e * e)), 0.5 * A * tau * (1.0 - e) ** 2],
                  [0.5 * A * tau * (1.0 - e) ** 2, 0.5 * A * (1.0 - e * e)]])
    P = np.eye(2)
    for _ in range(20000):
        F = P[0, 0] + h
        K = P[:, :1] / F
        Pn = T @ (P - K @ P[:1, :]) @ T.T + Q
        done = np.max(np.abs(Pn - P)) <= 1e-16 * np.max(np.abs(Pn))
        P = Pn
        if done:
            break
    return np.log(P[0, 0] + h)


@pytest.mark.parametrize("d", [2, 1])
def test_host_forms_plus_the_streamed_head_reproduce_the_engine_value(d, monkeypatch):
    M_tracks, T = 1000, 4500
    host, dd = _batch(M=M_tracks, T=T, d=d, seed=13 + d, free_mu=True)
    lag = _engine(dd, monkeypatch)
    Ms, ss, n_bulk = lag.lagstats()
    first_bulk = capi.lagstats_host([np.zeros((1, d))])[3]
    # the head alone: every track cut to its first observation and the first_bulk scored rows after it, streamed
    ID, times, obs, fixed = dd
    idh, th_, yh = ID.cpu().numpy(), times.cpu().numpy(), obs.cpu().numpy()
    assert len(idh) == M_tracks * T and n_bulk == M_tracks * (T - 1 - first_bulk)
    keep = (np.arange(len(idh)) % T) <= first_bulk
    dt = float(th_[1] - th_[0])
    with monkeypatch.context() as m:
        m.setenv("SSDE_LAGSTATS", "0")
        head = capi.Engine(capi.Problem("CTCRW", idh[keep], th_[keep], yh[keep], par_fixed=fixed))
    for k in range(3):
        theta = _theta(lag.n_par_full, d, k)
        v, g = lag.eval(theta)
        inf = lag.info()
        assert inf["lagstat_rows"] == n_bulk
        vh, _ = head.eval(theta)
        assert head.info()["lagstat_rows"] == 0
        f = capi.lagforms_host(Ms, ss, n_bulk, theta, dt, inf["window"])
        assert f["chk"] <= capi.WINDOW_TOL
        total = vh + f["acc"][0] + 0.5 * d * _stationary_log_f(theta, d, dt) * n_bulk
        print("d=%d theta %d: K=%d engine %.15g head + forms %.15g rel %.3e" % (d, k, inf["window"], v, total, abs(total - v) / abs(v)))
        assert abs(total - v) <= 1e-12 * abs(v), (v, total, vh, f["acc"][0])


def test_a_cut_near_the_longest_the_statistics_hold_agrees_with_streaming(monkeypatch):
    """The sweep of test_a_theta_whose_cut_exceeds_the_statistics_streams_every_row, stopped at the last log sigma_obs whose cut still
    fits: both engines walk the same thetas; the grid is refined by bisection between the last theta that fits and the first that
    does not until the cut is within 32 taps of the longest."""
    host, dd = _batch(M=1000, T=4500, d=2, seed=7, free_mu=True)
    lag = _engine(dd, monkeypatch)
    ref = _engine(dd, monkeypatch, lagstats=0)
    n_taps = capi.lagstats_host([np.zeros((1, 2))])[0].shape[0]
    th = _theta(lag.n_par_full, 2, 1)

    def both(ls):
        th[0] = ls
        vr, gr = ref.eval(th)
        v, g = lag.eval(th)
        return ref.info()["window"], lag.info(), (v, g, vr, gr)

    lo = hi = None
    best = None
    for ls in np.linspace(np.log(0.1), np.log(20.0), 40):
        w, inf, res = both(ls)
        if w >= n_taps:
            hi = ls
            break
        lo, best = ls, (w, inf, res)
    assert lo is not None and hi is not None
    for _ in range(12):
        if best[0] >= n_taps - 1 - 32:
            break
        mid = 0.5 * (lo + hi)
        w, inf, res = both(mid)
        if w >= n_taps:
            hi = mid
        else:
            lo, best = mid, (w, inf, res)
    w, inf, (v, g, vr, gr) = best
    print("largest cut that fits: K=%d at log sigma_obs=%.4f, lagstat_rows=%d, check %.3e" % (w, lo, inf["lagstat_rows"], inf["window_check"]))
    assert n_taps - 1 - 32 <= w <= n_taps - 1, w
    # (the path's own "window" is the head's plan: with a cut this long its 256 rows are one window)
    assert inf["lagstat_rows"] > 0 and inf["window_check"] <= capi.WINDOW_TOL, inf
    _close(g, gr, v, vr)
