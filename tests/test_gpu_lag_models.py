"""GPU suite: OU_SSM and BM_SSM with the rows past the first LAG_A rows of every track taken from lag statistics built at create
(the scalar-family forms; OU_SSM from the statistics of the levels y - ref, BM_SSM from those of the increments).

Small batches (about 200 tracks x 900 rows: 4 groups, the last one partial), the path forced with SSDE_LAGSTATS=2 -- no crossover has
been measured for these models, the dispatch rule builds nothing for them unforced.  Compared with the same batch streamed row by
row (SSDE_LAGSTATS=0: value 1e-12 relative, gradient 1e-10 of its max-norm, the limits of tests/test_gpu_lagstats.py) and with the
oracle (1e-10 / 1e-8).  Every theta of the parity cases keeps sigma_obs <= 0.5 x the process scale: the cut stays below 80 taps and
the evaluation takes the path (asserted: no case may fall back)."""
import os

import numpy as np
import pytest

from smoothsde_amd import capi

pytestmark = pytest.mark.gpu
K_ISO_SHARED = 3
THREADS = min(16, os.cpu_count() or 8)
M_TRACKS, T_ROWS = 200, 900
SIM = dict(OU_SSM=dict(mu=1.0, tau=2.0, kappa=1.0, sigma_obs=0.1), BM_SSM=dict(mu=0.2, sigma=1.0, sigma_obs=0.1))


def _batch(model, d, seed, ragged=False, free_mu=False, lengths=None, flags=0):
    import torch
    dev = torch.device("cuda:0")
    M, T = M_TRACKS, T_ROWS
    if ragged:
        lengths = np.random.default_rng(seed).integers(T // 2, T + 1, size=M).astype(np.int64)
    if lengths is not None:
        M, T = len(lengths), int(np.max(lengths))
    ID, times, obs = capi.simulate_device(model, M, T, d, seed=seed, track0=0, lengths=lengths, device=dev, **SIM[model])
    q = capi.n_sde_par(model, d)
    fixed = np.zeros(1 + q, dtype=np.uint8)
    if not free_mu:
        fixed[1:1 + d] = 1
    host = capi.Problem(model, ID.cpu().numpy(), times.cpu().numpy(), obs.cpu().numpy(), par_fixed=fixed, flags=flags)
    return host, (model, ID, times, obs, fixed)


def _env(monkeypatch, lagstats):
    if lagstats is not None:
        monkeypatch.setenv("SSDE_LAGSTATS", str(lagstats))
    else:
        monkeypatch.delenv("SSDE_LAGSTATS", raising=False)


def _engine(dev_data, monkeypatch, lagstats=2):
    """lagstats: 2 = the statistics whatever the dispatch rule says, 0 = none, None = the rule"""
    model, ID, times, obs, fixed = dev_data
    with monkeypatch.context() as m:
        _env(m, lagstats)
        return capi.Engine(capi.Problem.from_torch(model, ID, times, obs, par_fixed=fixed))


def _host_engine(host, monkeypatch, lagstats=2, devices=None):
    with monkeypatch.context() as m:
        _env(m, lagstats)
        return capi.Engine(host, devices=devices)


def _theta(model, d, k, log_tau=np.log(2.0)):
    """sigma_obs = 0.1 x the process scale (sqrt(kappa) = 1, sigma = 1), the other entries near what the data were simulated with"""
    if model == "OU_SSM":
        th = np.array([np.log(0.1)] + [1.0] * d + [log_tau, 0.0])
    else:
        th = np.array([np.log(0.1)] + [0.2] * d + [0.0])
    return th + 0.01 * np.sin(np.arange(th.size) + 0.7 * k)


def _close(a, b, va, vb, rv=1e-12, rg=1e-10):
    assert abs(va - vb) <= rv * abs(vb), (va, vb)
    assert np.max(np.abs(a - b)) <= rg * np.max(np.abs(b)), (a, b)


@pytest.mark.parametrize("ragged", [False, True], ids=["equal", "ragged"])
@pytest.mark.parametrize("free_mu", [False, True], ids=["mu_fixed", "mu_free"])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("model", ["OU_SSM", "BM_SSM"])
def test_bulk_from_lag_statistics_against_streaming_and_the_oracle(model, d, free_mu, ragged, monkeypatch):
    from oracle_lib import oracle_eval
    host, dd = _batch(model, d, seed=30 + d, ragged=ragged, free_mu=free_mu)
    lag = _engine(dd, monkeypatch)
    ref = _engine(dd, monkeypatch, lagstats=0)
    assert lag.info()["n_groups"] == 4
    for k in range(3):
        th = _theta(model, d, k)
        v, g = lag.eval(th)
        inf = lag.info()
        assert inf["lagstat_rows"] > 0, inf
        assert inf["kernel_id"] == K_ISO_SHARED, inf
        assert inf["main_kernel_rows"] + inf["lagstat_rows"] == inf["n_steps"], inf
        assert inf["window_check"] <= capi.WINDOW_TOL, inf
        vr, gr = ref.eval(th)
        assert ref.info()["lagstat_rows"] == 0
        print("%s d=%d k=%d: value %.3e gradient %.3e check %.3e" % (model, d, k, abs(v - vr) / abs(vr), np.max(np.abs(g - gr)) / np.max(np.abs(gr)),
                                                                   inf["window_check"]))
        _close(g, gr, v, vr)
        ov, og = oracle_eval(host, th, order=1, threads=THREADS)
        assert abs(v - ov) <= 1e-10 * abs(ov), (v, ov)
        assert np.max(np.abs(g - og)) <= 1e-8 * np.max(np.abs(og)), (g, og)
        fixed = host.par_fixed != 0
        assert np.all(g[fixed] == 0.0)
        if free_mu:
            assert np.all(g[1:1 + d] != 0.0)
    lag.close(); ref.close()


@pytest.mark.parametrize("model", ["OU_SSM", "BM_SSM"])
def test_a_theta_whose_cut_exceeds_the_statistics_streams_every_row(model, monkeypatch):
    """Noisier fixes make the filter forget more slowly: the first log sigma_obs on a grid whose own plan asks for a warm-up beyond the
    taps the statistics hold runs the streaming path, reports no bulk rows and computes bitwise what the streaming engine computes; a
    theta before it takes the bulk from the statistics.  (OU_SSM forgets at least like e^{-dt / tau}: the walk runs at tau = 200 dt,
    where a noisy fix does ask for that many rows.)"""
    host, dd = _batch(model, 2, seed=37, free_mu=True)
    lag = _engine(dd, monkeypatch)
    ref = _engine(dd, monkeypatch, lagstats=0)
    n_taps = capi.lagstats_host([np.zeros((1, 2))])[0].shape[0]
    th = _theta(model, 2, 1, log_tau=np.log(200.0))
    took_bulk = False
    for ls in np.linspace(np.log(0.1), np.log(20.0), 40):         # (both engines walk the same thetas: the same window policy history)
        th[0] = ls
        vr, gr = ref.eval(th)
        v, g = lag.eval(th)
        w, inf = ref.info()["window"], lag.info()
        if w >= n_taps:
            break
        if inf["lagstat_rows"] > 0:
            took_bulk = True
            _close(g, gr, v, vr)
    else:
        pytest.fail("no sigma_obs on the grid asks for a warm-up of %d rows or more" % n_taps)
    assert took_bulk
    assert inf["lagstat_rows"] == 0 and inf["window"] == w and inf["window_check"] <= capi.WINDOW_TOL, inf
    assert v == vr and np.array_equal(g, gr)
    lag.close(); ref.close()


def _tiled_tracks(ID, obs):
    idh, yh = ID.cpu().numpy(), obs.cpu().numpy()
    starts = np.flatnonzero(np.r_[True, idh[1:] != idh[:-1]])
    ends = np.r_[starts[1:], len(idh)]
    return [yh[a + 1:b] for a, b in zip(starts, ends)]            # tiled row t of a track = its row t + 1 (the scored rows)


@pytest.mark.parametrize("model", ["OU_SSM", "BM_SSM"])
def test_short_tracks_in_the_last_group_and_the_device_statistics_against_the_host_reference(model, monkeypatch):
    """Groups are sorted longest first: the last one holds only tracks of 40-180 rows, which the statistics leave alone.  The device's
    M, s and n match the host reference on the same tiled rows -- every lag and both end corrections -- with the handle's own ref;
    BM_SSM's are bitwise those of a CTCRW handle on the same rows."""
    d = 2
    rng = np.random.default_rng(41)
    lengths = np.concatenate([rng.integers(500, 901, size=160), rng.integers(40, 181, size=64)]).astype(np.int64)
    rng.shuffle(lengths)
    host, dd = _batch(model, d, seed=42, free_mu=True, lengths=lengths)
    lag = _engine(dd, monkeypatch)
    ref = _engine(dd, monkeypatch, lagstats=0)
    assert lag.info()["lagstat_create_ms"] > 0.0 and ref.info()["lagstat_create_ms"] == 0.0
    for k in range(2):
        th = _theta(model, d, k)
        v, g = lag.eval(th)
        assert lag.info()["lagstat_rows"] > 0
        vr, gr = ref.eval(th)
        _close(g, gr, v, vr)
    Md, sd, nd = lag.lagstats()
    rf = lag.lagstats_ref()
    assert ref.lagstats() is None and ref.lagstats_ref() is None and rf.shape == (2,)
    tracks = _tiled_tracks(dd[1], dd[3])
    if model == "OU_SSM":
        assert np.all(rf != 0.0) and any(np.array_equal(rf, y[255]) for y in tracks if y.shape[0] > 256)     # one observation, row LAG_A - 1
    else:
        assert np.all(rf == 0.0)
    Mh, sh, nh, _ = capi.lagstats_host(tracks, model=model, ref=rf)
    assert nd == nh == float(np.sum(np.maximum(lengths - 1 - 256, 0)))
    eM, es = np.max(np.abs(Md - Mh)) / np.max(np.abs(Mh)), np.max(np.abs(sd - sh)) / np.max(np.abs(sh))
    print("%s: M %.3e s %.3e" % (model, eM, es))
    assert eM <= 1e-12 and es <= 1e-12
    if model == "BM_SSM":
        _, ID, times, obs, fixed = dd
        with monkeypatch.context() as m:
            m.setenv("SSDE_LAGSTATS", "2")
            ct = capi.Engine(capi.Problem.from_torch("CTCRW", ID, times, obs))
        Mc, sc, nc = ct.lagstats()
        assert nc == nd and np.array_equal(Mc, Md) and np.array_equal(sc, sd)
        ct.close()
    lag.close(); ref.close()


@pytest.mark.parametrize("model", ["OU_SSM", "BM_SSM"])
def test_determinism_and_the_other_evaluation_forms(model, monkeypatch):
    """Two creates are bitwise equal; SSDE_FUSED_FINALIZE=1 is bitwise the two-launch form, check value included; ssde_eval_device
    calls queued on one stream give the synchronous results; a two-shard handle (each shard its own statistics and ref) agrees."""
    import torch
    d = 2
    host, dd = _batch(model, d, seed=45, free_mu=True)
    a = _engine(dd, monkeypatch)
    b = _engine(dd, monkeypatch)
    monkeypatch.setenv("SSDE_FUSED_FINALIZE", "1")
    one = _engine(dd, monkeypatch)
    monkeypatch.delenv("SSDE_FUSED_FINALIZE")
    thetas = [_theta(model, d, k) for k in range(4)]
    sync = []
    for th in thetas:
        va, ga = a.eval(th)
        vb, gb = b.eval(th)
        v1, g1 = one.eval(th)
        ia, i1 = a.info(), one.info()
        assert ia["lagstat_rows"] > 0 and b.info()["lagstat_rows"] > 0 and i1["lagstat_rows"] > 0
        assert va == vb and np.array_equal(ga, gb)
        assert v1 == va and np.array_equal(g1, ga)
        assert i1["window_check"] == ia["window_check"] <= capi.WINDOW_TOL
        sync.append((va, ga))
    assert np.array_equal(a.lagstats()[0], b.lagstats()[0]) and np.array_equal(a.lagstats()[1], b.lagstats()[1])
    assert np.array_equal(a.lagstats_ref(), b.lagstats_ref())
    # four evaluations queued on one stream, read once
    n = a.n_par_full
    outs = torch.zeros((4, 2 + n), dtype=torch.float64, device="cuda:0")
    s = torch.cuda.Stream()
    for k, th in enumerate(thetas):
        a.eval_device(th, outs[k].data_ptr(), order=1, stream=s.cuda_stream)
    s.synchronize()
    res = outs.cpu().numpy()
    for k, th in enumerate(thetas):
        pv, pg = a.penalty(th)
        assert res[k, -1] <= capi.WINDOW_TOL
        _close(res[k, 1:-1] + pg, sync[k][1], res[k, 0] + pv, sync[k][0], rv=1e-12, rg=1e-11)
    # a sharded handle
    sh = _host_engine(host, monkeypatch, devices=[0, 0])
    for k, th in enumerate(thetas[:2]):
        vs, gs = sh.eval(th)
        inf = sh.info()
        assert inf["n_devices"] == 2 and inf["lagstat_rows"] > 0, inf
        assert inf["main_kernel_rows"] + inf["lagstat_rows"] == inf["n_steps"], inf
        _close(gs, sync[k][1], vs, sync[k][0], rv=1e-12, rg=1e-12)
    for e in (a, b, one, sh):
        e.close()


@pytest.mark.parametrize("model", ["OU_SSM", "BM_SSM"])
def test_dispatch(model, monkeypatch):
    """Unforced, these small batches build nothing; ssde_hess and ssde_report on a forced handle stream every row and agree with an
    unforced handle's."""
    d = 2
    host, dd = _batch(model, d, seed=47, free_mu=True, flags=capi.FLAG_EXACT_HESS)
    rule = _engine(dd, monkeypatch, lagstats=None)
    th = _theta(model, d, 0)
    rule.eval(th)
    inf = rule.info()
    assert inf["lagstat_rows"] == 0 and inf["lagstat_create_ms"] == 0.0 and rule.lagstats() is None, inf
    rule.close()
    forced = _host_engine(host, monkeypatch, lagstats=2)
    plain = _host_engine(host, monkeypatch, lagstats=None)
    v, g = forced.eval(th)
    vp, gp = plain.eval(th)
    assert forced.info()["lagstat_rows"] > 0 and plain.info()["lagstat_rows"] == 0
    _close(g, gp, v, vp)
    idx = list(range(forced.n_par_full))
    Hf, Hp = forced.hess(th, idx), plain.hess(th, idx)
    assert np.all(np.isfinite(Hp)) and np.max(np.abs(Hf - Hp)) <= 1e-12 * np.max(np.abs(Hp))
    rf, rp = forced.report(th), plain.report(th)
    assert np.array_equal(np.isnan(rf), np.isnan(rp))
    ok = ~np.isnan(rp)
    assert np.max(np.abs(rf[ok] - rp[ok])) <= 1e-12 * np.max(np.abs(rp[ok]))
    v2, g2 = forced.eval(_theta(model, d, 1))                    # ... and the next evaluation is back on the path
    assert forced.info()["lagstat_rows"] > 0
    forced.close(); plain.close()
