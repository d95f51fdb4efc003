"""GPU suite: the head of the lag-statistics path under its latency plan (ssde_windows.hpp: head_latency_plan) --
the transient window on a wave of its own, [t0, LAG_A) in more stationary windows than the throughput rule allows.

The smallest shapes at which the new decode and geometry can go wrong: one group, a full group, a one-lane last group, three groups,
320 rows per track (barely longer than LAG_A: the look-ahead of the prefetch leaves the head), and a ragged batch whose lanes end
inside the transient window, inside window 1 and exactly at LAG_A.  The path is forced with SSDE_LAGSTATS=2.  A forced window count
(SSDE_CHUNKS=2) is the switch back to the throughput geometry: the transient window on the wave of window 1."""
import os

import numpy as np
import pytest

import hostsim_lib
from smoothsde_amd import capi
from test_head_plan_host import CONSTS, CTCRW, P0, WIN_ALIGN, _const

pytestmark = pytest.mark.gpu
K_ISO_SHARED = 3
WG_WAVES = 4
THREADS = min(16, os.cpu_count() or 8)
T = 320
TILE_U = _const("ssde_device.hpp", r"constexpr int TILE_U = (\d+);")
GLEN_MAX = -(-(T - 1) // TILE_U) * TILE_U           # steps of the longest group: a track's first row initialises its state; padded to the tile unit

SHAPES = [dict(M=1), dict(M=64), dict(M=65), dict(M=130), dict(M=100, ragged=True)]
CASES = [dict(s, d=d) for d in (2, 1) for s in SHAPES]


def _batch(M, d, ragged=False):
    import torch
    lengths = None
    if ragged:
        # (a track's first row initialises its state: 39 steps end inside the transient window, 255 inside the last window, 256 at LAG_A)
        lengths = np.resize(np.array([40, 256, 257, 300, 320], dtype=np.int64), M)
    ID, times, obs = capi.simulate_device("CTCRW", M, T, d, mu=0.0, tau=2.0, nu=1.0, kappa=1.0, sigma=1.0, sigma_obs=0.1, seed=31 + M + d,
                                          track0=0, lengths=lengths, device=torch.device("cuda:0"))
    fixed = np.zeros(1 + capi.n_sde_par("CTCRW", d), dtype=np.uint8)
    host = capi.Problem("CTCRW", ID.cpu().numpy(), times.cpu().numpy(), obs.cpu().numpy(), par_fixed=fixed)
    return host, (ID, times, obs, fixed)


def _engine(dev_data, monkeypatch, **env):
    ID, times, obs, fixed = dev_data
    with monkeypatch.context() as m:
        for name in ("SSDE_LAGSTATS", "SSDE_CHUNKS", "SSDE_FUSED_FINALIZE"):
            m.delenv(name, raising=False)
        for name, v in env.items():
            m.setenv(name, str(v))
        return capi.Engine(capi.Problem.from_torch("CTCRW", ID, times, obs, par_fixed=fixed))


def _theta(npar, d, k):
    th = np.zeros(npar)
    th[0] = np.log(0.1)
    th[1 + d] = np.log(2.0)
    return th + 0.01 * np.sin(np.arange(npar) + 0.7 * k)


def _host_window_counts(th, d, n_groups, glen_max):
    """the window counts the host plan gives this batch, over the gain tables an evaluation may have found (gain_last is not reported)"""
    par = hostsim_lib.window_params(CTCRW, th[1 + d], th[2 + d], float(np.exp(2.0 * th[0])), P0[CTCRW])
    want = max(1, 1024 // ((n_groups + 7) // 8 * 8))
    max_chunks = max(1, min(want + 1, max(1, glen_max // (4 * WIN_ALIGN))))        # ssde_engine_build.hip: plan_register_path
    facts = dict(model=CTCRW, use_shared=1, lag_ready=1, n_groups=n_groups, glen_max=glen_max, max_chunks=max_chunks,
                 want_chunks=max(1, min(want, max_chunks)))
    out = set()
    for gain_last in range(4, 65):
        g = hostsim_lib.window_geometry(CONSTS, par, ev=dict(gain_last=gain_last), **facts)
        if g["lag_K"] > 0:
            assert g["t0"] > 0 and g["t0_delta"] == 0, g
            out.add(g["n_chunks"])
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d_d%d%s" % (c["M"], c["d"], "_ragged" if c.get("ragged") else ""))
def test_the_head_on_its_latency_plan(case, monkeypatch):
    from oracle_lib import oracle_eval
    d = case["d"]
    host, dd = _batch(**case)
    engines = dict(lag=_engine(dd, monkeypatch, SSDE_LAGSTATS=2), stream=_engine(dd, monkeypatch, SSDE_LAGSTATS=0),
                   shared_wave=_engine(dd, monkeypatch, SSDE_LAGSTATS=2, SSDE_CHUNKS=2),
                   fused=_engine(dd, monkeypatch, SSDE_LAGSTATS=2, SSDE_FUSED_FINALIZE=1))
    try:
        lag = engines["lag"]
        for k in range(2):
            th = _theta(lag.n_par_full, d, k)
            v, g = lag.eval(th)
            inf = lag.info()
            g8 = (inf["n_groups"] + 7) // 8 * 8
            assert inf["lagstat_rows"] > 0 and inf["kernel_id"] == K_ISO_SHARED and inf["window_retries"] == 0, inf
            assert inf["window_check"] <= capi.WINDOW_TOL, inf
            # the plan in force: as many windows as the host plan says (more than three), every one on a wave of its own
            nc = inf["lanes_per_track"]
            counts = _host_window_counts(th, d, inf["n_groups"], GLEN_MAX)
            assert counts and min(counts) > 3 and nc in counts, (nc, counts)
            assert inf["n_kernel_blocks"] == (g8 * nc + WG_WAVES - 1) // WG_WAVES, inf
            # ... against the same batch streamed row by row
            vr, gr = engines["stream"].eval(th)
            assert engines["stream"].info()["lagstat_rows"] == 0
            assert abs(v - vr) <= 1e-12 * abs(vr), (v, vr)
            assert np.max(np.abs(g - gr)) <= 1e-10 * np.max(np.abs(gr)), (g, gr)
            # ... the oracle
            ov, og = oracle_eval(host, th, order=1, threads=THREADS)
            assert abs(v - ov) <= 1e-10 * abs(ov), (v, ov)
            assert np.max(np.abs(g - og)) <= 1e-8 * np.max(np.abs(og)), (g, og)
            # ... the throughput geometry (the transient window on the wave of window 1: one wave per group fewer than windows)
            vs, gs = engines["shared_wave"].eval(th)
            si = engines["shared_wave"].info()
            assert si["lagstat_rows"] > 0 and si["window_retries"] == 0 and si["window_check"] <= capi.WINDOW_TOL, si
            assert si["n_kernel_blocks"] == (g8 * (si["lanes_per_track"] - 1) + WG_WAVES - 1) // WG_WAVES, si
            print("head plan: windows %d (own wave) against %d (shared wave), value rel %.2e, gradient rel %.2e" %
                  (nc, si["lanes_per_track"], abs(v - vs) / abs(vs), np.max(np.abs(g - gs)) / np.max(np.abs(gs))))
            assert abs(v - vs) <= 1e-13 * abs(vs), (v, vs)
            assert np.max(np.abs(g - gs)) <= 1e-13 * np.max(np.abs(gs)), (g, gs)
            # ... and the finalising work inside the launch: bitwise the two-launch result
            vf, gf = engines["fused"].eval(th)
            fi = engines["fused"].info()
            assert fi["lagstat_rows"] > 0 and fi["lanes_per_track"] == nc and fi["n_kernel_blocks"] == inf["n_kernel_blocks"], fi
            assert vf == v and np.array_equal(gf, g)
            assert fi["window_check"] == inf["window_check"]
    finally:
        for e in engines.values():
            e.close()

