"""CPU suite: the head of the lag-statistics path from its Gram statistics (ssde_headforms.hpp, through
ssde_headforms_host) against the lanes' own recursion (ctcrw_mean_step, restated here) run row by row per track in numpy.longdouble
with the same gain rows: cuts 32, 64 and 128, free-parameter masks 15, 13, 1 and 0, mu zero and non-zero.  Bound: 1e-12 of
max(|sum|, 1), the bound of test_lagforms_cut_host.py.  The statistics come from the host reference (ssde_headstats_host).

Measured gap (40 tracks of 128 rows, sigma_obs 0.1, tau 2, nu 1, unit grid; 16 probe columns): at most 3.7e-15 of max(|sum|, 1) over
all 24 cases (cut 128, every direction, mu zero), 2.5e-16 .. 4.6e-16 on most; the shifted-column shortcut against the run with every
column a probe: 0 (the same bits) on every case.

The stand-alone sanitizer program of the same header (tests/hostsim/headforms_san.cpp, AddressSanitizer + UndefinedBehaviorSanitizer)
runs here too."""
import os
import subprocess

import numpy as np
import pytest

from smoothsde_amd import capi

LD = np.longdouble
N_TRACKS = 40
ROWS = 128
THETA0 = np.array([np.log(0.1), 0.0, 0.0, np.log(2.0), 0.0])
P0 = (1.0, 0.0, 10.0)
DIR_SIG, DIR_MU, DIR_P1, DIR_P2 = 1, 2, 4, 8
HOSTSIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(321)
    tracks, a0 = [], []
    for _ in range(N_TRACKS):
        vel = np.zeros(2)
        pos = 20.0 * rng.standard_normal(2)
        y = np.zeros((ROWS, 2))
        start = np.array([pos[0] + 0.1 * rng.standard_normal(), 0.2 * rng.standard_normal(), pos[1] + 0.1 * rng.standard_normal(), 0.2 * rng.standard_normal()])
        for t in range(ROWS):
            vel = 0.6 * vel + 0.8 * rng.standard_normal(2)
            pos = pos + vel
            y[t] = pos + 0.1 * rng.standard_normal(2)
        tracks.append(y)
        a0.append(start)
    a0 = np.stack(a0)
    G, s, n = capi.headstats_host(tracks, a0)
    return np.stack(tracks), a0, G, s, n


def lanes_longdouble(y, a0, gain, trans, mu, cut, mask):
    """ctcrw_mean_step row by row, every track and coordinate at once; returns the 6 accumulators ctcrw_finish_parts forms"""
    e, t12, b1, b2, de_, dt12_ = (LD(v) for v in trans)
    x = a0[:, 0::2].astype(LD)
    v = a0[:, 1::2].astype(LD)
    mu = np.asarray(mu, dtype=LD)[None, :]
    tx = np.zeros((3,) + x.shape, dtype=LD)
    tv = np.zeros_like(tx)
    mx = np.zeros_like(x)
    mv = np.zeros_like(x)
    accq = LD(0)
    gq = np.zeros(3, dtype=LD)
    gmu = np.zeros(2, dtype=LD)
    for t in range(cut):
        r = gain[t].astype(LD)
        iF, k1, k2, bm = r[0], r[1], r[2], r[3]
        u = y[:, t, :].astype(LD) - x
        su2 = np.sum(u * u)
        accq += iF * su2
        for j in range(3):
            du = -tx[j]
            gq[j] += LD(0.5) * r[4 + j] * su2 + iF * np.sum(u * du)
            nx = tx[j] + t12 * tv[j] + r[7 + j] * u + k1 * du
            nv = e * tv[j] + r[10 + j] * u + k2 * du
            if j == 1:
                w = v - bm * mu
                nx = nx + dt12_ * w
                nv = nv + de_ * w
            tx[j], tv[j] = nx, nv
        gmu += iF * np.sum(u * (-mx), axis=0)
        mx, mv = mx + t12 * mv - k1 * mx + bm * b1, e * mv - k2 * mx + bm * b2
        x, v = x + t12 * v + k1 * u + bm * b1 * mu, e * v + k2 * u + bm * b2 * mu
    out = np.array([LD(0.5) * accq, gq[0], gmu[0], gmu[1], gq[1], gq[2]], dtype=LD)
    keep = [True, bool(mask & DIR_SIG), bool(mask & DIR_MU), bool(mask & DIR_MU), bool(mask & DIR_P1), bool(mask & DIR_P2)]
    return np.where(keep, out, LD(0))


@pytest.mark.parametrize("with_mu", [False, True], ids=["mu0", "mu"])
@pytest.mark.parametrize("mask", [15, 13, 1, 0])
@pytest.mark.parametrize("cut", [32, 64, 128])
def test_the_forms_match_the_lanes_recursion_in_longdouble(batch, cut, mask, with_mu):
    y, a0, G, s, n = batch
    theta = THETA0.copy()
    if with_mu:
        theta[1:3] = (0.3, -0.2)
    got = capi.headforms_host(G, s, n, theta, 1.0, cut, p0=P0, mask=mask)
    full = capi.headforms_host(G, s, n, theta, 1.0, cut, p0=P0, mask=mask, full_probes=True)
    assert full["n_probe"] == cut + 1 and got["n_probe"] <= full["n_probe"]
    assert got["n_probe"] < cut + 1, got["n_probe"]                      # (the table is shorter than the head: the shortcut is in use)
    assert np.array_equal(got["gain"], full["gain"]) and np.all(got["gain"][:, 0] != 0.0)
    want = lanes_longdouble(y, a0, got["gain"], got["trans"], theta[1:3], cut, mask)
    scale = np.maximum(np.abs(want), LD(1))
    gap = float(np.max(np.abs(got["acc"].astype(LD) - want) / scale))
    gap_full = float(np.max(np.abs(got["acc"] - full["acc"]) / scale.astype(np.float64)))
    print("cut %d mask %d mu %d: %.2e against the lanes, %.2e shortcut against full probes (%d probe columns)" % (cut, mask, with_mu, gap, gap_full, got["n_probe"]))
    assert gap <= 1e-12, (gap, got["acc"], want)
    assert gap_full <= 1e-12, (gap_full, got["acc"], full["acc"])
    for k, bit in ((1, DIR_SIG), (2, DIR_MU), (3, DIR_MU), (4, DIR_P1), (5, DIR_P2)):
        assert (mask & bit) or got["acc"][k] == 0.0


def test_two_calls_give_the_same_bits_and_bad_arguments_are_refused(batch):
    y, a0, G, s, n = batch
    a = capi.headforms_host(G, s, n, THETA0, 1.0, 64, p0=P0)
    b = capi.headforms_host(G, s, n, THETA0, 1.0, 64, p0=P0)
    assert np.array_equal(a["acc"], b["acc"])
    for cut in (0, 129):
        with pytest.raises(ValueError):
            capi.headforms_host(G, s, n, THETA0, 1.0, cut, p0=P0)
    with pytest.raises(ValueError):
        capi.headforms_host(G, s, n, THETA0, 0.0, 64, p0=P0)


def test_the_header_under_the_sanitizers_as_a_program_of_its_own():
    prog = os.path.join(HOSTSIM, "headforms_san")
    if not os.path.exists(prog):
        subprocess.run(["make", "-s", "-C", HOSTSIM, "-f", "headforms.mk"], check=True)
    r = subprocess.run([prog], capture_output=True, text=True)
    assert r.returncode == 0 and "headforms_san ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
