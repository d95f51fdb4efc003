"""CPU suite: the latency plan of the lag-statistics head (smoothsde_amd/csrc/ssde_windows.hpp: head_latency_plan),
through hostsim_lib.window_geometry.

The head -- rows [0, LAG_A) of every track -- is a few hundred waves on 1024 SIMDs: what its launch takes is the chain of rows of its
longest wave.  Where that is cheaper the transient window [0, t0) gets a wave of its own (t0 > 0 with t0_delta == 0) and [t0, LAG_A)
is cut into more stationary windows than the throughput rule (windows at least two warm-ups long) allows.  A forced window count
(the fact SSDE_CHUNKS sets: chunks_forced) keeps the throughput geometry -- the switch for A/B runs; the parent's geometry is also
recomputed here from its own rules.  window_bounds of ssde_device.hpp is mirrored below: the tests deal the rows as the kernels do."""
import os
import re

import numpy as np

from hostsim_lib import window_geometry, window_params

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smoothsde_amd", "csrc")


def _read(header):
    with open(os.path.join(CSRC, header)) as f:
        return f.read()


def _const(header, pattern, conv=int):
    return conv(re.search(pattern, _read(header)).group(1))


WIN_ALIGN = _const("ssde_device.hpp", r"constexpr int WIN_ALIGN = (\d+);")
SHARED_U = _const("ssde_device.hpp", r"#define SSDE_SHARED_U (\d+)")
LAG_A = _const("ssde_lagstats.hpp", r"constexpr int LAG_A = (\d+);")
LAG_KMAX = _const("ssde_lagstats.hpp", r"constexpr int LAG_N = (\d+);") - 1
T0_COST = _const("ssde_windows.hpp", r"constexpr double T0_COST = ([0-9.]+)", float)
CONSTS = (WIN_ALIGN, SHARED_U, LAG_A, LAG_KMAX)
BM_SSM, OU_SSM, CTCRW = 2, 3, 4
P0 = {CTCRW: [1.0, 0.0, 10.0], OU_SSM: [10.0, 0.0, 0.0], BM_SSM: [10.0, 0.0, 0.0]}
WAVE_SLOTS = 1024


def _align(x):
    return -(-x // WIN_ALIGN) * WIN_ALIGN


def window_bounds(L, n_chunks, window, t0, c, delta):
    """ssde_device.hpp: window_bounds -> (s_begin, s_acc, s_end)"""
    WA = WIN_ALIGN
    if n_chunks <= 1:
        return 0, 0, L
    if t0 > 0:
        if c == 0:
            return 0, 0, min(L, t0)
        rest, nw = max(L - t0, 0), n_chunks - 1
        units = -(-(rest + delta) // WA)
        per, extra = divmod(units, nw)
        cl = (per + (1 if extra else 0)) * WA
        if cl <= delta + WA:
            w1 = min(rest, 2 * WA)
            if c == 1:
                s_acc, s_end = t0, (t0 + w1 if n_chunks > 2 else L)
            else:
                per2, ex2 = divmod(-(-(rest - w1) // WA), n_chunks - 2)
                k = c - 2
                s_acc = t0 + w1 + (k * per2 + min(k, ex2)) * WA
                s_end = t0 + w1 + ((k + 1) * per2 + min(k + 1, ex2)) * WA
            s_acc, s_end = min(s_acc, L), min(s_end, L)
        else:
            e0 = t0 - delta + ((c - 1) * per + min(c - 1, extra)) * WA
            e1 = t0 - delta + (c * per + min(c, extra)) * WA
            s_acc = min(t0 if c == 1 else e0, L)
            s_end = max(min(e1, L), s_acc)
    else:
        per, extra = divmod(-(-L // WA), n_chunks)
        s_acc = min((c * per + min(c, extra)) * WA, L)
        s_end = min(((c + 1) * per + min(c + 1, extra)) * WA, L)
    return max(s_acc - window, 0), s_acc, s_end


def wave_rows(g, L=None):
    """rows every wave of a group walks under the geometry g (k_iso_shared.inc: shared_wave): warm-up and scored rows of its windows;
    with t0_delta > 0 the wave of window 1 walks window 0 first, with t0_delta == 0 window 0 has a wave of its own"""
    L = LAG_A if L is None else L
    n = [e - b for b, _, e in (window_bounds(L, g["n_chunks"], g["window"], g["t0"], c, g["t0_delta"]) for c in range(g["n_chunks"]))]
    if g["t0"] > 0 and g["t0_delta"] > 0:
        return [n[0] + n[1]] + n[2:]
    return n


def theta_for(npar, d, k):
    """bench.py: theta_for (CTCRW, q = d + 2)"""
    base = np.zeros(npar)
    base[0] = np.log(0.1)
    base[1 + d] = np.log(2.0)
    return base + 0.01 * np.sin(np.arange(npar) + 0.7 * k)


def _bench_par(k):
    th = theta_for(5, 2, k)
    return window_params(CTCRW, th[3], th[4], float(np.exp(2.0 * th[0])), P0[CTCRW])


BENCH = dict(model=CTCRW, use_shared=1, lag_ready=1, n_groups=157, max_chunks=7, want_chunks=6, glen_max=10000)


def _parent_head(g):
    """the parent commit's head geometry from its own rules: the throughput plan of a LAG_A-row batch (windows at least two warm-ups
    long), the transient window on top and on the wave of window 1, which gives T0_COST x t0 rows away"""
    W = g["plan"]["warmup"]
    nc = BENCH["want_chunks"]
    while nc > 1 and LAG_A // nc < 2 * W:
        nc -= 1
    assert nc > 1
    t0 = _align(g["s_stat"] + W)
    assert t0 + 2 * W < LAG_A
    return dict(n_chunks=min(nc + 1, BENCH["max_chunks"]), window=W, t0=t0, t0_delta=_align(int(T0_COST * t0)))


def test_the_bench_head_gets_the_transient_on_its_own_wave_and_a_shorter_longest_wave():
    seen = set()
    for k in (-6, 0, 7, 50, 99):
        par = _bench_par(k)
        for gain_last in range(20, 33):
            g = window_geometry(CONSTS, par, ev=dict(gain_last=gain_last), **BENCH)
            assert g["lag_K"] == g["first"]["warmup"] > 0 and g["window"] == g["plan"]["warmup"]
            assert g["t0"] > 0 and g["t0_delta"] == 0 and g["n_chunks"] >= 4, g
            assert 160 * g["n_chunks"] <= WAVE_SLOTS                              # one round of waves (157 groups padded to 8)
            assert g["t0"] + 2 * g["window"] < LAG_A and g["n_chunks"] <= BENCH["max_chunks"]
            parent = _parent_head(g)
            forced = window_geometry(CONSTS, par, ev=dict(gain_last=gain_last), **dict(BENCH, chunks_forced=1))
            assert {k_: forced[k_] for k_ in parent} == parent, (forced, parent)   # the switch gives exactly the parent's geometry here
            new_rows, old_rows = wave_rows(g), wave_rows(parent)
            assert len(new_rows) == g["n_chunks"] and len(old_rows) == parent["n_chunks"] - 1
            assert max(new_rows) < max(old_rows), (new_rows, old_rows)
            assert new_rows[0] == g["t0"] and max(new_rows[1:]) <= g["window"] + _align(-(-(LAG_A - g["t0"]) // (g["n_chunks"] - 1)))
            seen.add((g["t0"], g["n_chunks"]))
    assert seen


def test_more_groups_than_wave_slots_keep_the_parents_plan():
    """c4: 10^5 tracks, 1563 groups -- the engine allows it two windows (one wave per group: more waves than wave slots already); a
    second wave per group would be a further round"""
    par = _bench_par(0)
    kw = dict(BENCH, n_groups=1563, max_chunks=2, want_chunks=1)
    for gain_last in (12, 20, 32):
        g = window_geometry(CONSTS, par, ev=dict(gain_last=gain_last), **kw)
        W = g["plan"]["warmup"]
        # the parent's rules: one stationary window, the transient window before it on the same wave
        assert g["lag_K"] == W > 0 and g["window"] == W and g["n_chunks"] == 2 and g["t0"] == _align(g["s_stat"] + W)
        assert g["t0_delta"] == _align(int(T0_COST * g["t0"])) > 0
        assert wave_rows(g) == [LAG_A + W]                     # (one wave per group: the head, and window 1's warm-up a second time)


def _sweep(rng, n):
    for _ in range(n):
        model = int(rng.choice([CTCRW, OU_SSM, BM_SSM]))
        par = window_params(model, rng.uniform(-1, 1.5), rng.uniform(-1, 1), float(np.exp(rng.uniform(-8, 1))), P0[model])
        facts = dict(model=model, glen_max=int(rng.integers(40, 20000)), max_chunks=int(rng.integers(1, 40)), use_shared=1,
                     lag_ready=int(rng.random() < 0.8), n_groups=int(rng.integers(1, 3001)))
        facts["want_chunks"] = int(rng.integers(1, facts["max_chunks"] + 1))
        boost = int(rng.choice([1, 1, 2, 4, 16]))
        ev = dict(gain_last=int(rng.integers(1, 300)))
        yield par, facts, boost, ev


def test_with_a_forced_window_count_the_transient_stays_on_the_wave_of_window_1():
    rng = np.random.default_rng(20250808)
    n_lag = 0
    for par, facts, boost, ev in _sweep(rng, 1500):
        g = window_geometry(CONSTS, par, boost=boost, ev=ev, **dict(facts, chunks_forced=1))
        assert g["t0_delta"] == _align(int(T0_COST * g["t0"])), (facts, g)
        n_lag += g["lag_K"] > 0 and g["t0"] > 0
    assert n_lag > 100


def test_the_invariants_of_the_geometry_and_the_tiling_of_the_head():
    rng = np.random.default_rng(20250809)
    n_own = n_shared = 0
    for par, facts, boost, ev in _sweep(rng, 3000):
        g = window_geometry(CONSTS, par, boost=boost, ev=ev, **facts)
        forced = window_geometry(CONSTS, par, boost=boost, ev=ev, **dict(facts, chunks_forced=1))
        assert g["lag_K"] == forced["lag_K"] and g["s_stat"] == forced["s_stat"], (facts, g, forced)      # the plan leaves them alone
        assert g["t0"] % WIN_ALIGN == 0 and g["t0_delta"] % WIN_ALIGN == 0
        if g["lag_K"] == 0:
            continue
        assert g["lag_K"] == g["first"]["warmup"] <= LAG_KMAX and g["s_stat"] + g["lag_K"] <= LAG_A
        if g["t0"] == 0:
            continue
        assert g["t0"] + 2 * g["window"] < LAG_A, (facts, g)
        assert 2 <= g["n_chunks"] <= max(2, facts["max_chunks"]), (facts, g)
        assert g["t0_delta"] in (0, _align(int(T0_COST * g["t0"])))
        n_own += g["t0_delta"] == 0
        n_shared += g["t0_delta"] > 0
        if g["t0_delta"] == 0:
            # no stationary window is left empty on a full-length head, and every one starts its warm-up in the stationary regime
            rows = wave_rows(g)
            assert min(rows) > 0 and rows[0] == g["t0"]
            assert g["t0"] - g["window"] >= g["s_stat"]
        for L in sorted({1, 15, 16, 17, g["t0"] - 1, g["t0"], g["t0"] + 1, 255, 256}):
            b = [window_bounds(L, g["n_chunks"], g["window"], g["t0"], c, g["t0_delta"]) for c in range(g["n_chunks"])]
            assert b[0][1] == 0 and b[-1][2] == L, (L, g, b)
            for c in range(g["n_chunks"]):
                s_begin, s_acc, s_end = b[c]
                assert 0 <= s_begin <= s_acc <= s_end <= L, (L, g, b)
                assert s_acc - s_begin <= g["window"]
                if c > 0:
                    assert s_acc == b[c - 1][2], (L, g, b)                            # no gap, no overlap
                    assert s_acc == L or s_acc - s_begin == g["window"], (L, g, b)    # a full warm-up before every scored row
    assert n_own > 200 and n_shared > 20
