"""The window policy (smoothsde_amd/csrc/ssde_windows.hpp) on the host: the retry / rounding-floor / probation state machine, the
stationary radius, the warm-up and chunk plan and the geometry that follows it -- compiled by g++ into tests/hostsim and driven
here without a GPU, with the loop ssde_eval runs around an evaluation (hostsim_lib.WindowPolicy.call)."""
import os
import re

import numpy as np
import pytest

import hostsim_lib
from hostsim_lib import WindowPolicy, closed_loop_rho, window_geometry, window_params, window_plan

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smoothsde_amd", "csrc")


def _const(header, pattern):
    with open(os.path.join(CSRC, header)) as f:
        return int(re.search(pattern, f.read()).group(1))


WIN_ALIGN = _const("ssde_device.hpp", r"constexpr int WIN_ALIGN = (\d+);")
SHARED_U = _const("ssde_device.hpp", r"#define SSDE_SHARED_U (\d+)")
LAG_A = _const("ssde_lagstats.hpp", r"constexpr int LAG_A = (\d+);")
LAG_KMAX = _const("ssde_lagstats.hpp", r"constexpr int LAG_N = (\d+);") - 1
CONSTS = (WIN_ALIGN, SHARED_U, LAG_A, LAG_KMAX)
BM_SSM, OU_SSM, CTCRW = 2, 3, 4
TOL = 1e-11
P0 = {CTCRW: [1.0, 0.0, 10.0], OU_SSM: [10.0, 0.0, 0.0], BM_SSM: [10.0, 0.0, 0.0]}


def _changed(before, after):
    return {k for k in before if before[k] != after[k]}


def _until_sequential(check):
    """an evaluation whose windows disagree by `check` as long as it has more than one"""
    return lambda st: check if st["max_chunks"] > 1 else 0.0


# ---- the retry policy --------------------------------------------------------------------------------------------------------------
def test_an_agreeing_check_is_accepted_at_the_first_attempt():
    p = WindowPolicy()
    s0 = p.state()
    assert p.call([0.0]) == ([], 1)
    assert _changed(s0, p.state()) == {"calm"} and p.state()["calm"] == 1
    s1 = p.state()
    assert p.call([TOL]) == ([], 1)                                  # at the tolerance: accepted, and the largest accepted check so far
    assert _changed(s1, p.state()) == {"calm", "last_check", "check_max"}
    assert p.state()["check_max"] == TOL and p.state()["n_retries"] == 0 and p.state()["window_boost"] == 1


def test_failing_checks_quadruple_the_boost_three_times_then_give_up():
    p = WindowPolicy(max_chunks=9, want_chunks=8)
    boosts = []

    def check(st):
        boosts.append(st["window_boost"])
        return 1e-6 if st["max_chunks"] > 1 else 0.0
    actions, n = p.call(check)
    assert boosts == [1, 4, 16, 64, 64] and n == 5
    assert actions == ["sequential_saving"]
    s = p.state()
    assert s["gave_up"] == 1 and s["max_chunks"] == 1 and s["want_chunks"] == 1
    assert s["saved_max_chunks"] == 9 and s["saved_want_chunks"] == 8
    assert s["n_retries"] == 4 and s["calm"] == 0 and s["check_floor"] == 0.0


def test_three_flat_small_checks_set_the_floor_and_take_the_boost_back():
    p = WindowPolicy()
    assert p.call([3e-10, 2.5e-10, 2e-10]) == ([], 3)
    s = p.state()
    assert s["check_floor"] == min(1e-8, 4.0 * 3e-10) and s["window_boost"] == 1 and s["gave_up"] == 0 and s["n_retries"] == 2
    assert s["check_max"] == 2e-10
    assert p.call([1e-9]) == ([], 1)                                 # under the floor: accepted as it is
    assert p.state()["n_retries"] == 2 and p.state()["check_floor"] == s["check_floor"]
    assert p.call([0.5 * TOL]) == ([], 1)                            # an outright agreement ends the regime that showed the floor
    assert p.state()["check_floor"] == 0.0
    _, n = p.call([1e-9, 0.0])                                       # ... and the same check is a failure again
    assert n == 2 and p.state()["n_retries"] == 3
    # the floor is capped at 1e-8, and the boost goes back by 16 from wherever it stands (kept as it is)
    q = WindowPolicy()
    q.widen(8)
    assert q.call([9e-9, 8e-9, 7e-9]) == ([], 3)
    assert q.state()["check_floor"] == 1e-8 and q.state()["window_boost"] == 8


def test_a_check_that_shrinks_over_the_retries_sets_no_floor():
    p = WindowPolicy()
    assert p.call([8e-9, 2e-9, 4e-10, 0.0]) == ([], 4)              # each less than half the one before
    s = p.state()
    assert s["check_floor"] == 0.0 and s["window_boost"] == 64 and s["gave_up"] == 0 and s["n_retries"] == 3
    q = WindowPolicy()
    assert q.call([3e-10, 2.5e-10, 1e-10, 0.0]) == ([], 4)          # flat, then not
    assert q.state()["check_floor"] == 0.0 and q.state()["window_boost"] == 64
    r = WindowPolicy()
    assert r.call([3e-7, 2.5e-7, 2e-7, 1.9e-7, 0.0])[0] == ["sequential_saving"]      # flat, but not small
    assert r.state()["check_floor"] == 0.0 and r.state()["gave_up"] == 1


def test_the_floor_found_one_attempt_late_leaves_the_boost_at_four():
    """kept as it is: `/ 16` takes back two quadruplings, a call that needed three keeps x4"""
    p = WindowPolicy()
    assert p.call([1e-6, 3e-10, 2.5e-10, 2e-10]) == ([], 4)
    assert p.state()["check_floor"] == 4.0 * 3e-10 and p.state()["window_boost"] == 4 and p.state()["gave_up"] == 0


@pytest.mark.parametrize("check", [float("inf"), float("nan"), 1.0])
def test_a_non_finite_value_is_never_retried_and_never_widens_the_plan(check):
    p = WindowPolicy()
    s0 = p.state()
    assert p.call([check], finite=False) == ([], 1)
    s1 = p.state()
    assert _changed(s0, s1) <= {"last_check", "calm"}
    assert s1["window_boost"] == 1 and s1["n_retries"] == 0 and s1["check_max"] == 0.0 and s1["gave_up"] == 0


def test_one_window_with_nothing_to_disagree_breaks_out_unless_others_decide_too():
    p = WindowPolicy()
    assert p.call([1e-6], one_window=True) == ([], 1)
    assert p.state()["n_retries"] == 0 and p.state()["window_boost"] == 1 and p.state()["check_max"] == 1e-6
    q = WindowPolicy()
    _, n = q.call([1e-6, 0.0], one_window=True, dist=True)           # shards or ranks: everyone retries alike
    assert n == 2 and q.state()["n_retries"] == 1 and q.state()["window_boost"] == 4


def test_the_row_varying_paths_retry_once_without_a_boost():
    p = WindowPolicy()
    _, n = p.call([1e-6, 0.0], replans=True)
    assert n == 2 and p.state()["window_boost"] == 1 and p.state()["n_retries"] == 1
    boosts = []

    def check(st):
        boosts.append(st["window_boost"])
        return 1e-6 if st["max_chunks"] > 1 else 0.0
    actions, n = p.call(check, replans=True)
    assert boosts == [1, 1, 4, 16, 16] and actions == ["sequential_saving"]          # (the fourth retry gives up, the boost at x16)


def test_a_widened_plan_is_halved_on_probation_after_the_cooldown():
    p = WindowPolicy()
    p.widen(4)
    assert p.state()["window_boost"] == 4 and p.state()["cooldown"] == 32
    for k in range(31):
        assert p.call([0.0]) == ([], 1)
    assert p.state()["probing"] == 0 and p.state()["window_boost"] == 4 and p.state()["calm"] == 31
    assert p.call([0.0]) == ([], 1)
    s = p.state()
    assert s["probing"] == 1 and s["probe_from"] == 4 and s["window_boost"] == 2 and s["calm"] == 0
    for k in range(3):
        p.call([0.0])
        assert p.state()["probing"] == 1
    p.call([0.0])                                                    # four calm calls: the narrower plan holds
    assert p.state()["probing"] == 0 and p.state()["window_boost"] == 2 and p.state()["cooldown"] == 32
    # SSDE_CHUNKS: the window count is the tester's, calm calls are not counted
    f = WindowPolicy()
    f.widen(4)
    for k in range(40):
        f.call([0.0], forced=True)
    assert f.state()["calm"] == 0 and f.state()["window_boost"] == 4 and f.state()["probing"] == 0


def test_a_given_up_plan_is_restored_on_probation():
    p = WindowPolicy(max_chunks=9, want_chunks=8)
    p.call(_until_sequential(1e-6))
    assert p.state()["gave_up"] == 1
    for k in range(31):
        assert p.call([0.0], one_window=True) == ([], 1)
    assert p.call([0.0], one_window=True) == (["restore"], 1)
    s = p.state()
    assert s["gave_up"] == 0 and s["max_chunks"] == 9 and s["want_chunks"] == 8 and s["probing"] == 1 and s["probe_from"] == 0
    assert s["window_boost"] == 64                                   # (kept as it is: the boost the retries left)
    # ... and does not hold: one sequential window again, the saved limits untouched, twice the wait
    actions, n = p.call([1e-6, 0.0])
    assert actions == ["sequential"] and n == 2
    s = p.state()
    assert s["gave_up"] == 1 and s["max_chunks"] == 1 and s["saved_max_chunks"] == 9 and s["saved_want_chunks"] == 8
    assert s["probing"] == 0 and s["cooldown"] == 64


def test_a_failure_on_probation_restores_the_boost_and_doubles_the_cooldown_up_to_its_cap():
    p = WindowPolicy()
    p.widen(4)
    cooldown = 32
    while True:
        for k in range(cooldown):
            p.call([0.0])
        s = p.state()
        assert s["probing"] == 1 and s["probe_from"] == 4 and s["window_boost"] == 2
        _, n = p.call([1e-6, 0.0])                                   # the first attempt on probation fails
        s = p.state()
        assert n == 2 and s["window_boost"] == 4 and s["probing"] == 0
        assert s["cooldown"] == min(2 * cooldown, 1 << 14)
        if cooldown == 1 << 14:
            break
        cooldown = s["cooldown"]
    # a failure once the probation has ended is an ordinary one: the boost is quadrupled from where it stands
    q = WindowPolicy()
    q.widen(4)
    for k in range(32 + 4):
        q.call([0.0])
    assert q.state()["probing"] == 0 and q.state()["window_boost"] == 2
    q.call([1e-6, 0.0])
    assert q.state()["window_boost"] == 8 and q.state()["cooldown"] == 32


def test_no_more_than_seven_retries_ever():
    for kw in (dict(), dict(replans=True), dict(dist=True, one_window=True)):
        p = WindowPolicy()
        _, n = p.call([1e-6], **kw)
        assert n == 8 and p.state()["n_retries"] == 7 and p.state()["check_max"] == 1e-6, kw
        _, n = p.call([1e-6], **kw)                                  # and again at the next call
        assert n == 8 and p.state()["n_retries"] == 14, kw


def test_widen_and_relax():
    p = WindowPolicy()
    p.widen(4); p.widen(2)
    assert p.state()["window_boost"] == 8
    p.relax()
    assert p.state()["window_boost"] == 4
    for k in range(5):
        p.relax()
    assert p.state()["window_boost"] == 1
    for k in range(30):
        p.widen(4)
    assert p.state()["window_boost"] == 1 << 20                      # widened no further from there
    p.widen(0)
    assert p.state()["window_boost"] == 1 << 20                      # (factor <= 0 is the engines': one sequential window)


# ---- the stationary radius ---------------------------------------------------------------------------------------------------------
def _rho_numpy(model, dt, p1, p2, h):
    """the closed-loop radius from the stationary covariance, by plain iteration in numpy"""
    if model == CTCRW:
        tau, nu = np.exp(p1), np.exp(p2)
        beta, sigma = 1.0 / tau, 2.0 * nu / np.sqrt(np.pi * tau)
        e = np.exp(-beta * dt)
        T = np.array([[1.0, (1.0 - e) / beta], [0.0, e]])
        s2 = sigma * sigma
        Q = np.array([[s2 / beta ** 2 * (dt - 2.0 * (1.0 - e) / beta + (1.0 - e * e) / (2.0 * beta)), s2 / (2.0 * beta ** 2) * (1.0 - e) ** 2],
                      [0.0, s2 / (2.0 * beta) * (1.0 - e * e)]])
        Q[1, 0] = Q[0, 1]
        Z = np.array([[1.0, 0.0]])
        P = np.diag([1.0, 10.0])
    else:
        if model == OU_SSM:
            t = np.exp(-dt / np.exp(p1))
            T, Q = np.array([[t]]), np.array([[np.exp(p2) * (1.0 - t * t)]])
        else:
            T, Q = np.array([[1.0]]), np.array([[np.exp(2.0 * p1) * dt]])
        Z = np.array([[1.0]])
        P = np.array([[10.0]])
    for it in range(20000):
        K = T @ P @ Z.T / (Z @ P @ Z.T + h)
        Pn = T @ P @ (T - K @ Z).T + Q
        done = np.max(np.abs(Pn - P)) <= 1e-15 * np.max(np.abs(Pn))
        P = Pn
        if done:
            break
    return np.max(np.abs(np.linalg.eigvals(T - K @ Z)))


GRID = [(m, dt, p1, p2, h) for m in (CTCRW, OU_SSM, BM_SSM) for dt in (0.25, 1.0, 3.5) for p1 in (-1.0, 0.3, 1.5)
        for p2 in (-0.7, 0.4) for h in (1e-4, 0.04, 2.0)]


def test_the_plans_radius_is_closed_loop_rho_bit_for_bit():
    for model, dt, p1, p2, h in GRID:
        r = closed_loop_rho(model, dt, p1, p2, h, P0[model])
        plan = window_plan(CONSTS, window_params(model, p1, p2, h, P0[model]), model=model, uniform_dt=1, dt_uniform=dt)
        assert plan["rho"] == r and 0.0 <= r < 1.0, (model, dt, p1, p2, h, plan["rho"], r)
        irregular = window_plan(CONSTS, window_params(model, p1, p2, h, P0[model]), model=model, uniform_dt=0, dt_uniform=0.0, dt_min=dt,
                                dt_max=2 * dt)
        assert irregular["rho"] == r
        assert abs(r - _rho_numpy(model, dt, p1, p2, h)) <= 1e-9, (model, dt, p1, p2, h)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert closed_loop_rho(CTCRW, bad, 0.3, 0.1, 0.04, P0[CTCRW]) == 1.0


def test_row_varying_tau_nu_plans_from_the_slowest_corner_of_the_ranges():
    par = window_params(CTCRW, 0.3, 0.1, 0.04, P0[CTCRW])
    lo, hi = (-0.2, -0.5), (0.9, 0.6)
    plan = window_plan(CONSTS, par, model=CTCRW, drift=3, uniform_dt=0, dt_uniform=0.0, dt_min=0.5, dt_max=1.5, eta_lo0=lo[0], eta_lo1=lo[1],
                       eta_hi0=hi[0], eta_hi1=hi[1])
    corners = [closed_loop_rho(CTCRW, dt, a, b, 0.04, P0[CTCRW]) for dt in (0.5, 1.5) for a in (lo[0], hi[0]) for b in (lo[1], hi[1])]
    assert plan["rho"] == max(corners)


# ---- the warm-up and the plan -------------------------------------------------------------------------------------------------------
def test_the_warm_up_is_aligned_at_least_sixteen_and_grows_with_the_boost():
    lib = hostsim_lib.load()
    for rho in (0.0, 1e-300, 0.01, 0.3, 0.7, 0.9, 0.97, 0.999):
        for slack in (0, 16, 16 + WIN_ALIGN):
            last = 0
            for boost in (1, 2, 4, 16, 64, 1024):
                w = lib.hostsim_warmup(rho, slack, -1, boost, WIN_ALIGN)
                assert w % WIN_ALIGN == 0 and w >= 16 and w > last, (rho, slack, boost, w)
                assert rho == 0.0 or rho ** (w / boost - slack + 1) <= 1e-18 or w / boost == 16
                last = w
    assert lib.hostsim_warmup(0.9, 16, 2, 1, WIN_ALIGN) == WIN_ALIGN             # SSDE_WINDOW replaces the estimate ...
    assert lib.hostsim_warmup(0.9, 16, 2, 64, WIN_ALIGN) == 128                  # ... and is boosted like it
    for model, dt, p1, p2, h in GRID:
        par = window_params(model, p1, p2, h, P0[model])
        last = 0
        for boost in (1, 4, 16):
            plan = window_plan(CONSTS, par, boost=boost, model=model, dt_uniform=dt, glen_max=100000, max_chunks=64, want_chunks=32)
            if plan["warmup"] == 0:
                assert plan["n_chunks"] == 1 and plan["window"] == 0
                continue
            assert plan["warmup"] % WIN_ALIGN == 0 and plan["warmup"] >= 16 and plan["warmup"] > last
            assert plan["warmup"] == lib.hostsim_warmup(plan["rho"], 16, -1, boost, WIN_ALIGN)
            assert plan["window"] in (0, plan["warmup"]) and (plan["n_chunks"] > 1) == (plan["window"] > 0)
            assert plan["n_chunks"] == 1 or 100000 // plan["n_chunks"] >= 2 * plan["warmup"]
            last = plan["warmup"]


def _find(model, lo, hi):
    """parameters of `model` whose closed-loop radius lies in (lo, hi): slow movement under a large observation variance"""
    for h in (1.0, 10.0, 100.0, 1e3, 1e4, 1e5, 1e6, 1e7):
        for p1 in (0.3, 4.0, 8.0):
            for p2 in (0.0, -1.0, -2.0):
                q1 = p1 if model != BM_SSM else p2
                r = closed_loop_rho(model, 1.0, q1, p2, h, P0[model])
                if lo < r < hi:
                    return window_params(model, q1, p2, h, P0[model]), r
    raise AssertionError("no such parameters on the grid")


def test_no_usable_forgetting_gives_a_sequential_plan():
    for model in (CTCRW, OU_SSM, BM_SSM):
        par, r = _find(model, 0.9995, 1.0 + 1e-9)
        plan = window_plan(CONSTS, par, model=model, glen_max=1000000, max_chunks=64, want_chunks=32)
        assert plan == dict(n_chunks=1, window=0, warmup=0, rho=r), (model, plan)
    # the transfer-function lanes of the shared CTCRW path stop at 0.97; the general kernel, the scalar models and a drift do not
    par, r = _find(CTCRW, 0.97, 0.9995)
    kw = dict(model=CTCRW, glen_max=1000000, max_chunks=64, want_chunks=32)
    assert window_plan(CONSTS, par, use_shared=1, **kw) == dict(n_chunks=1, window=0, warmup=0, rho=r)
    assert window_plan(CONSTS, par, use_shared=0, **kw)["n_chunks"] > 1
    assert window_plan(CONSTS, par, use_shared=1, drift=1, **kw)["n_chunks"] > 1
    par, r = _find(OU_SSM, 0.97, 0.9995)
    assert window_plan(CONSTS, par, use_shared=1, **dict(kw, model=OU_SSM))["n_chunks"] > 1
    # one chunk allowed (a plan that has given up): nothing is planned at all
    assert window_plan(CONSTS, window_params(CTCRW, 0.3, 0.1, 0.04, P0[CTCRW]), max_chunks=1, want_chunks=1)["warmup"] == 0
    # a warm-up longer than the longest track: sequential
    assert window_plan(CONSTS, window_params(CTCRW, 0.3, 0.1, 0.04, P0[CTCRW]), boost=1024, glen_max=4000)["warmup"] == 0


# ---- the geometry ------------------------------------------------------------------------------------------------------------------
def test_a_transient_window_leaves_room_for_two_warm_ups():
    rng = np.random.default_rng(20250101)
    n_t0 = 0
    for k in range(3000):
        model = int(rng.choice([CTCRW, OU_SSM, BM_SSM]))
        par = window_params(model, rng.uniform(-1, 1.5), rng.uniform(-1, 1), float(np.exp(rng.uniform(-8, 1))), P0[model])
        shared = int(rng.random() < 0.7)
        lag = int(shared and rng.random() < 0.3)
        facts = dict(model=model, glen_max=int(rng.integers(40, 20000)), max_chunks=int(rng.integers(1, 40)), use_shared=shared,
                     lag_ready=lag, chunks_forced=int(rng.random() < 0.1), any_dirty=int(shared and not lag and rng.random() < 0.5),
                     want_chunks_d=int(rng.integers(0, 30)), quiet_ok=int(not lag and rng.random() < 0.3))
        facts["want_chunks"] = int(rng.integers(1, facts["max_chunks"] + 1))
        boost = int(rng.choice([1, 1, 2, 4, 16]))
        g = window_geometry(CONSTS, par, boost=boost, ev=dict(gain_last=int(rng.integers(1, 300)), can_derive=int(rng.random() < 0.5)), **facts)
        glen = LAG_A if g["lag_K"] > 0 else facts["glen_max"]
        if g["t0"] > 0:
            n_t0 += 1
            assert g["t0"] + 2 * g["window"] < glen and g["t0"] % WIN_ALIGN == 0 and g["n_chunks"] >= 2, (facts, g)
            assert g["n_chunks"] <= max(2, facts["max_chunks"])
        assert g["t0_delta"] % WIN_ALIGN == 0 and (g["t0_delta"] == 0 or shared)
        if g["dual"]:
            assert g["n_chunks_d"] > 1 and facts["glen_max"] // g["n_chunks_d"] >= 2 * g["window"]
            assert g["t0_d"] == 0 or g["t0_d"] + 2 * g["window"] < facts["glen_max"]
        assert g["s_stat"] % SHARED_U == 0 and 0 <= g["s_stat"] - 0 < 300 + SHARED_U
        # the cut of the lag statistics: only where it fits the statistics and the head
        if g["lag_K"] > 0:
            assert lag and g["lag_K"] == g["first"]["warmup"] <= LAG_KMAX and g["s_stat"] + g["lag_K"] <= LAG_A, (facts, g)
        elif lag and g["first"]["warmup"] > 0:
            assert g["first"]["warmup"] > LAG_KMAX or g["s_stat"] + g["first"]["warmup"] > LAG_A, (facts, g)
    assert n_t0 > 300


def test_the_lag_cut_needs_a_usable_plan_and_stationary_gains():
    par = window_params(CTCRW, np.log(2.0), 0.0, 0.01, P0[CTCRW])
    kw = dict(model=CTCRW, use_shared=1, lag_ready=1, glen_max=3000, max_chunks=3, want_chunks=2)
    g = window_geometry(CONSTS, par, ev=dict(gain_last=30), **kw)
    assert g["lag_K"] == g["first"]["warmup"] > 0 and g["t0"] + 2 * g["window"] < LAG_A          # the head is planned as a LAG_A-row batch
    assert window_geometry(CONSTS, par, gave_up=True, ev=dict(gain_last=30), **kw)["lag_K"] == 0
    assert window_geometry(CONSTS, par, ev=dict(gain_last=30, gain_usable=0), **kw)["lag_K"] == 0
    assert window_geometry(CONSTS, par, ev=dict(gain_last=30, hess_req=1), **kw)["lag_K"] == 0
    assert window_geometry(CONSTS, par, ev=dict(gain_last=30, n_parts=2), **kw)["lag_K"] == 0
    assert window_geometry(CONSTS, par, ev=dict(gain_last=LAG_A - 8), **kw)["lag_K"] == 0         # no room for K rows before LAG_A
    assert window_geometry(CONSTS, par, boost=16, ev=dict(gain_last=30), **kw)["lag_K"] == 0      # K beyond the statistics' taps


def test_the_mixed_batchs_second_plan_uses_the_balance_of_the_all_general_case():
    par = window_params(CTCRW, np.log(2.0), 0.0, 0.01, P0[CTCRW])
    mixed = window_geometry(CONSTS, par, model=CTCRW, use_shared=1, any_dirty=1, want_chunks_d=12, glen_max=6000, max_chunks=5, want_chunks=4,
                            ev=dict(gain_last=30, can_derive=1))
    general = window_geometry(CONSTS, par, model=CTCRW, use_shared=0, glen_max=6000, max_chunks=13, want_chunks=12, ev=dict(can_derive=1))
    assert mixed["dual"] == 1 and mixed["n_chunks_d"] == general["n_chunks"] == 12 and mixed["window"] == general["window"] > 0
    assert mixed["t0_d"] == general["t0"] > 0 and general["t0_delta"] == 0
    lib = hostsim_lib.load()
    assert mixed["t0_d"] == lib.hostsim_balanced_window0(6000, 12, mixed["window"], 1, WIN_ALIGN)
    # window 0 costs W0_RATIO a row where the later windows derive a direction: it is the shorter for it
    assert lib.hostsim_balanced_window0(6000, 12, mixed["window"], 0, WIN_ALIGN) > mixed["t0_d"]
    assert mixed["t0"] > 0 and mixed["t0_delta"] > 0               # (the shared launch's own transient window is another matter)


def test_quiet_rows_remember_the_warm_up_and_stop_with_a_given_up_plan():
    par = window_params(CTCRW, np.log(2.0), 0.0, 0.01, P0[CTCRW])
    kw = dict(model=CTCRW, use_shared=0, quiet_ok=1, block_rows=4, glen_max=4000)
    g = window_geometry(CONSTS, par, ev=dict(gain_last=30), **kw)
    assert g["quiet_window"] == g["plan"]["warmup"] > 0 and g["quiet_w"] == -(-g["quiet_window"] // 4) and g["quiet_b0"] == g["s_stat"] // 4 + 1
    assert window_geometry(CONSTS, par, gave_up=True, ev=dict(gain_last=30), **kw)["quiet_window"] == 0
    assert window_geometry(CONSTS, par, ev=dict(gain_last=30, gain_usable=0), **kw)["quiet_window"] == 0
    short = window_geometry(CONSTS, par, boost=4, ev=dict(gain_last=30), **dict(kw, quiet_window=2))        # SSDE_QUIET_WINDOW, boosted
    assert short["quiet_window"] == 8 and short["quiet_w"] == 2
