"""Multi-step-ahead forecast scores without a GPU: the host twin of k_smooth_ahead.hip's lane math
(tests/aheadsim_lib.py: csrc/ssde_ahead.hpp walked block by block as the kernel walks it) against the numpy definition of
tests/ahead_ref.py (a dense Kalman filter that blanks rows t - k + 1 .. t - 1 and filters the track again, per target and
horizon), the call's host plan (csrc/ssde_smooth_plan.hpp), and the stand-alone sanitizer program.

Limits: loo_cases' (test_loo_host.py's twin-versus-definition limits): z at RESID_TOL = 1e-9, lpd and the sums of the statistics at
LPD_TOL (1 + max|ref|) = 1e-11 (1 + max|ref|); NaN patterns, scored counts and threshold counts exactly (the thresholds lie midway
between neighbouring reference q)."""
import subprocess

import numpy as np
import pytest

import aheadsim_lib as AS
import loo_cases as LC
from ahead_ref import ahead_ref
from cases import make_spec, problem_from_spec

HORIZONS = (1, 2, 5, 33)
_REF = {}


def _lengths():
    return [1, 2, 3, 14, 2 * AS.block() + 5]


def _case(model, d):
    """irregular times, NA rows (inside the short and the long track, one ending the 14-row track), a per-row H_array; tracks of
    1, 2, 3, 14 and 2 blocks + 5 rows.  (pb, par, thresholds, ahead_ref): computed once, shared, never changed."""
    key = (model, d)
    if key not in _REF:
        lengths = _lengths()
        na = (4, 6 + 9, 6 + 13, 20 + 30, 20 + 31, 20 + 50)
        spec = make_spec(f"ahead_{model}_{d}", model, d, seed=300 + d, lengths=lengths, with_H=True, na_rows=na)
        pb, par = problem_from_spec(spec), np.asarray(spec["par"], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            thr = LC.midway_thresholds(ahead_ref(pb, par, HORIZONS)["q"].ravel())
        _REF[key] = (pb, par, thr, ahead_ref(pb, par, HORIZONS, thr))
    return _REF[key]


def compare(got, ref, gaps=None):
    """the twin's or the engine's outputs against a reference's: NaN patterns and counts exactly, values at loo_cases' limits"""
    note = (lambda k, v: gaps.__setitem__(k, max(gaps.get(k, 0.0), v))) if gaps is not None else (lambda k, v: None)
    for key, tol, rel in (("z", LC.RESID_TOL, False), ("lpd", LC.LPD_TOL, True)):
        g, r = got.get(key), ref[key]
        if g is None:
            continue
        assert g.shape == r.shape, (key, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (key, np.argwhere(np.isnan(g) != np.isnan(r))[:8])
        ok = ~np.isnan(r)
        if ok.any():
            scale = 1.0 + np.max(np.abs(r[ok])) if rel else 1.0
            err = np.max(np.abs(g[ok] - r[ok]))
            note(key, err / scale)
            assert err <= tol * scale, (key, err, tol * scale)
    if got.get("stats") is None:
        return
    gs, rs = got["stats"], ref["stats"]
    assert gs.shape == rs.shape, (gs.shape, rs.shape)
    assert np.array_equal(gs[..., 0], rs[..., 0]), "scored targets"
    assert np.array_equal(gs[..., 5:], rs[..., 5:]), "counts"
    for k in (1, 2, 3, 4):
        scale = 1.0 + np.max(np.abs(rs[..., k]))
        err = np.max(np.abs(gs[..., k] - rs[..., k]))
        note(f"stats{k}", err / scale)
        assert err <= LC.LPD_TOL * scale, (k, err, LC.LPD_TOL * scale)


@pytest.mark.parametrize("model,d", [("CTCRW", 2), ("OU_SSM", 1), ("BM_SSM", 2)])
def test_twin_is_the_definition(model, d):
    pb, par, thr, ref = _case(model, d)
    got = AS.forecast_scores(pb, par, HORIZONS, thr)
    gaps = {}
    compare(got, ref, gaps)
    print("GAPS", model, d, {k: f"{v:.1e}" for k, v in gaps.items()})
    # what the definition says about these tracks
    bounds = list(pb.seg_start) + [pb.n]
    assert np.all(ref["stats"][0] == 0.0)                                   # the one-row track
    assert ref["stats"][1, 0, 0] == 1 and np.all(ref["stats"][1, 1:, 0] == 0)   # two rows: one target at horizon 1, none later
    assert np.all(ref["stats"][3, 3] == 0.0) and ref["stats"][4, 3, 0] > 0      # horizon 33 reaches the long track only
    for j, k in enumerate(HORIZONS):
        for m in range(pb.n_seg):
            assert np.all(np.isnan(ref["lpd"][bounds[m]:min(bounds[m] + k, bounds[m + 1]), j]))
    assert np.all(np.isnan(ref["lpd"][[4, 15, 19, 50, 51, 70]]))            # NA targets
    assert np.isfinite(ref["lpd"][52, 1]) and np.isfinite(ref["lpd"][52, 2])    # ... are stepped through as intermediate rows
    # a chain that crosses a block boundary: start in block 0, target in block 1 of the long track
    blk = AS.block()
    assert np.isfinite(ref["lpd"][20 + blk + 3, 2]) and np.isfinite(ref["lpd"][20 + 2 * blk + 2, 3])


def test_outputs_alone_are_the_full_calls_and_repeat():
    pb, par, thr, _ = _case("CTCRW", 2)
    a = AS.forecast_scores(pb, par, HORIZONS, thr)
    b = AS.forecast_scores(pb, par, HORIZONS, thr)
    for k in ("z", "lpd", "stats"):
        assert np.array_equal(a[k], b[k], equal_nan=True)
    # a horizon list that is a subset gives the same columns: one chain serves all horizons
    c = AS.forecast_scores(pb, par, (2, 33), thr)
    assert np.array_equal(c["z"], a["z"][:, [1, 3]], equal_nan=True) and np.array_equal(c["stats"], a["stats"][:, [1, 3]])


def test_horizon_one_is_the_filters_innovation():
    from smooth_ref import smooth_ref
    for model, d in (("CTCRW", 2), ("OU_SSM", 1), ("BM_SSM", 2)):
        pb, par, _, ref = _case(model, d)
        sm = smooth_ref(pb, par)
        assert np.array_equal(np.isnan(ref["z"][:, 0]), np.isnan(sm["resid"]))
        ok = ~np.isnan(sm["resid"])
        assert np.max(np.abs(ref["z"][:, 0][ok] - sm["resid"][ok])) <= LC.RESID_TOL


# ---- the host plan --------------------------------------------------------------------------------------------------------------
def test_block_counts():
    lib, B = AS.load(), AS.block()
    assert B == 32
    assert [lib.hostsim_ahead_blocks(s) for s in (0, 1, B - 1, B, B + 1, 2 * B, 2 * B + 4)] == [0, 1, 1, 1, 2, 2, 3]
    assert list(AS.block_offsets([1, B, B + 1, 0, 2 * B + 4])) == [0, 1, 2, 4, 4, 7]


def test_budget_accounting():
    lib, B = AS.load(), AS.block()
    # a group's partial records: blocks x n_h x n_stat x 64 doubles
    assert lib.hostsim_ahead_partial_doubles(B + 1, 4, 13) == 2 * 4 * 13 * 64
    assert lib.hostsim_ahead_partial_doubles(0, 4, 13) == 0
    # three groups of 68, 13 and 2 state rows, CTCRW d = 2 (R = 31, SW = 11), four horizons, thirteen statistics
    steps, R, SW, nh, ns = [68, 13, 2], 31, 11, 4, 13
    cost = [s * (R + SW) * 64 + lib.hostsim_ahead_partial_doubles(s, nh, ns) for s in steps]
    assert cost[0] == 68 * 42 * 64 + 3 * 4 * 13 * 64
    assert AS.chunks(steps, R, SW, nh, ns, sum(cost)) == [0, 3]                     # everything fits
    assert AS.chunks(steps, R, SW, nh, ns, sum(cost) - 1) == [0, 2, 3]              # one double short: the last group alone
    assert AS.chunks(steps, R, SW, nh, ns, cost[0] + cost[1] - 1) == [0, 1, 3]      # the partial records count
    assert AS.chunks(steps, R, SW, nh, ns, 1) == [0, 1, 2, 3]                       # a group always goes
    # without statistics the partial records cost nothing: n_stat = 0
    assert AS.chunks(steps, R, SW, nh, 0, (68 + 13) * 42 * 64) == [0, 2, 3]


@pytest.mark.parametrize("hz,code", [((1, 2, 5, 33), 0), ((64,), 0), (tuple(range(1, 9)), 0), ((), 1), (tuple(range(1, 10)), 1), (None, 1),
                                     ((0,), 2), ((-1, 2), 2), ((1, 65), 2), ((2, 2), 3), ((5, 2), 3), ((1, 3, 3, 7), 3)])
def test_horizon_lists(hz, code):
    assert AS.check_horizons(hz) == code


# ---- the sanitizer program ------------------------------------------------------------------------------------------------------
def test_the_sanitizer_program_runs_clean():
    AS.load()
    r = subprocess.run([AS.SAN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ahead_san ok" in r.stdout and r.stderr == "", (r.returncode, r.stdout, r.stderr)
