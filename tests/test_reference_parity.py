"""CPU suite: the oracle (oracle/ssde_oracle.hpp, the project's restatement) against the REFERENCE's own likelihood sources,
compiled unmodified behind the TMB stand-in (oracle/tmb_shim/, oracle/ref_capi.cpp -> oracle/_ref/; tests/reference_lib.py).

What this pins: the oracle's READING of src/nllk/*.hpp -- which interval a row uses, what the detF <= 0 branch drops, which
column decides missingness, how the a0 counter advances, which constants each penalty adds.  Every other check of the oracle
(joint Gaussian, autograd, binary128) shares its reading; this one does not.  What stays a restatement: the TMB / Eigen semantics
inside the stand-in and the R-side assembly of tmb_dat in ref_capi.cpp, a0 / P0 defaults included (tools/tmb_oracle.R is the
check of those against real TMB).

Bounds.  binary128 against binary128: both sides evaluate the same formulas in 113 bits and round once to double, so they may
differ by an ulp or so of double: <= 4 ulp relative.  double against double: each side is within 1e-12 (value) / 1e-9 (gradient)
of its binary128 evaluation (tests/test_oracle_quad.py), hence 2e-12 * max(1, |v|) and 2e-9 * max(1, max|g|).  aest_all: the
tolerance of test_gpu_parity.py::test_report_aest_all.  Largest gaps measured: oracle/README.md."""
import json
import os

import numpy as np
import pytest

import reference_lib
from cases import problem_from_spec
from golden_io import dec, load_golden
from oracle_lib import oracle_eval, oracle_eval_quad
from reference_lib import ref_eval, ref_eval_quad
from smoothsde_amd import capi
from smoothsde_amd.synth import bspline_basis, second_difference_penalty

pytestmark = pytest.mark.skipif(not reference_lib.available(),
                                reason="reference checkout absent and oracle/_ref/ not built")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = load_golden()
UNSTABLE = [dec(r) for r in json.load(open(os.path.join(HERE, "golden", "unstable_cases.json")))]
KALMAN = [r for r in GOLD if r["model"] in ("CTCRW", "OU_SSM", "BM_SSM")]
EPS = float(np.finfo(np.float64).eps)


def _ulps(a, b):
    return abs(a - b) / (EPS * abs(b))


def _assert_exact_pair(pb, par, label):
    """reference in binary128 == oracle in binary128, to 4 ulp of double (both NaN counts as agreement, one NaN does not)"""
    qr = ref_eval_quad(pb, par, order=0)
    qo = oracle_eval_quad(pb, par, order=0)
    if np.isnan(qr) or np.isnan(qo):
        assert np.isnan(qr) and np.isnan(qo), (label, qr, qo)
        print(f"{label}: binary128 pair both NaN")
        return qr
    print(f"{label}: binary128 reference {qr!r} oracle {qo!r} gap {_ulps(qo, qr):.2f} ulp")
    assert abs(qo - qr) <= 4 * EPS * abs(qr), (label, qr, qo)
    return qr


def _assert_double_pair(pb, par, label):
    vr, gr = ref_eval(pb, par, order=1)
    vo, go = oracle_eval(pb, par, order=1)
    if np.isnan(vr) or np.isnan(vo):
        assert np.isnan(vr) and np.isnan(vo), (label, vr, vo)
        print(f"{label}: double pair both NaN")
        return vr
    dv = abs(vo - vr) / max(1.0, abs(vr))
    dg = np.max(np.abs(go - gr)) / max(1.0, np.max(np.abs(gr)))
    print(f"{label}: double value gap {dv:.2e}, gradient gap {dg:.2e}")
    assert abs(vo - vr) <= 2e-12 * max(1.0, abs(vr)), (label, vr, vo)
    assert np.max(np.abs(go - gr)) <= 2e-9 * max(1.0, np.max(np.abs(gr))), (label, gr, go)
    assert np.all(gr[np.asarray(pb.par_fixed) != 0] == 0.0), label
    return vr


def _assert_report_pair(pb, par, label):
    _, _, ar = ref_eval(pb, par, order=1, report=True)
    _, _, ao = oracle_eval(pb, par, order=1, report=True)
    assert ar.shape == ao.shape == (pb.n, pb.sdim)
    assert np.allclose(ao, ar, rtol=1e-10, atol=1e-10, equal_nan=True), (label, np.nanmax(np.abs(ao - ar)))
    return ar


# ---- (a) every golden case and every unstable case ------------------------------------------------------------------------------

@pytest.mark.parametrize("rec", GOLD, ids=[r["name"] for r in GOLD])
def test_golden_case_reference_equals_oracle(rec):
    pb = problem_from_spec(rec)
    _assert_exact_pair(pb, rec["par"], rec["name"])
    vr = _assert_double_pair(pb, rec["par"], rec["name"])
    # no golden case needs the documented CIR deviation (a reference value that overflowed): every one is finite in the reference
    assert np.isfinite(vr), rec["name"]


@pytest.mark.parametrize("rec", UNSTABLE, ids=[r["name"] for r in UNSTABLE])
def test_unstable_case_reference_equals_oracle_in_binary128(rec):
    """the four fixtures of DESIGN 5c (a coupling H_array / P0 on 200-row tracks): the literal recursion in double is roundoff
    there on either side, so only the binary128 pair is compared"""
    pb = problem_from_spec(rec)
    _assert_exact_pair(pb, rec["par"], rec["name"])


# ---- (b) REPORT(aest_all), every row ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rec", KALMAN, ids=[r["name"] for r in KALMAN])
def test_golden_case_reference_report_equals_oracle_report(rec):
    pb = problem_from_spec(rec)
    ar = _assert_report_pair(pb, rec["par"], rec["name"])
    # the rows compared include every track's last row, whose predict uses the interval to the NEXT track's first time (Q4)
    last = np.r_[pb.seg_start[1:] - 1, pb.n - 1]
    assert np.all(np.isfinite(ar[last[np.diff(np.r_[pb.seg_start, pb.n]) > 1]]))


# ---- (c) the quirk battery: one small hand-made case per reading, each shown to discriminate --------------------------------------

def _moved(a, b):
    """the value moved by more than 1e-3 relative (finite against non-finite counts as moved)"""
    return not (abs(a - b) <= 1e-3 * max(abs(a), abs(b)))


def _grid(lengths, d, seed):
    rng = np.random.default_rng(seed)
    ID = np.concatenate([np.full(T, float(k)) for k, T in enumerate(lengths)])
    n = len(ID)
    times = np.cumsum(rng.uniform(0.4, 1.6, size=n))
    obs = np.cumsum(rng.standard_normal((n, d)) * 0.5, axis=0)
    return ID, times, obs, rng


def _check(case, variant, label):
    """case / variant: (Problem, par).  Reference against oracle on both as in (a); the variant (the case with its trigger
    removed) must move the reference's value by more than 1e-3 relative."""
    vals = []
    for tag, (pb, par) in (("case", case), ("variant", variant)):
        par = np.asarray(par, dtype=np.float64)
        _assert_exact_pair(pb, par, f"{label}/{tag}")
        vals.append(_assert_double_pair(pb, par, f"{label}/{tag}"))
    assert _moved(vals[0], vals[1]), (label, vals)
    return vals


def _detf_case(model, drift):
    """F = P0[0, 0] + H_array[1] = 0 exactly at a track's second row: det F = 0 takes the detF <= 0 branch (for OU_SSM / BM_SSM
    through exp(log|0|) = 0)."""
    ID, times, obs, _ = _grid([6, 5], 1, seed=5)
    n = len(ID)
    p00 = 1.0 if model == "CTCRW" else 10.0             # the default P0's first entry
    H = np.full((1, 1, n), 0.04)
    H[0, 0, 1] = -p00
    pb = capi.Problem(model, ID, times, obs, H=H, par_fixed=np.array([1] + [0] * capi.n_sde_par(model, 1), dtype=np.uint8), na_mode=0)
    par = [0.0, drift, 0.3] + ([0.2] if model != "BM_SSM" else [])
    return pb, np.array(par)


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM", "BM_SSM"])
def test_quirk_detF_nonpositive_branch_with_a_drift(model):
    """Q3: CTCRW's branch predicts with a <- T a, dropping B mu; OU_SSM / BM_SSM keep the drift.  The drift is 3 per unit time
    against fixes precise to 0.2, so the row after the branch is scored at a visibly different state either way."""
    case = _detf_case(model, 3.0)
    _check(case, _detf_case(model, 0.0), f"detF<=0 {model}")
    # ... and the branch itself is in the number: an ordinary H at that row gives another value
    pb, par = case
    H2 = pb.H.copy()
    H2[0, 0, 1] = 0.04
    pb2 = capi.Problem(model, pb.id, pb.times, pb.obs, H=H2, par_fixed=pb.par_fixed, na_mode=0)
    assert _moved(ref_eval(pb, par, order=0), ref_eval(pb2, par, order=0))


def _na_problem(model, row, col, na, na_mode=0):
    ID, times, obs, _ = _grid([7, 6], 2, seed=11)
    obs = obs.copy()
    obs[row, col] = na
    pb = capi.Problem(model, ID, times, obs, na_mode=na_mode)
    par = {"CTCRW": [-0.5, 0.1, -0.1, 0.3, 0.2], "OU_SSM": [-0.5, 0.4, -0.2, 0.5, 0.1], "BM": [0.1, -0.1, 0.2]}[model]
    return pb, np.array(par)


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM"])
def test_quirk_missingness_is_decided_by_column_0(model):
    """Q5: NA in column 1 only is NOT a missing row for the Kalman families (the NA enters the innovation: NaN); NA in column 0
    only IS one, although column 1 holds a fix (the row is skipped, the fix unused)."""
    na = capi.na_real()
    vals = _check(_na_problem(model, 3, 1, na), _na_problem(model, 3, 0, na), f"NA col 1 only {model}")
    assert np.isnan(vals[0]) and np.isfinite(vals[1])
    # column 0 NA with column 1 observed against the complete row: the skipped fix is in the number
    ID, times, obs, _ = _grid([7, 6], 2, seed=11)
    pb_full = capi.Problem(model, ID, times, obs, na_mode=0)
    _check(_na_problem(model, 3, 0, na), (pb_full, _na_problem(model, 3, 0, na)[1]), f"NA col 0 only {model}")


def test_quirk_direct_families_test_each_column():
    """Q5, nllk_sde: each dimension of both endpoints is tested on its own -- NA in column 1 drops that dimension of the two
    transitions it touches and keeps column 0's"""
    na = capi.na_real()
    _check(_na_problem("BM", 3, 1, na), _na_problem("BM", 3, 0, na), "NA col 1 only BM")


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM"])
def test_quirk_plain_nan_is_not_na_real(model):
    """Q5: R_IsNA is true for NA_real_ only (low word 1954); a plain NaN in column 0 is an observation and poisons the value"""
    vals = _check(_na_problem(model, 4, 0, float("nan")), _na_problem(model, 4, 0, capi.na_real()), f"plain NaN {model}")
    assert np.isnan(vals[0]) and np.isfinite(vals[1])


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM", "BM_SSM"])
def test_quirk_reappearing_id_consumes_the_next_a0_row(model):
    """Q9: IDs 0, 1, 0 are three segments; the third starts from a0 row 2, not from row 0 again"""
    rng = np.random.default_rng(21)
    ID = np.repeat([0.0, 1.0, 0.0], [5, 4, 5])
    n = len(ID)
    times = np.cumsum(rng.uniform(0.5, 1.5, size=n))
    obs = np.cumsum(rng.standard_normal((n, 1)) * 0.4, axis=0)
    sdim = capi.state_dim(model, 1)
    a0 = np.zeros((3, sdim))
    a0[:, 0] = [obs[0, 0] + 0.5, obs[5, 0] - 0.7, obs[9, 0] + 2.0]
    par = np.array([-0.8, 0.1, 0.3] + ([0.1] if model != "BM_SSM" else []))
    a0_again = a0.copy()
    a0_again[2] = a0[0]
    _check((capi.Problem(model, ID, times, obs, a0=a0), par), (capi.Problem(model, ID, times, obs, a0=a0_again), par),
           f"reappearing ID {model}")


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM", "BM_SSM"])
@pytest.mark.parametrize("gap", [-3.0, 1048576.0])
def test_quirk_cross_track_interval_at_a_tracks_last_row(model, gap):
    """Q4: the last row of a track predicts over dtimes(i) = (next track's first time) - (its own time), negative when times
    restart and huge after a long pause; the state is discarded by the re-initialisation but REPORTed.  The number the quirk
    decides is aest_all's last row of the first track; the value must not depend on the interval at all."""
    rng = np.random.default_rng(31)
    ID = np.repeat([0.0, 1.0], [6, 6])
    t1 = np.cumsum(rng.integers(4, 13, size=6) / 8.0)       # eighths: every time and interval below is exact in double
    t2 = np.cumsum(rng.integers(4, 13, size=6) / 8.0)
    obs = np.cumsum(rng.standard_normal((12, 1)) * 0.4, axis=0)
    par = np.array([-0.8, 0.4, 0.3] + ([0.1] if model != "BM_SSM" else []))
    out = {}
    for tag, g in (("case", gap), ("variant", 1.0)):
        times = np.r_[t1, t1[-1] + g + (t2 - t2[0])]
        pb = capi.Problem(model, ID, times, obs)
        _assert_exact_pair(pb, par, f"cross-track {model} {gap} {tag}")
        v = _assert_double_pair(pb, par, f"cross-track {model} {gap} {tag}")
        out[tag] = (v, _assert_report_pair(pb, par, f"cross-track {model} {gap} {tag}"))
    assert out["case"][0] == out["variant"][0]
    a, b = out["case"][1][5, 0], out["variant"][1][5, 0]
    assert np.isfinite(a) and np.isfinite(b) and _moved(a, b), (a, b)
    assert np.array_equal(np.delete(out["case"][1], 5, axis=0), np.delete(out["variant"][1], 5, axis=0))


def _smooth_problem(model, d, include_penalty=1, s_scale=1.0, two=False, seed=41, decay=None):
    ID, times, obs, rng = _grid([9, 8], d, seed=seed)
    if model == "CIR":
        obs = np.exp(0.3 * obs)
    n = len(ID)
    q = capi.n_sde_par(model, d)
    x = np.clip((np.sin(np.linspace(0, 6, n)) + 1) / 2, 0, 1)
    X_re = [None] * q
    X_re[0] = bspline_basis(x, n_basis=4)
    S_list = [s_scale * second_difference_penalty(4)]
    if two:
        X_re[q - 1] = bspline_basis(np.clip(x ** 2, 0, 1), n_basis=5)
        S_list.append(s_scale * second_difference_penalty(5))
    kw = {}
    if decay is not None:
        kw = dict(t_decay=np.linspace(0.0, 2.0, q * n), col_decay=np.arange(9, dtype=np.int32), ind_decay=np.asarray(decay, dtype=np.int32))
    pb = capi.Problem(model, ID, times, obs, X_re=X_re, S_list=S_list, include_penalty=include_penalty, **kw)
    par = np.zeros(pb.n_par_full)
    par[:pb.off_lambda] = 0.2
    par[pb.off_lambda:pb.off_lambda + pb.n_smooth] = [0.7, -0.9][:pb.n_smooth]
    if decay is not None:
        par[pb.off_lambda + pb.n_smooth:pb.off_re] = [0.4, -1.2][:pb.n_decay]
    par[pb.off_re:] = 0.8 * np.cos(1.0 + np.arange(pb.n_re))
    return pb, par


@pytest.mark.parametrize("model", ["CTCRW", "OU_SSM", "BM_SSM"])
def test_quirk_include_penalty_is_ignored_by_the_kalman_families(model):
    """Q7: the state-space templates declare no include_penalty: 0 and 1 give the same number, penalty included -- and the
    penalty is a visible part of it (a penalty matrix a thousand times larger moves the value)"""
    off, par = _smooth_problem(model, 1, include_penalty=0)
    on, _ = _smooth_problem(model, 1, include_penalty=1)
    big, _ = _smooth_problem(model, 1, include_penalty=0, s_scale=1000.0)
    _check((off, par), (big, par), f"include_penalty=0 {model}")
    assert ref_eval(off, par, order=0) == ref_eval(on, par, order=0)
    assert oracle_eval(off, par, order=0) == oracle_eval(on, par, order=0)


@pytest.mark.parametrize("model", ["BM", "OU"])
def test_quirk_include_penalty_gates_the_direct_families(model):
    """Q7: nllk_sde adds its penalty (with the Gaussian normalising constants) only when include_penalty is set"""
    off, par = _smooth_problem(model, 1, include_penalty=0)
    on, _ = _smooth_problem(model, 1, include_penalty=1)
    _check((off, par), (on, par), f"include_penalty=0 {model}")


@pytest.mark.parametrize("model", ["CTCRW", "OU"])
def test_quirk_penalty_with_two_smooths(model):
    """each smooth takes its own log_lambda, its own block of S and its own slice of coeff_re, in order: exchanging the two
    log_lambda moves the value"""
    pb, par = _smooth_problem(model, 1, two=True)
    swapped = par.copy()
    swapped[pb.off_lambda:pb.off_lambda + 2] = par[pb.off_lambda:pb.off_lambda + 2][::-1]
    _check((pb, par), (pb, swapped), f"two smooths {model}")


def test_quirk_decaying_columns_with_two_rates():
    """nllk_sde.hpp:47-58: column col_decay(i) decays with rate ind_decay(i) (both 1-based in tmb_dat); with every column on the
    first rate the value is another"""
    two = _smooth_problem("BM", 1, two=True, decay=[0, 0, 0, 0, 1, 1, 1, 1, 1])
    one = _smooth_problem("BM", 1, two=True, decay=[0] * 9)
    assert two[0].n_decay == 2 and one[0].n_decay == 1
    _check(two, one, "decay two rates")


def test_quirk_bm_t():
    """tr_dens.hpp:38-44: Student-t increments, scale = sd / sqrt(df / (df - 2)); against the Gaussian BM on the same data"""
    ID, times, obs, _ = _grid([9, 7], 1, seed=51)
    par = np.array([0.15, -0.2])
    _check((capi.Problem("BM_t", ID, times, obs, other_data=np.array([3.5])), par), (capi.Problem("BM", ID, times, obs), par), "BM_t")


def test_quirk_cir_uses_the_parameters_of_row_i_minus_1():
    """tr_dens.hpp:53-67 through nllk_sde.hpp:80-81 (Q6): the transition into row i takes par_mat.row(i - 1); a covariate
    shifted by one row gives another value"""
    ID, times, obs, rng = _grid([10, 8], 1, seed=61)
    obs = np.exp(0.3 * obs)
    n = len(ID)
    x = rng.uniform(0.0, 1.0, size=n)
    par = np.array([0.2, 0.9, -0.4, -0.7])

    def pb(cov):
        return capi.Problem("CIR", ID, times, obs, X_fe=[np.column_stack([np.ones(n), cov]), None, None])

    _check((pb(x), par), (pb(np.roll(x, -1)), par), "CIR row i-1")


def test_quirk_eseal_ssm():
    """nllk_e_seal_ssm.hpp: Z_i = (a1, a2 / R_i), H_i = tau^2 / h_i at row i, the two inverse-gamma priors; R shifted by one
    row gives another value"""
    rng = np.random.default_rng(71)
    lengths = [8, 7]
    ID = np.repeat([0.0, 1.0], lengths)
    n = len(ID)
    times = np.cumsum(rng.uniform(0.7, 1.5, size=n))
    L = 30.0 + np.cumsum(0.3 + 0.4 * rng.standard_normal(n))
    R = rng.uniform(60.0, 250.0, size=n)
    h = rng.integers(200, 400, size=n).astype(float)       # many dives a day: fixes precise enough for R_i to show in the value
    y = (-0.578 + 1.214 * L / R + rng.standard_normal(n) / np.sqrt(h))[:, None]
    a0 = np.column_stack([np.ones(2), [L[0], L[lengths[0]]]])
    par = np.array([-1.0, -0.55, 0.2, 0.3, -0.8])

    def pb(Rv):
        return capi.Problem("ESEAL_SSM", ID, times, y, a0=a0, eseal_h=h, eseal_R=Rv)

    _check((pb(R), par), (pb(np.roll(R, 1)), par), "ESEAL_SSM")


def test_quirk_three_columns_with_a_coupling_H_array():
    """nllk_ctcrw.hpp:12-24, 203-205: beyond two columns det F comes from the LU, and H_array(, , i) enters whole; without its
    off-diagonal entries the value is another.  Short tracks: the literal recursion is still exact to rounding here."""
    ID, times, obs, rng = _grid([7, 6], 3, seed=81)
    n = len(ID)
    A = rng.standard_normal((n, 3, 3)) * 0.3
    H = np.einsum("nij,nkj->ikn", A, A) + 0.05 * np.eye(3)[:, :, None]
    Hd = H * np.eye(3)[:, :, None]
    fixed = np.array([1, 0, 0, 0, 0, 0], dtype=np.uint8)
    par = np.array([0.0, 0.1, -0.1, 0.05, 0.3, 0.2])
    _check((capi.Problem("CTCRW", ID, times, obs, H=H, par_fixed=fixed), par),
           (capi.Problem("CTCRW", ID, times, obs, H=Hd, par_fixed=fixed), par), "3 columns coupling H")


def test_quirk_first_observation_is_never_scored():
    """Q1: with a user a0 the first row of a track only (re)initialises the state -- its observation is in no term of the value"""
    ID, times, obs, _ = _grid([6, 5], 1, seed=91)
    a0 = np.array([[obs[0, 0], 0.0], [obs[6, 0], 0.0]])
    par = np.array([-0.7, 0.1, 0.3, 0.1])
    obs2 = obs.copy()
    obs2[0, 0] += 5.0
    a0_moved = a0 + np.array([[0.8, 0.0], [0.0, 0.0]])
    vals = _check((capi.Problem("CTCRW", ID, times, obs, a0=a0), par), (capi.Problem("CTCRW", ID, times, obs, a0=a0_moved), par), "first obs")
    assert ref_eval(capi.Problem("CTCRW", ID, times, obs2, a0=a0), par, order=0) == vals[0]
    assert oracle_eval(capi.Problem("CTCRW", ID, times, obs2, a0=a0), par, order=0) == oracle_eval(capi.Problem("CTCRW", ID, times, obs, a0=a0), par, order=0)


# ---- (5) the recorded reference results are what the reference's program computes ------------------------------------------------

def test_recorded_reference_results_equal_a_fresh_evaluation():
    """tests/golden/reference_results.json (tests/golden/gen_reference_results.py) against oracle/_ref/ now: bitwise with the same
    compiler and -ffp-contract=off; 4 ulp (of the entry, or of the largest entry of its array) are allowed and the largest gap
    is printed"""
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from gen_reference_results import PATH, reference_record
    stored = {r["name"]: r for r in (dec(r) for r in json.load(open(PATH)))}
    assert list(stored) == [r["name"] for r in GOLD]
    assert os.path.getsize(PATH) <= os.path.getsize(os.path.join(HERE, "golden", "cases.json"))
    worst = 0.0
    for rec in GOLD:
        fresh, kept = reference_record(rec), stored[rec["name"]]
        assert set(fresh) == set(kept), rec["name"]
        for key in fresh:
            if key == "name":
                continue
            a, b = np.asarray(fresh[key], dtype=np.float64), np.asarray(kept[key], dtype=np.float64)
            assert a.shape == b.shape, (rec["name"], key)
            assert np.array_equal(np.isnan(a), np.isnan(b)), (rec["name"], key)
            if a.size:
                scale = EPS * max(np.nanmax(np.abs(b)), np.finfo(np.float64).tiny)
                gap = np.nanmax(np.abs(a - b)) / scale
                worst = max(worst, gap)
                assert gap <= 4.0, (rec["name"], key, gap)
    print(f"recorded reference results: largest gap to a fresh evaluation {worst:.2f} ulp")
