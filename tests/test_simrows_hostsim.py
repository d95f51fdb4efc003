"""CPU suite: the lane math of ssde_simulate_rows (csrc/ssde_simrows.hpp), built with g++ (tests/hostsim/hostsim_simrows.cpp through
tests/simrowsim_lib.py), against the numpy definition (tests/simrows_ref.py) on the cases of tests/simrows_cases.py with the limits
of simrows_cases.compare; the float64 definition against the long double one; the forms of the factors against the literal formulas
in long double; the stand-alone sanitizer program."""
import subprocess

import numpy as np
import pytest

import simrowsim_lib
from simrows_cases import CASES, case, compare, ref_args, ref_kwargs, reference
from simrows_ref import simrows_ref

U = 2.0 ** -53


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_against_the_definition(name):
    c = case(name)
    got = simrowsim_lib.simulate_rows(*ref_args(c), thr=c["thr"], **ref_kwargs(c))
    compare(got, reference(name), c, name)
    # an empty track writes nothing (the twin's buffer starts as NaN and every row belongs to a track: none is left)
    assert not np.isnan(got["obs"]).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_float64_against_long_double(name):
    """A step rounds the state by a few u of its size (exp, expm1, sqrt, log, cos at about one ulp each and six fma): 16 u a row is
    generous, and the roundings add up linearly at worst over the T rows of the longest track: 16 T u (1 + max|y|) for obs, that
    times the track's rows for the sums."""
    c, ref = case(name), reference(name)
    ld = simrows_ref(*ref_args(c), thr=c["thr"], dtype=np.longdouble, **ref_kwargs(c))
    T = float(max(c["lengths"].max(), 1))
    lim = 16.0 * T * U * (1.0 + float(np.nanmax(np.abs(ref["obs"]))))
    gap = float(np.nanmax(np.abs(ld["obs"] - ref["obs"])))
    d = c["n_dim"]
    sums = [3 * cc + k for cc in range(d) for k in range(3)] + [3 * d]
    assert np.array_equal(np.isnan(ld["stats"]), np.isnan(ref["stats"]))
    with np.errstate(invalid="ignore"):
        sgap = np.abs(ld["stats"] - ref["stats"]).astype(np.float64)
    lim_t = lim * np.maximum(c["lengths"], 1)[None, :, None]
    worst_s = float(np.nanmax(sgap[:, :, sums] / lim_t, initial=0.0))
    print(f"simrows {name}: float64 against long double: obs {gap / lim:.3g}, sums {worst_s:.3g} of the limit")
    assert gap <= lim and worst_s <= 1.0
    assert float(np.nanmax(sgap[:, :, 3 * d + 1], initial=0.0)) <= lim
    assert float(np.nanmax(sgap[:, :, 3 * d + 2:], initial=0.0)) == 0.0


@pytest.mark.parametrize("x", [1e-6, 1e-3, 0.2, 0.25, 0.3, 2.0, 40.0, 1e3])
def test_ctcrw_factors_against_the_literal_formulas(x):
    """simrows_factors at beta dt = x against R/sde.R:1465-1468 and CTCRW_cov (R/utility.R:188-196) evaluated as written, in long
    double.  1 - e and the two covariance entries that have one difference: to 64 u (the literal long double forms lose
    2^-64 / x there: 5e-14 at 1e-6).  The position variance as written cancels to 3 u_ld / x^2 -- useless at 1e-6 even in long double
    -- so it is held against its own series in long double (x^3 / 3 - x^4 / 4 + 7 x^5 / 60 - ...), to 1e-13 relative."""
    ld = np.longdouble
    tau, nu = 1.7, 0.8
    dt = x * tau
    F = simrowsim_lib.factors("CTCRW", dt, tau, nu)
    beta, sigma = 1 / ld(tau), 2 * ld(nu) / np.sqrt(ld(tau) * ld("3.14159265358979323846264338327950288"))
    xx = beta * ld(dt)
    e, e2 = np.exp(-xx), np.exp(-2 * xx)
    lim = max(64 * U, 2.0 ** -62 / x)
    assert abs(F["ome"] - (1 - e)) <= lim * float(1 - e)
    assert abs(F["e"] - e) <= 4 * U
    qvv = sigma ** 2 / (2 * beta) * (1 - e2)
    qvz = sigma ** 2 / (2 * beta ** 2) * (1 - 2 * e + e2)
    assert abs(F["l11"] - np.sqrt(qvv)) <= lim * float(np.sqrt(qvv))
    assert abs(F["l21"] - qvz / np.sqrt(qvv)) <= max(lim, 2.0 ** -60 / x ** 2) * float(qvz / np.sqrt(qvv))
    if x < 0.5:
        import math
        G = sum(ld((-1) ** (k + 1) * (2 ** (k - 1) - 2)) / ld(math.factorial(k)) * xx ** k for k in range(3, 40))
    else:
        G = xx + (1 - e2) / 2 - 2 * (1 - e)
    qzz = (sigma / beta) ** 2 / beta * G
    # (the two entries under the root from expm1 in long double: as written, 1 - 2 e + e^2 is already off by 2^-60 / x^2)
    l21sq = (sigma ** 2 / (2 * beta ** 2) * np.expm1(-xx) ** 2) ** 2 / (sigma ** 2 / (2 * beta) * -np.expm1(-2 * xx))
    l22 = np.sqrt(qzz - l21sq)
    assert abs(F["l22"] - l22) <= 1e-13 * float(l22), (F["l22"], float(l22))
    assert abs(F["a"] - (1 - e) / beta) <= lim * float((1 - e) / beta)


def test_ou_and_bm_factors():
    ld = np.longdouble
    for x in (1e-6, 0.3, 50.0):
        tau, kappa = 2.5, 0.7
        F = simrowsim_lib.factors("OU", x * tau, tau, kappa)
        sd = np.sqrt(ld(kappa) * (1 - np.exp(-2 * ld(x * tau) / ld(tau))))
        assert abs(F["sd"] - sd) <= max(64 * U, 2.0 ** -62 / x) * float(sd)
    F = simrowsim_lib.factors("BM", 0.37, 1.3)
    assert abs(F["sd"] - 1.3 * np.sqrt(0.37)) <= 4 * U * 1.3


def test_the_sanitizer_program_runs_clean():
    """tests/hostsim/simrows_san: the twin's walk on small problems (tracks of 0, 1, 2, 5 and 33 rows, the three recursions, one
    replicate alone against the batch, a blown-up parameter), built with -fsanitize=address,undefined, run as a program"""
    simrowsim_lib.load()
    r = subprocess.run([simrowsim_lib.SAN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "simrows_san ok" in r.stdout, (r.stdout, r.stderr)
