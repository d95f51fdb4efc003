"""CPU suite: the lane math of ssde_par_bands (csrc/ssde_bands.hpp), built with g++ (tests/hostsim/hostsim_bands.cpp through
tests/bandsim_lib.py), against the definition (tests/bands_ref.py) on the cases of tests/bands_cases.py, with the limits of
bands_cases.compare: 4 (K + 4) u S_i per row for est, pw_*, se and max_dev, and max(1e-12, 64 g) (1 + max|ref|) for crit and sim_*
with g the gap between the float64 and the long double definition."""
import subprocess

import numpy as np
import pytest

import bandsim_lib
from bands_cases import CASES, case, compare, make_case, ref_args
from bands_ref import bands_ref, tail_sizes


def _check(c, tag):
    ref = bands_ref(*ref_args(c), resp=c["resp"])
    ref_ld = bands_ref(*ref_args(c), resp=c["resp"], dtype=np.longdouble)
    got = bandsim_lib.par_bands(*ref_args(c), resp=c["resp"])
    compare(got, ref, ref_ld, c, tag)
    return got, ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_against_the_definition(name):
    _check(case(name), name)


def test_a_tail_of_exactly_64():
    assert bandsim_lib.plan(2500, 0.95) == (64, 64) == tail_sizes(2500, 0.95)
    assert bandsim_lib.plan(1000, 0.90) == (51, 51) and bandsim_lib.plan(1000, 0.5)[0] == 251 and bandsim_lib.plan(2540, 0.95)[0] == 65
    _check(make_case(3, 2500, [(2, 1), (0, 0)], [1, 0], seed=64), "tail 64")


def test_ties_collapse_and_nan_rows():
    c = make_case(9, 40, [(2, 2), (3, 0), (0, 0)], [1, 0, 1], seed=5)
    c["coeff"] = np.vstack([c["coeff"][:1], np.repeat(c["coeff"][1:21], 2, axis=0)])       # every draw twice
    c["coeff"][1:, 4:7] = c["coeff"][0, 4:7]                                                # parameter 1 has no spread
    c["X_fe"][0][6, 1] = np.nan
    got, ref = _check(c, "ties / collapse / NaN")
    assert np.all(got["se"][:, 1] == 0.0) and got["crit"][1] == 0.0 and np.all(got["max_dev"][1] == 0.0)
    for k in ("pw_low", "pw_upp", "sim_low", "sim_upp"):
        assert np.array_equal(got[k][:, 1], got["est"][:, 1]), k
    for k in ("est", "pw_low", "pw_upp", "se", "sim_low", "sim_upp"):
        assert np.isnan(got[k][6, 0]) and np.isnan(got[k]).sum() == 1, k


def test_se_zero_with_a_deviation_is_inf():
    coeff = np.array([[1.0], [4.0], [1.0], [5.0], [2.0], [3.0]])
    coeff[0, 0] = bandsim_lib.par_bands([None], [None], [0], coeff, 0.95, 1.96)["pw_low"][0, 0]
    got = bandsim_lib.par_bands([None], [None], [0], coeff, 0.95, 1.96)
    assert got["se"][0, 0] == 0.0 and np.all(np.isinf(got["max_dev"][0])) and np.isinf(got["crit"][0])


def test_the_sanitizer_program_runs_clean():
    """tests/hostsim/bands_san: the twin's walk on small problems (tails of 2 and 64, ties, a NaN row), every tail buffer checked after
    every insert, built with -fsanitize=address,undefined, run as a program"""
    bandsim_lib.load()
    r = subprocess.run([bandsim_lib.SAN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bands_san ok" in r.stdout, (r.stdout, r.stderr)
