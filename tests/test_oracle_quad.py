"""CPU suite: the double-precision oracle against the SAME restated templates evaluated in IEEE binary128
(oracle/oracle_quad.cpp, 113-bit mantissa, gradient by central differences of the binary128 function -- no dual numbers).

What this pins: the oracle's double arithmetic (rounding, summation order, the LU of F) and its forward-mode gradient
(oracle/dual.hpp) on every golden case -- at ordinary parameters the double-precision value sits within 1e-12 of the exact
value of the reference's formulas and the dual-number gradient within 1e-9 of the derivative of that exact function.
What it cannot pin: a misreading of the reference shared by both instantiations.  That is pinned elsewhere: the reference's
own likelihood sources, compiled unmodified behind a stand-in <TMB.hpp>, against this oracle in double and in binary128
(tests/test_reference_parity.py; oracle/README.md says what of TMB and of the R side stays a restatement).  The binary128
build is also the arbiter of tools/extreme_probe.py, where the literal double formulas are ill-conditioned and oracle and
engine disagree."""
import numpy as np
import pytest

from cases import problem_from_spec
from golden_io import load_golden
from oracle_lib import oracle_eval, oracle_eval_quad

GOLD = load_golden()


@pytest.mark.parametrize("rec", GOLD, ids=[r["name"] for r in GOLD])
def test_double_oracle_matches_binary128_evaluation(rec):
    pb = problem_from_spec(rec)
    par = rec["par"]
    v, g = oracle_eval(pb, par, order=1)
    qv, qg = oracle_eval_quad(pb, par)
    assert abs(v - qv) <= 1e-12 * max(1.0, abs(qv)), (v, qv)
    assert np.max(np.abs(g - qg)) <= 1e-9 * max(1.0, np.max(np.abs(qg))), (g, qg)
    # and the committed expectation (torch-autograd-pinned, tests/golden/gen_golden.py) agrees with the exact value
    assert abs(rec["expected"]["value"] - qv) <= 1e-10 * max(1.0, abs(qv))


def test_binary128_resolves_an_ill_conditioned_point():
    """BM_SSM with a process variance of e^200: the literal update P (T - K Z)' cancels, the double oracle is off by
    parts in 1e11 in the value and 1e6 in a gradient entry; the binary128 evaluation is what tells."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_fuzz import random_problem
    pb, par = random_problem(114)
    par = par.copy()
    par[3] = 100.0
    v, g = oracle_eval(pb, par, order=1)
    qv, qg = oracle_eval_quad(pb, par)
    assert 1e-12 < abs(v - qv) / abs(qv) < 1e-9
    assert 1e-8 < np.max(np.abs(g - qg)) / np.max(np.abs(qg)) < 1e-4
    # a coarser / finer differencing step moves nothing: the binary128 gradient is not a step-size artefact
    _, qg2 = oracle_eval_quad(pb, par, fd_step=1e-8)
    assert np.max(np.abs(qg - qg2)) <= 1e-12 * np.max(np.abs(qg))
