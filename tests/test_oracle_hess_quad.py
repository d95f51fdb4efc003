"""CPU suite: oracle_hess_quad (oracle/oracle_quad.cpp) -- second central differences of the binary128 restatement, the outside
reference of tests/test_gpu_hess_windows.py at lengths where an autograd Hessian of the dense restatement is out of reach.

Pinned here: on every golden record that tests/test_gpu_laplace.py compares with autograd, over the same index list, it agrees with
torch.autograd.functional.hessian of the dense restatement.  Measured (oracle/README.md): worst gap 6.1e-14 of max|H| (OU_SSM_d1_drift,
308 rows: autograd in double is the limiting side), 2.7e-14 on CTCRW_d2_tv_H_P0, 1e-16 .. 9e-15 elsewhere.  BOUND = 10 x that worst
gap, inside the 1e-12 the issue allows at most."""
import numpy as np
import pytest
import torch

from cases import problem_from_spec
from golden_io import load_golden
from oracle_lib import oracle_eval_quad, oracle_hess_quad
from refimpl import direct_nllk, eseal_dense_nllk, eseal_priors, kalman_dense_nllk, penalty

GOLD = {r["name"]: r for r in load_golden()}
BOUND = 6.1e-13

DIRECT = ["OU_d1_tv", "OU_d2_tv", "BM_d1_tv", "BM_d2_tv", "OU_d1_tv2", "OU_d1_const", "BM_d2_const", "BM_t_d1_tv", "BM_t_d1_const",
          "OU_d1_decay", "BM_d2_decay2", "CIR_d1_const", "CIR_d2_tv"]
ROW_VARYING = ["CTCRW_d1_tv", "CTCRW_d2_tv", "OU_SSM_d1_tv", "OU_SSM_d2_tv", "BM_SSM_d1_tv", "BM_SSM_d2_tv", "CTCRW_d2_tv2_RNA"]
CONST_KALMAN = ["CTCRW_d2_const", "CTCRW_d1_const_regular_fixmu", "OU_SSM_d2_const", "OU_SSM_d1_const", "BM_SSM_d1_const", "BM_SSM_d2_const"]
DENSE_TV = [n for n in GOLD if GOLD[n]["model"] in ("CTCRW", "OU_SSM", "BM_SSM") and GOLD[n]["n_dim"] <= 2
            and (GOLD[n].get("H") is not None or GOLD[n].get("P0") is not None)]
ESEAL = ["ESEAL_const", "ESEAL_tv"]
CASES = [(n, "all") for n in DIRECT] + [(n, "free") for n in ROW_VARYING + CONST_KALMAN + ESEAL if n in GOLD] + \
        [(n, "dense") for n in DENSE_TV] + [("OU_SSM_d1_drift", "mu")]


def _index_list(pb, kind):
    """the index lists of tests/test_gpu_laplace.py"""
    if kind == "all":
        return list(range(pb.n_par_full))
    if kind == "dense":
        return [k for k in range(pb.n_par_full) if not pb.par_fixed[k] and not (pb.H is not None and k == 0)]
    if kind == "mu":
        idx = []
        for j in range(pb.n_dim):
            idx += [pb.off_fe + pb.fe_off[j] + c for c in range(pb.ncol_fe[j])]
            idx += [pb.off_re + pb.re_off[j] + c for c in range(pb.ncol_re[j])]
        return sorted(idx) + [pb.off_lambda + s for s in range(pb.n_smooth)]
    return [k for k in range(pb.n_par_full) if not pb.par_fixed[k]]


def _autograd_hessian(pb, par, idx):
    p0 = torch.tensor(par)

    def f(x):
        p = p0.clone()
        p[idx] = x
        if pb.model == "ESEAL_SSM":
            return eseal_dense_nllk(pb, p) + penalty(pb, p) + eseal_priors(pb, p)
        return (kalman_dense_nllk(pb, p) if pb.kalman else direct_nllk(pb, p)) + penalty(pb, p)

    return torch.autograd.functional.hessian(f, torch.tensor(par[idx])).numpy()


@pytest.mark.parametrize("name, kind", CASES, ids=[n for n, _ in CASES])
def test_binary128_hessian_matches_autograd_of_the_dense_restatement(name, kind):
    rec = GOLD[name]
    pb = problem_from_spec(rec)
    par = rec["par"].copy()
    idx = _index_list(pb, kind)
    H = oracle_hess_quad(pb, par, idx)
    Ha = _autograd_hessian(pb, par, idx)
    gap = np.max(np.abs(H - Ha)) / np.max(np.abs(Ha))
    print("%s: binary128 against autograd %.2e of max|H|" % (name, gap))
    assert np.array_equal(H, H.T)                                   # bitwise: both triangles are one number
    assert gap <= BOUND, gap


@pytest.fixture(scope="module")
def long_track():
    """one 640-row CTCRW d = 2 track with smooth tau and nu and missing rows: 15 directions + 2 log_lambda"""
    from hess_cases import free_entries, ragged_problem
    pb, par = ragged_problem("CTCRW", 2, lengths=[640])
    idx = free_entries(pb)
    return pb, par, idx, oracle_hess_quad(pb, par, idx)


def test_the_step_does_not_matter_on_a_640_row_track(long_track):
    pb, par, idx, H = long_track
    assert pb.n == 640 and len(idx) == 17
    H7 = oracle_hess_quad(pb, par, idx, fd_step=1e-7)
    gap = np.max(np.abs(H - H7)) / np.max(np.abs(H))
    print("step 1e-8 against 1e-7: %.2e of max|H|" % gap)
    assert gap <= BOUND, gap
    assert np.array_equal(H, H.T) and np.array_equal(H7, H7.T)


def test_threads_and_index_order_change_nothing(long_track):
    pb, par, idx, H = long_track
    sub = idx[::-3]
    Hs = oracle_hess_quad(pb, par, sub, threads=1)
    pos = [idx.index(k) for k in sub]
    assert np.array_equal(Hs, H[np.ix_(pos, pos)])                  # every entry is its own difference: bitwise


def test_the_diagonal_is_the_second_difference_of_the_binary128_value(long_track):
    """an independent look at one entry: the three-point form from values rounded to double loses digits (1e-16 / h^2 relative to
    f / h^2), so with h = 1e-3 it pins the entry to ~1e-7 -- enough to catch a wrong index, sign or factor"""
    pb, par, idx, H = long_track
    for a in (0, 5, len(idx) - 1):
        h = 1e-3
        pp, pm = par.copy(), par.copy()
        pp[idx[a]] += h
        pm[idx[a]] -= h
        f0, fp, fm = (oracle_eval_quad(pb, p, order=0) for p in (par, pp, pm))
        fd = (fp - 2 * f0 + fm) / h ** 2
        assert abs(fd - H[a, a]) <= 1e-5 * np.max(np.abs(H)), (a, fd, H[a, a])


def test_a_fixed_entry_is_differentiated_like_any_other():
    """the reference does not consult par_fixed: CTCRW_d1_const_regular_fixmu holds mu fixed, its row and column are there all the
    same and equal those of the same problem with nothing fixed"""
    rec = GOLD["CTCRW_d1_const_regular_fixmu"]
    pb = problem_from_spec(rec)
    par = rec["par"].copy()
    fixed = [k for k in range(pb.n_par_full) if pb.par_fixed[k]]
    assert fixed
    idx = list(range(pb.n_par_full))
    H = oracle_hess_quad(pb, par, idx)
    assert np.all(np.abs(H[fixed][:, fixed].diagonal()) > 0.0)
    Ha = _autograd_hessian(pb, par, idx)
    assert np.max(np.abs(H - Ha)) <= BOUND * np.max(np.abs(Ha))
    # (the gradient of the same library leaves a fixed entry at zero: the Hessian deliberately does not)
    assert np.all(oracle_eval_quad(pb, par)[1][fixed] == 0.0)


def test_the_call_counts_as_an_oracle_evaluation_and_honours_the_arbiter_mode():
    import oracle_lib
    from hess_cases import free_entries, ragged_problem
    pb, par = ragged_problem("CTCRW", 2, lengths=[60], full="H", missing=False)
    idx = free_entries(pb)
    n0 = oracle_lib.CALLS[0]
    H = oracle_hess_quad(pb, par, idx)
    assert oracle_lib.CALLS[0] == n0 + 1
    oracle_lib.keep_P_symmetric(True)
    try:
        Hs = oracle_hess_quad(pb, par, idx)
    finally:
        oracle_lib.keep_P_symmetric(False)
    # in binary128 the antisymmetric part that P <- (P + P') / 2 removes is rounding at 1e-34: the two modes agree far inside
    # double precision, but not bitwise in binary128 -- the switch reaches the library
    assert np.max(np.abs(Hs - H)) <= 1e-15 * np.max(np.abs(H))
    assert np.array_equal(oracle_hess_quad(pb, par, idx), H)
