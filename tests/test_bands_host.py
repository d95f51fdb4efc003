"""CPU suite: the numpy definition of ssde_par_bands (tests/bands_ref.py) against a plain triple loop written here
with sorted() and the quantile formula, against np.quantile, against a case worked by hand, and on the patterns the definition
names: ties, a parameter without spread, a NaN design row, a row with se = 0."""
import math
import statistics

import numpy as np
import pytest

from bands_ref import bands_ref, quantile7, tail_sizes

Z95 = statistics.NormalDist().inv_cdf(0.975)


def _q7(xs, p):
    m = len(xs)
    h = (m - 1) * p
    lo = int(math.floor(h))
    hi = min(lo + 1, m - 1)
    return xs[lo] if xs[hi] == xs[lo] else xs[lo] + (h - lo) * (xs[hi] - xs[lo])      # (equal ends: no inf - inf)


def _loop(X_fe, X_re, link, coeff, level, z, resp):
    """the definition, one number at a time"""
    q = len(X_fe)
    n = max(b.shape[0] for b in list(X_fe) + list(X_re) if b is not None)
    n_post = coeff.shape[0] - 1
    alpha = (1.0 - level) / 2.0
    out = {k: np.full((n, q), np.nan) for k in ("est", "pw_low", "pw_upp", "se", "sim_low", "sim_upp")}
    out["crit"], out["max_dev"] = np.zeros(q), np.zeros((q, n_post))
    off = 0
    for j in range(q):
        kf = 1 if X_fe[j] is None else X_fe[j].shape[1]
        kr = 0 if X_re[j] is None else X_re[j].shape[1]
        g = math.exp if (resp and link[j] == 1) else (lambda v: v)

        def x(i, c):
            return (1.0 if X_fe[j] is None else X_fe[j][i, c]) if c < kf else X_re[j][i, c - kf]
        lp = [[sum(x(i, c) * coeff[k, off + c] for c in range(kf + kr)) for k in range(1 + n_post)] for i in range(n)]
        dev = [[sum(x(i, c) * (coeff[k, off + c] - coeff[0, off + c]) for c in range(kf + kr)) for k in range(1, 1 + n_post)] for i in range(n)]
        se = [None] * n
        for i in range(n):
            if not all(math.isfinite(v) for v in lp[i]):
                continue
            srt = sorted(lp[i][1:])
            se[i] = (lp[i][0] - _q7(srt, alpha)) / z
            out["est"][i, j] = g(lp[i][0])
            out["pw_low"][i, j] = _q7([g(v) for v in srt], alpha)
            out["pw_upp"][i, j] = _q7([g(v) for v in srt], 1.0 - alpha)
            out["se"][i, j] = se[i]
        for k in range(n_post):
            mx = 0.0
            for i in range(n):
                if se[i] is None:
                    continue
                if se[i] == 0.0:
                    a = 0.0 if dev[i][k] == 0.0 else math.inf
                else:
                    a = abs(dev[i][k] / se[i])
                mx = max(mx, a)
            out["max_dev"][j, k] = mx
        srt = sorted(out["max_dev"][j])
        crit = _q7(srt, level)
        crit = 0.0 if math.isnan(crit) else crit
        out["crit"][j] = crit
        for i in range(n):
            if se[i] is not None:
                out["sim_low"][i, j] = g(lp[i][0] - crit * se[i])
                out["sim_upp"][i, j] = g(lp[i][0] + crit * se[i])
        off += kf + kr
    return out


def _case(n_post, seed=0, n=5):
    rng = np.random.default_rng(seed)
    X_fe = [None, np.column_stack([np.ones(n), rng.uniform(-1, 1, (n, 2))]), np.column_stack([np.ones(n), rng.uniform(-1, 1, (n, 3))])]
    X_re = [None, None, rng.uniform(0, 1, (n, 5))]
    link = np.array([1, 0, 1], dtype=np.uint8)
    chat = rng.uniform(-1, 1, 1 + 3 + 9)
    coeff = np.vstack([chat, chat + 0.3 * rng.standard_normal((n_post, len(chat)))])
    return X_fe, X_re, link, coeff


def _close(a, b, lim_rel, tag):
    for k in a:
        assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), (tag, k)
        big = np.nanmax(np.abs(b[k])) if np.isfinite(np.nanmax(np.abs(b[k]))) else 1.0
        with np.errstate(invalid="ignore"):
            gap = np.abs(a[k] - b[k])
        gap[a[k] == b[k]] = 0.0
        assert np.nanmax(gap) <= lim_rel * (1.0 + big), (tag, k, np.nanmax(gap))


@pytest.mark.parametrize("resp", [True, False])
@pytest.mark.parametrize("n_post", [2, 7, 40])
def test_definition_against_a_plain_loop(n_post, resp):
    args = _case(n_post, seed=n_post)
    _close(bands_ref(*args, 0.95, Z95, resp=resp), _loop(*args, 0.95, Z95, resp), 1e-13, f"n_post={n_post}")


@pytest.mark.parametrize("n_post", [2, 7, 40, 1000, 2500])
def test_quantile_against_numpy(n_post):
    rng = np.random.default_rng(n_post)
    x = np.sort(rng.standard_normal((6, n_post)), axis=1)
    for p in (0.025, 0.975, 0.95, 0.25, (1 - 0.95) / 2, 1 - (1 - 0.95) / 2):
        ref = np.quantile(x, p, axis=1)
        assert np.max(np.abs(quantile7(x, p) - ref)) <= 1e-14 * (1.0 + np.max(np.abs(ref)))
    args = _case(n_post, seed=3) if n_post <= 40 else None
    if args:
        X_fe, X_re, link, coeff = args
        got = bands_ref(X_fe, X_re, link, coeff, 0.95, Z95, resp=False)
        lp = np.column_stack([np.ones(5), X_fe[1][:, 1:]]) @ coeff[1:, 1:4].T
        for name, p in (("pw_low", 0.025), ("pw_upp", 0.975)):
            ref = np.quantile(lp, (1 - 0.95) / 2 if name == "pw_low" else 1 - (1 - 0.95) / 2, axis=1)
            assert np.max(np.abs(got[name][:, 1] - ref)) <= 1e-14 * (1.0 + np.max(np.abs(ref)))


def test_a_case_worked_by_hand():
    # one parameter, one column of ones, the draws 1 .. 5 (in another order), the estimate 3: Q(0.025) = 1.1, Q(0.975) = 4.9
    coeff = np.array([[3.0], [4.0], [1.0], [5.0], [2.0], [3.0]])
    out = bands_ref([None], [None], np.array([0], dtype=np.uint8), coeff, 0.95, Z95, resp=True)
    assert out["est"][0, 0] == 3.0
    assert abs(out["pw_low"][0, 0] - 1.1) <= 1e-15 and abs(out["pw_upp"][0, 0] - 4.9) <= 2e-15
    assert abs(out["se"][0, 0] - 1.9 / Z95) <= 1e-15
    # deviations -2 .. 2 over se: the maxima are |dev| / se, their 0.95 quantile is (1 + 0.8) / se ... of 0, 1, 1, 2, 2
    assert np.allclose(np.sort(out["max_dev"][0]) * out["se"][0, 0], [0, 1, 1, 2, 2], rtol=0, atol=1e-14)
    assert abs(out["crit"][0] - 2.0 / out["se"][0, 0]) <= 1e-13
    assert abs(out["sim_low"][0, 0] - 1.0) <= 1e-13 and abs(out["sim_upp"][0, 0] - 5.0) <= 1e-13
    assert tail_sizes(2500, 0.95) == (64, 64) and tail_sizes(1000, 0.90) == (51, 51) and tail_sizes(1000, 0.5)[0] == 251


def test_ties_count_with_their_multiplicity():
    X_fe, X_re, link, coeff = _case(20, seed=9)
    coeff = np.vstack([coeff[:1], np.repeat(coeff[1:], 2, axis=0)])          # every draw twice: n_post = 40
    _close(bands_ref(X_fe, X_re, link, coeff, 0.95, Z95), _loop(X_fe, X_re, link, coeff, 0.95, Z95, True), 1e-13, "ties")


def test_a_parameter_without_spread_collapses():
    X_fe, X_re, link, coeff = _case(40, seed=11)
    coeff[1:, 1:4] = coeff[0, 1:4]                                            # parameter 1: the same coefficients in every draw
    out = bands_ref(X_fe, X_re, link, coeff, 0.95, Z95)
    assert np.all(out["se"][:, 1] == 0.0) and out["crit"][1] == 0.0 and np.all(out["max_dev"][1] == 0.0)
    for k in ("pw_low", "pw_upp", "sim_low", "sim_upp"):
        assert np.array_equal(out[k][:, 1], out["est"][:, 1]), k
    assert np.all(out["se"][:, 2] != 0.0) and out["crit"][2] > 0.0


def test_a_nan_design_row_is_nan_alone():
    X_fe, X_re, link, coeff = _case(40, seed=13)
    clean = bands_ref(X_fe, X_re, link, coeff, 0.95, Z95)
    X_fe[2] = X_fe[2].copy()
    X_fe[2][3, 1] = np.nan
    out = bands_ref(X_fe, X_re, link, coeff, 0.95, Z95)
    rest = [i for i in range(5) if i != 3]
    for k in ("est", "pw_low", "pw_upp", "se", "sim_low", "sim_upp"):
        assert np.isnan(out[k][3, 2]) and not np.isnan(out[k][:, :2]).any() and not np.isnan(out[k][rest, 2]).any(), k
        assert np.array_equal(out[k][:, :2], clean[k][:, :2])
    # the row adds nothing to max_dev: what is left is the maximum over the other rows, and crit is unchanged where the NaN row
    # was not the one that set it -- compared with the definition on the other rows alone
    sub = bands_ref([None, X_fe[1][rest], X_fe[2][rest]], [None, None, X_re[2][rest]], link, coeff, 0.95, Z95)
    # (a matrix product of other rows may round its sums in another order: 1e-13, not bitwise)
    assert np.allclose(out["max_dev"][2], sub["max_dev"][2], rtol=1e-13, atol=1e-13) and abs(out["crit"][2] - sub["crit"][2]) <= 1e-13
    assert np.allclose(out["sim_low"][rest, 2], sub["sim_low"][:, 2], rtol=1e-12, atol=1e-12)
    assert np.array_equal(out["crit"][:2], clean["crit"][:2]) and np.array_equal(out["max_dev"][:2], clean["max_dev"][:2])


def test_a_row_with_se_zero_and_a_deviation_is_inf():
    # two rows, one column: row 0's design value is 0 -> lp = 0 in every draw, se = 0, dev = 0: counts as 0.  Add a second column that is
    # zero in the draws' low quantile only ... simpler: se = 0 because the estimate EQUALS the low quantile while the draws differ
    coeff = np.array([[1.1], [4.0], [1.0], [5.0], [2.0], [3.0]])
    coeff[0, 0] = bands_ref([None], [None], [0], coeff, 0.95, Z95)["pw_low"][0, 0]
    out = bands_ref([None], [None], np.array([0], dtype=np.uint8), coeff, 0.95, Z95)
    assert out["se"][0, 0] == 0.0 and np.all(np.isinf(out["max_dev"][0])) and np.isinf(out["crit"][0])
    same = _loop([np.ones((1, 1))], [None], [0], coeff, 0.95, Z95, True)
    assert np.all(np.isinf(same["max_dev"][0]))
