"""GPU suite: ssde_par_bands (csrc/k_par_bands.hip; include/ssde.h) against its numpy definition
(tests/bands_ref.py) on the cases of tests/bands_cases.py, its bitwise invariances, its argument checks, and SDE.CI_pointwise /
SDE.CI_simultaneous on a small fit.

Limits (bands_cases.compare).  est, pw_*, max_dev: two fma chains of K terms differ by at most 2 K u S_i, u = 2^-53, S_i = max_k
sum_c |X[i, c] coeff[k, c]|; the interpolation adds a few u: 4 (K + 4) u S_i per row, relative on the response scale; the cases keep
1 <= S_i <= 100.  crit, sim_*: they divide by se; with g the gap between the definition in float64 and in long double the inputs must
give g <= 1e-11 (1 + max|ref|) and the limit is max(1e-12, 64 g) (1 + max|ref|).  NaN patterns identical.  Every comparison prints
its largest gap over its limit."""
import ctypes as C

import numpy as np
import pytest

from bands_cases import CASES, case, compare, make_case, ref_args
from bands_ref import bands_ref, tail_sizes
from smoothsde_amd import capi

pytestmark = pytest.mark.gpu

ROW_OUT = ("est", "pw_low", "pw_upp", "sim_low", "sim_upp")


def _gpu(c, **kw):
    return capi.par_bands(c["X_fe"], c["X_re"], c["link"], c["coeff"], level=c["level"], resp=c["resp"], z=c["z"], **kw)


def _check(c, tag, **kw):
    ref = bands_ref(*ref_args(c), resp=c["resp"])
    ref_ld = bands_ref(*ref_args(c), resp=c["resp"], dtype=np.longdouble)
    got = _gpu(c, **kw)
    compare(got, ref, ref_ld, c, tag)
    return got, ref


def _same(a, b, names=None):
    for k in (names or a.keys()):
        x, y = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (a[k], b[k]))
        assert np.array_equal(x, y, equal_nan=True), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_definition(name):
    _check(case(name), name)


def test_the_cap_a_tail_of_exactly_64():
    assert tail_sizes(2500, 0.95) == (64, 64)
    _check(make_case(3, 2500, [(2, 1), (0, 0)], [1, 0], seed=64), "tail 64")


def test_many_rows_and_a_thousand_draws():
    _check(make_case(4099, 1000, [(4, 6)], [1], seed=4099), "4099 x 1000 x 10")


def test_ties_collapse_and_nan_rows():
    c = make_case(70, 40, [(2, 2), (3, 0), (0, 0)], [1, 0, 1], seed=5)
    c["coeff"] = np.vstack([c["coeff"][:1], np.repeat(c["coeff"][1:21], 2, axis=0)])       # every draw twice
    c["coeff"][1:, 4:7] = c["coeff"][0, 4:7]                                                # parameter 1 has no spread
    c["X_fe"][0][66, 1] = np.nan
    got, _ = _check(c, "ties / collapse / NaN")
    assert got["crit"][1] == 0.0 and np.all(got["max_dev"][1] == 0.0)
    for k in ("pw_low", "pw_upp", "sim_low", "sim_upp"):
        assert np.array_equal(got[k][:, 1], got["est"][:, 1]), k
    for k in ROW_OUT:
        assert np.isnan(got[k][66, 0]) and np.isnan(got[k]).sum() == 1, k


@pytest.mark.parametrize("row", [0, 100, 191, 199])
def test_the_row_of_the_maximum_in_every_kind_of_row_block(row):
    """200 rows are four row blocks of pass 2 (64, 64, 64, 8).  Two columns; the draws spread in the second alone, and every row but
    one has a zero there: its linear predictor is the same in every draw, se = 0, dev = 0, and it adds 0.  The one row that does vary
    is planted in the first row, a middle block, the last full block and the last partial block."""
    n, n_post = 200, 70
    rng = np.random.default_rng(3)
    X = np.column_stack([np.ones(n), np.zeros(n)])
    X[row, 1] = 1.0
    coeff = np.column_stack([np.full(1 + n_post, 1.5), 0.4 + 0.3 * np.r_[0.0, rng.standard_normal(n_post)]])
    c = dict(X_fe=[X], X_re=[None], link=np.array([1], dtype=np.uint8), coeff=coeff, level=0.95, resp=True, z=1.959963984540054, n=n, n_post=n_post)
    got, ref = _check(c, f"planted row {row}")
    alone = _gpu(dict(c, X_fe=[X[row:row + 1]], n=1))
    assert np.array_equal(got["max_dev"], alone["max_dev"]) and np.all(got["max_dev"][0, :] >= 0.0) and got["max_dev"].max() > 1.0
    assert got["crit"][0] == alone["crit"][0] > 0.0
    others = np.arange(n) != row
    for k in ("pw_low", "pw_upp", "sim_low", "sim_upp"):
        assert np.array_equal(got[k][others, 0], got["est"][others, 0]), k


@pytest.fixture(scope="module")
def wide():
    """15 000 rows, two parameters of 2 and 9 + 10 columns, 64 draws, and one call's outputs"""
    c = make_case(15000, 64, [(2, 0), (9, 10)], [1, 0], seed=15)
    return c, _gpu(c)


def _rows(c, lo, hi):
    return dict(c, X_fe=[None if b is None else b[lo:hi] for b in c["X_fe"]], X_re=[None if b is None else b[lo:hi] for b in c["X_re"]], n=hi - lo)


def test_bitwise_two_identical_calls_and_the_definition(wide):
    c, whole = wide
    _same(whole, _gpu(c))
    ref = bands_ref(*ref_args(c), resp=c["resp"])
    compare(whole, ref, bands_ref(*ref_args(c), resp=c["resp"], dtype=np.longdouble), c, "15000 rows")


def test_bitwise_the_halves(wide):
    c, whole = wide
    a, b = _gpu(_rows(c, 0, 7001)), _gpu(_rows(c, 7001, 15000))
    for k in ("est", "pw_low", "pw_upp"):
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]]), equal_nan=True), k
    assert np.array_equal(whole["max_dev"], np.maximum(a["max_dev"], b["max_dev"]))


def test_bitwise_three_or_more_chunks(wide):
    c, whole = wide
    row_bytes = 8 * (2 + 19) + 8 * 2 * 3                     # the staged blocks and the three staged outputs of one row
    assert 15000 * row_bytes > 3 * (1 << 20)                 # budget_mb = 1: four chunks
    _same(whole, _gpu(c, budget_mb=1))


def test_bitwise_device_data_and_device_out(wide):
    import torch
    c, whole = wide
    dev = torch.device("cuda", 0)
    Xf = [None if b is None else torch.as_tensor(b, device=dev) for b in c["X_fe"]]
    Xr = [None if b is None else torch.as_tensor(b, device=dev) for b in c["X_re"]]
    kw = dict(level=c["level"], resp=c["resp"], z=c["z"])
    _same(whole, capi.par_bands(Xf, Xr, c["link"], c["coeff"], **kw))
    out = capi.par_bands(Xf, Xr, c["link"], c["coeff"], device_out=True, **kw)
    assert all(out[k].is_cuda for k in ROW_OUT)
    _same(whole, out)
    _same(whole, _gpu(c, device_out=True, budget_mb=1))       # host blocks in chunks, outputs straight into HBM


def test_bitwise_pointwise_alone(wide):
    c, whole = wide
    pw = _gpu(c, simultaneous=False)
    assert sorted(pw) == ["est", "pw_low", "pw_upp"]
    _same(pw, whole, names=pw.keys())
    _same(_gpu(c, want=("pw_upp",)), whole, names=("pw_upp",))
    _same(_gpu(c, want=("crit",)), whole, names=("crit",))
    _same(_gpu(c, want=("sim_low", "max_dev")), whole, names=("sim_low", "max_dev"))


# ---- the argument checks: each one SSDE_ERR_ARG, with a text, before anything touches the device --------------------------------
def _raw(**over):
    """a valid descriptor of 4 rows, two parameters (the intercept alone; 2 + 1 columns), 20 draws -- and what `over` changes"""
    lib = capi.load_library()
    keep = {}
    keep["xf1"] = np.asfortranarray(np.column_stack([np.ones(4), np.linspace(-1, 1, 4)]))
    keep["xr1"] = np.asfortranarray(np.linspace(0, 1, 4)[:, None])
    n_post = over.pop("n_post", 20)
    keep["coeff"] = over.pop("coeff", 1.0 + 0.1 * np.random.default_rng(0).standard_normal((1 + n_post, 4)))
    keep["kf"] = np.array(over.pop("ncol_fe", [1, 2]), dtype=np.int32)
    keep["kr"] = np.array(over.pop("ncol_re", [0, 1]), dtype=np.int32)
    keep["link"] = np.array(over.pop("link", [0, 1]), dtype=np.uint8)
    q = over.pop("n_par", 2)
    xf = (C.c_void_p * 16)(*over.pop("x_fe", [None, keep["xf1"].ctypes.data]))
    xr = (C.c_void_p * 16)(*over.pop("x_re", [None, keep["xr1"].ctypes.data]))
    d = capi.SsdeBandsDesc()
    d.abi_version, d.n_par, d.n = over.pop("abi_version", capi.ABI_VERSION), q, over.pop("n", 4)
    d.ncol_fe, d.x_fe = keep["kf"].ctypes.data_as(C.POINTER(C.c_int32)), xf
    d.ncol_re, d.x_re = keep["kr"].ctypes.data_as(C.POINTER(C.c_int32)), xr
    d.link, d.coeff = keep["link"].ctypes.data_as(C.POINTER(C.c_uint8)), keep["coeff"].ctypes.data_as(C.POINTER(C.c_double))
    d.n_post, d.resp, d.level, d.z = n_post, 1, over.pop("level", 0.95), over.pop("z", 1.959963984540054)
    d.device, d.budget_mb, d.flags = -1, 0, over.pop("flags", 0)
    outs = over.pop("outs", None)
    null_desc = over.pop("null_desc", False)
    assert not over, over
    bufs = [np.zeros((2, 4)) for _ in range(5)] + [np.zeros(2), np.zeros((2, n_post))]
    ptrs = [b.ctypes.data for b in bufs] if outs is None else outs
    st = lib.ssde_par_bands(None if null_desc else C.byref(d), *ptrs)
    msg = lib.ssde_last_error(None)
    return st, (msg.decode() if msg else ""), bufs


BAD = {
    "a NULL descriptor": dict(null_desc=True),
    "every output NULL": dict(outs=[None] * 7),
    "another ABI version": dict(abi_version=capi.ABI_VERSION + 1),
    "n < 1": dict(n=0),
    "n_par = 0": dict(n_par=0),
    "n_par = 17": dict(n_par=17),
    "K = 0": dict(ncol_fe=[0, 2]),
    "K = 65": dict(ncol_fe=[1, 64], ncol_re=[0, 1]),
    "a NULL fixed-effect block of two columns": dict(x_fe=[None, None]),
    "a NULL random-effect block of one column": dict(x_re=[None, None]),
    "link = 2": dict(link=[0, 2]),
    "n_post = 1": dict(n_post=1),
    "level = 0": dict(level=0.0),
    "level = 1": dict(level=1.0),
    "level NaN": dict(level=float("nan")),
    "z = 0": dict(z=0.0),
    "z NaN": dict(z=float("nan")),
    "z inf": dict(z=float("inf")),
    "a tail of 65": dict(n_post=2540),
    "a tail of 251": dict(n_post=1000, level=0.5),
    "an unknown flag": dict(flags=4),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_argument_checks(what):
    st, msg, bufs = _raw(**BAD[what])
    assert st == 1 and msg.startswith("ssde_par_bands: "), (what, st, msg)
    assert all(not b.any() for b in bufs)                                          # nothing was written


def test_argument_checks_coeff_and_a_valid_call():
    for bad in (np.nan, np.inf):
        coeff = 1.0 + 0.1 * np.random.default_rng(0).standard_normal((21, 4))
        coeff[20, 3] = bad
        st, msg, _ = _raw(coeff=coeff)
        assert st == 1 and "finite" in msg
    st, msg, bufs = _raw()
    assert st == 0 and all(np.isfinite(b).all() for b in bufs) and bufs[5].min() > 0.0
    assert tail_sizes(2540, 0.95)[0] == 65 and tail_sizes(2500, 0.95) == (64, 64)
    st, _, _ = _raw(n_post=2500)                                                    # the cap itself goes through
    assert st == 0


# ---- SDE.CI_pointwise / SDE.CI_simultaneous ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    from smoothsde_amd.sde import SDE
    from smoothsde_amd.synth import simulate
    ID, times, obs = simulate("CTCRW", 24, 120, 2, tau=2.0, nu=4.0, sigma_obs=0.1, seed=8)   # (|log nu| > 1: S_i of the intercept-only nu)
    n = len(ID)
    data = dict(ID=ID, time=times, z0=obs[:, 0], z1=obs[:, 1], x=(np.sin(np.arange(n) * 0.013) + 1) / 2)
    sde = SDE(formulas={"mu1": "~1", "mu2": "~1", "tau": "~x", "nu": "~1"}, data=data, type="CTCRW", response=["z0", "z1"],
              par0=[0, 0, 1, 3], fixpar=["mu1", "mu2"])
    sde.fit(maxiter=60)
    return sde


def _sde_ref(sde, rows, level, n_post, seed, resp=True, term=None):
    import statistics
    tab = sde._band_table(n_post, seed=seed, term=term)
    X_fe, X_re = sde._band_blocks(rows)
    z = statistics.NormalDist().inv_cdf((1 + level) / 2)
    c = dict(X_fe=X_fe, X_re=X_re, link=sde._links(), coeff=tab, level=level, resp=resp, z=z, n=X_fe[2].shape[0], n_post=n_post)
    return c, bands_ref(*ref_args(c), resp=resp), bands_ref(*ref_args(c), resp=resp, dtype=np.longdouble)


def test_sde_bands_against_the_definition(fitted):
    sde = fitted
    for resp in (True, False):
        c, ref, ref_ld = _sde_ref(sde, "all", 0.95, 200, seed=3, resp=resp)
        pw = sde.CI_pointwise(t="all", n_post=200, seed=3, resp=resp)
        sim = sde.CI_simultaneous(t="all", n_post=200, seed=3, resp=resp)
        assert pw["names"] == ["mu1", "mu2", "tau", "nu"] and pw["low"].shape == (sde.n_, 4)
        compare(dict(pw_low=pw["low"], pw_upp=pw["upp"], sim_low=sim["low"], sim_upp=sim["upp"]), ref, ref_ld, c, f"SDE resp={resp}")
    # tau and nu have a width, and the simultaneous band is the wider one on the rows as a whole
    assert np.all(pw["low"][:, 2:] < pw["upp"][:, 2:]) and np.all(sim["low"][:, 2] <= pw["low"][:, 2] + 1e-12)
    # the default is row 0; rows are picked by index
    one = sde.CI_pointwise(n_post=200, seed=3, resp=False)
    some = sde.CI_pointwise(t=[5, 0, 77], n_post=200, seed=3, resp=False)
    assert one["low"].shape == (1, 4) and np.array_equal(one["low"][0], pw["low"][0]) and np.array_equal(some["upp"], pw["upp"][[5, 0, 77]])
    # post_par is the matrix behind them
    pp = sde.post_par(n_post=200, resp=False, seed=3)
    assert pp.shape == (sde.n_, 4, 200)
    assert np.max(np.abs(np.quantile(pp, 0.025, axis=2) - pw["low"])) <= 1e-12 * (1 + np.max(np.abs(pw["low"])))


def test_sde_fixed_parameters_collapse(fitted):
    sde = fitted
    est = sde.par()
    tab = sde._band_table(50, seed=1)
    assert np.all(tab[:, :2] == tab[0, :2]) and np.ptp(tab[1:, 2]) > 0
    out = capi.par_bands(*sde._band_blocks("all"), sde._links(), tab)
    assert np.all(out["crit"][:2] == 0.0) and np.all(out["crit"][2:] > 0.0)
    for k in ("pw_low", "pw_upp", "sim_low", "sim_upp"):
        assert np.array_equal(out[k][:, :2], out["est"][:, :2]), k
    assert np.allclose(out["est"][:, 2], est["tau"], rtol=1e-13, atol=0)


def test_sde_term(fitted):
    sde = fitted
    c, ref, ref_ld = _sde_ref(sde, "all", 0.95, 100, seed=2, resp=False, term="x")
    assert np.all(c["coeff"][:, [0, 1, 2, 4]] == 0.0) and np.all(c["coeff"][:, 3] != 0.0)        # only tau's slope is left
    sim = sde.CI_simultaneous(t="all", n_post=100, seed=2, resp=False, term="x")
    compare(dict(sim_low=sim["low"], sim_upp=sim["upp"]), ref, ref_ld, c, "SDE term")
    assert np.all(sim["low"][:, [0, 1, 3]] == 0.0) and np.all(sim["upp"][:, [0, 1, 3]] == 0.0)
    x = np.asarray(sde.data()["x"])
    assert np.allclose(0.5 * (sim["low"][:, 2] + sim["upp"][:, 2]) , sde.coeff_fe()[3] * x, rtol=0, atol=1e-12)
