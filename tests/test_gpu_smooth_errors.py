"""GPU suite (-m gpu): what the ten calls of csrc/ssde_engine_smooth.hip refuse, and in which order.

Every refusal here comes before a kernel is launched, so the whole module is host work on two small handles: a CTCRW of two
columns (3 tracks x 4 rows) and a CTCRW of three columns run as ONE coupled filter, which the calls that need the position or
velocity columns in one lane (and the draws) turn away.  For every call: each refused argument alone, then -- for each adjacent pair
of checks of the entry point -- both wrong at once, where the EARLIER check must be the one reported.  The status and the ENTIRE text
of ssde_last_error are asserted; the texts are literals of the interface.  Everything goes through the raw ctypes functions, which
also send what the Python layer cannot (a wrong parameter length, an unknown flag)."""
import ctypes as C

import numpy as np
import pytest

from cases import make_spec, problem_from_spec
from smoothsde_amd import capi

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_MODEL = 1, 2
_dp, _lp, _ip, _up = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
BIG = (1 << 28) - 1                      # draw0 + n_draws = 2^28 with one draw


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


def _f(v):
    return None if v is None else np.ascontiguousarray(v, dtype=np.float64)


def _i(v, dt=np.int64):
    return None if v is None else np.ascontiguousarray(v, dtype=dt)


@pytest.fixture(scope="module")
def engines():
    s2 = make_spec("ge_ctcrw2", "CTCRW", 2, seed=5, lengths=[4, 4, 4])
    s3 = make_spec("ge_coupled3", "CTCRW", 3, seed=6, lengths=[4, 4, 4], with_H=True)
    e = {}
    for key, sp in (("d2", s2), ("d3", s3)):
        pb = problem_from_spec(sp)
        eng = capi.Engine(pb)
        assert eng.info()["n_devices"] == 1
        e[key] = (eng, pb, np.ascontiguousarray(sp["par"], dtype=np.float64))
    assert e["d2"][1].n == 12 and e["d2"][1].n_seg == 3
    yield e
    for eng, _, _ in e.values():
        eng.close()


# ---- the calls: every argument valid unless overridden ------------------------------------------------------------------------------
def _common(E, kw):
    eng, pb, par = E
    return eng, pb, par, kw.get("n_par", eng.n_par_full)


def call_smooth(E, **kw):
    eng, pb, par, npar = _common(E, kw)
    out = np.zeros(pb.n * 8)
    return eng.lib.ssde_smooth(eng._h, _p(par), npar, _p(out), None, None)


def call_loo(E, **kw):
    eng, pb, par, npar = _common(E, kw)
    out, stats = np.zeros(pb.n * 4), np.zeros(pb.n_seg * (4 + capi.LOO_MAX_THR + 2))
    thr = _f(kw.get("thr"))
    return eng.lib.ssde_smooth_loo(eng._h, _p(par), npar, _p(out), None, None, None, _p(thr), kw.get("n_thr", 0 if thr is None else len(thr)),
                                   _p(stats) if kw.get("stats", True) else None, kw.get("flags", 0))


def call_draws(E, **kw):
    eng, pb, par, npar = _common(E, kw)
    out = np.zeros(pb.n * 8)
    return eng.lib.ssde_smooth_draws(eng._h, _p(par), npar, 0, kw.get("draw0", 0), kw.get("n_draws", 1), C.c_void_p(out.ctypes.data),
                                     kw.get("flags", 0))


def call_path(E, **kw):
    eng, pb, par, npar = _common(E, kw)
    reg = _f(kw.get("regions"))
    out = np.zeros(pb.n_seg * (2 + capi.PATH_MAX_REGIONS + 2))
    return eng.lib.ssde_path_stats(eng._h, _p(par), npar, 0, kw.get("draw0", 0), kw.get("n_draws", 1), _p(reg),
                                   kw.get("n_regions", 0 if reg is None else len(reg) // 4), None, _p(out), kw.get("flags", 0))


def call_speed(E, **kw):
    eng, pb, par, npar = _common(E, kw)
    thr = _f(kw.get("thr"))
    out, rows = np.zeros(pb.n_seg * (5 + capi.SPEED_MAX_THR + 2)), np.zeros(pb.n * (capi.SPEED_MAX_THR + 2), dtype=np.uint32)
    return eng.lib.ssde_path_speed(eng._h, _p(par), npar, 0, kw.get("draw0", 0), kw.get("n_draws", 1), _p(thr),
                                   kw.get("n_thr", 0 if thr is None else len(thr)), None, _p(out),
                                   _p(rows, _up) if kw.get("rows", False) else None, kw.get("flags", 0))


def _occ(fine):
    def call(E, **kw):
        eng, pb, par, npar = _common(E, kw)
        g = dict(x0=0.0, dx=1.0, y0=0.0, dy=1.0, nx=4, ny=3)
        g.update(kw.get("grid", {}))
        G = capi.SsdeOccGrid(g["x0"], g["dx"], g["y0"], g["dy"], g["nx"], g["ny"])
        w, grp = _f(kw.get("weight")), _i(kw.get("group"), np.int32)
        occ, out = np.zeros(64), np.zeros(4)
        head = (eng._h, _p(par), npar, 0, kw.get("draw0", 0), kw.get("n_draws", 1), C.byref(G))
        tail = (_p(w), _p(grp, _ip), kw.get("n_groups", 1), _p(occ), _p(out), kw.get("flags", 0))
        if fine:
            return eng.lib.ssde_path_occupancy_fine(*head, kw.get("max_step", np.inf), *tail)
        return eng.lib.ssde_path_occupancy(*head, *tail)
    return call


def call_predict(E, **kw):
    eng, pb, par, npar = _common(E, kw)
    rows, offs = _i(kw.get("rows", [1, 2])), _f(kw.get("offs", [0.1, 0.2]))
    out = np.zeros(len(rows) * 8)
    return eng.lib.ssde_predict(eng._h, _p(par), npar, _p(rows, _lp), _p(offs), kw.get("nq", len(rows)), _p(out), None)


def call_predict_draws(E, **kw):
    eng, pb, par, npar = _common(E, kw)
    rows, offs = _i(kw.get("rows", [1, 2])), _f(kw.get("offs", [0.1, 0.2]))
    out = np.zeros(len(rows) * 8)
    return eng.lib.ssde_predict_draws(eng._h, _p(par), npar, _p(rows, _lp), _p(offs), kw.get("nq", len(rows)), 0, kw.get("draw0", 0),
                                      kw.get("n_draws", 1), _p(out), kw.get("flags", 0))


def call_prox(E, **kw):
    eng, pb, par, npar = _common(E, kw)
    ra, oa = _i(kw.get("rows", [1, 2])), _f(kw.get("offs", [0.1, 0.2]))
    rb, ob = _i(kw.get("rows_b", [5, 6])), _f(kw.get("offs_b", [0.1, 0.2]))
    ptr = _i(kw.get("pair_ptr", [0, 2]))
    w, rad = _f(kw.get("weight")), _f(kw.get("radii"))
    out = np.zeros(2 + capi.PROX_MAX_RADII + 2)
    return eng.lib.ssde_path_proximity(eng._h, _p(par), npar, 0, kw.get("draw0", 0), kw.get("n_draws", 1), _p(ra, _lp), _p(oa), _p(rb, _lp), _p(ob),
                                       _p(ptr, _lp), kw.get("n_pairs", len(ptr) - 1), _p(w), _p(rad),
                                       kw.get("n_radii", 0 if rad is None else len(rad)), _p(out), kw.get("flags", 0))


# ---- the checks of every entry point, IN THE ORDER THEY RUN: (handle, overrides, status, text after "<call>: " or whole text) -------
PAR_LEN = ("d2", dict(n_par=1), ERR_ARG, "=parameter vector has the wrong length")
DRAWS = "n_draws >= 1, draw0 >= 0 and draw0 + n_draws < 2^28 are required"
FLAG = "unknown flag"
Q_ROW, Q_OFF = "a query row outside [0, n)", "a query offset that is negative or not finite"
WEIGHT = "a weight that is negative or not finite"
COUPLED = ("a response of three or more columns that runs as ONE coupled filter is not served (uncoupled wide responses run as column "
           "pairs and are)")


def _width(what, which):
    return f"a response of three or more columns is not served, as column pairs or as one coupled filter (a {what} needs the {which} columns in one lane)"


def _draw_range():
    return [("d2", dict(n_draws=0), ERR_ARG, DRAWS), ("d2", dict(draw0=-1), ERR_ARG, DRAWS), ("d2", dict(draw0=BIG), ERR_ARG, DRAWS)]


def _queries():
    # (checked query by query, the row before the offset: the first wrong QUERY is reported, see test_query_order)
    return [("d2", dict(rows=[1, 12]), ERR_ARG, Q_ROW), ("d2", dict(rows=[-1, 2]), ERR_ARG, Q_ROW),
            ("d2", dict(offs=[0.1, -1e-300]), ERR_ARG, Q_OFF), ("d2", dict(offs=[np.nan, 0.2]), ERR_ARG, Q_OFF),
            ("d2", dict(offs=[0.1, np.inf]), ERR_ARG, Q_OFF)]


def _occ_checks(fine):
    w = lambda v: np.r_[np.ones(11), v]
    c = [PAR_LEN] + _draw_range() + [
        ("d2", dict(flags=2), ERR_ARG, FLAG),
        ("d2", dict(grid=dict(nx=0)), ERR_ARG, "nx and ny must be 1 ... 4096"), ("d2", dict(grid=dict(ny=4097)), ERR_ARG, "nx and ny must be 1 ... 4096"),
        ("d2", dict(n_groups=0), ERR_ARG, "n_groups >= 1 and nx * ny * n_groups <= 2^28 are required"),
        ("d2", dict(n_groups=2), ERR_ARG, "without a group table there is one group"),
        ("d3", dict(), ERR_MODEL, _width("cell", "position")),
        ("d2", dict(grid=dict(dx=0.0)), ERR_ARG, "the grid's origin must be finite and its steps finite and positive"),
        ("d2", dict(grid=dict(y0=np.nan)), ERR_ARG, "the grid's origin must be finite and its steps finite and positive"),
        ("d2", dict(group=[0, 1, 0], n_groups=1), ERR_ARG, "a group outside -1 ... n_groups - 1"),
        ("d2", dict(weight=w(-1e-300)), ERR_ARG, WEIGHT), ("d2", dict(weight=w(np.nan)), ERR_ARG, WEIGHT), ("d2", dict(weight=w(np.inf)), ERR_ARG, WEIGHT)]
    if fine:
        c += [("d2", dict(max_step=0.0), ERR_ARG, "max_step must be positive (+inf: no refinement)"),
              ("d2", dict(max_step=np.nan), ERR_ARG, "max_step must be positive (+inf: no refinement)")]
    return c


CALLS = {
    "ssde_smooth": (call_smooth, [PAR_LEN]),
    "ssde_smooth_loo": (call_loo, [
        PAR_LEN,
        ("d2", dict(n_thr=-1), ERR_ARG, "0 <= n_thr <= SSDE_LOO_MAX_THR, with a table of thresholds when there are any"),
        ("d2", dict(n_thr=1), ERR_ARG, "0 <= n_thr <= SSDE_LOO_MAX_THR, with a table of thresholds when there are any"),
        ("d2", dict(n_thr=9), ERR_ARG, "0 <= n_thr <= SSDE_LOO_MAX_THR, with a table of thresholds when there are any"),
        ("d2", dict(thr=[1.0, -1.0]), ERR_ARG, "a threshold that is not finite or negative"),
        ("d2", dict(thr=[np.inf]), ERR_ARG, "a threshold that is not finite or negative"),
        ("d2", dict(thr=[1.0], stats=False), ERR_ARG, "thresholds are counted in the statistics, which were not asked for"),
        ("d2", dict(flags=1), ERR_ARG, FLAG)]),
    "ssde_smooth_draws": (call_draws, [PAR_LEN] + _draw_range() + [("d2", dict(flags=2), ERR_ARG, FLAG), ("d3", dict(), ERR_MODEL, COUPLED)]),
    "ssde_path_stats": (call_path, [PAR_LEN] + _draw_range() + [
        ("d2", dict(n_regions=-1), ERR_ARG, "0 <= n_regions <= SSDE_PATH_MAX_REGIONS, with a table of bounds when there are regions"),
        ("d2", dict(n_regions=1), ERR_ARG, "0 <= n_regions <= SSDE_PATH_MAX_REGIONS, with a table of bounds when there are regions"),
        ("d2", dict(n_regions=9), ERR_ARG, "0 <= n_regions <= SSDE_PATH_MAX_REGIONS, with a table of bounds when there are regions"),
        ("d2", dict(regions=[0.0, 1.0, 2.0, 1.0]), ERR_ARG, "a region bound that is NaN, or lo > hi"),
        ("d2", dict(regions=[np.nan, 1.0, 0.0, 1.0]), ERR_ARG, "a region bound that is NaN, or lo > hi"),
        ("d2", dict(flags=1), ERR_ARG, FLAG),
        ("d3", dict(), ERR_MODEL, _width("distance", "position"))]),
    "ssde_path_speed": (call_speed, [PAR_LEN] + _draw_range() + [
        ("d2", dict(n_thr=-1), ERR_ARG, "0 <= n_thr <= SSDE_SPEED_MAX_THR, with a table of thresholds when there are any"),
        ("d2", dict(n_thr=1), ERR_ARG, "0 <= n_thr <= SSDE_SPEED_MAX_THR, with a table of thresholds when there are any"),
        ("d2", dict(n_thr=9), ERR_ARG, "0 <= n_thr <= SSDE_SPEED_MAX_THR, with a table of thresholds when there are any"),
        ("d2", dict(thr=[1.0, -1.0]), ERR_ARG, "a threshold that is NaN or negative"),
        ("d2", dict(thr=[np.nan]), ERR_ARG, "a threshold that is NaN or negative"),
        ("d2", dict(rows=True), ERR_ARG, "per-row counts need a threshold"),
        ("d2", dict(flags=1), ERR_ARG, FLAG),
        ("d3", dict(), ERR_MODEL, _width("speed", "velocity"))]),
    "ssde_path_occupancy": (_occ(False), _occ_checks(False)),
    "ssde_path_occupancy_fine": (_occ(True), _occ_checks(True)),
    "ssde_predict": (call_predict, [PAR_LEN, ("d2", dict(nq=0), ERR_ARG, "n_query >= 1 is required")] + _queries() + [("d3", dict(), ERR_MODEL, COUPLED)]),
    "ssde_predict_draws": (call_predict_draws, [PAR_LEN, ("d2", dict(nq=0), ERR_ARG, "n_query >= 1 is required")] + _queries() + _draw_range() + [
        ("d2", dict(flags=1), ERR_ARG, FLAG), ("d3", dict(), ERR_MODEL, COUPLED)]),
    "ssde_path_proximity": (call_prox, [
        PAR_LEN,
        ("d2", dict(n_pairs=0), ERR_ARG, "n_pairs >= 1 is required"),
        ("d2", dict(pair_ptr=[1, 2]), ERR_ARG, "pair_ptr must start at 0, not decrease, and end at n_point >= 1"),
        ("d2", dict(pair_ptr=[0, 2, 1]), ERR_ARG, "pair_ptr must start at 0, not decrease, and end at n_point >= 1"),
        ("d2", dict(pair_ptr=[0, 0]), ERR_ARG, "pair_ptr must start at 0, not decrease, and end at n_point >= 1")] + _queries() + [
        ("d2", dict(rows_b=[12, 6]), ERR_ARG, Q_ROW), ("d2", dict(offs_b=[-1.0, 0.2]), ERR_ARG, Q_OFF)] + _draw_range() + [
        ("d2", dict(n_radii=-1), ERR_ARG, "0 <= n_radii <= SSDE_PROX_MAX_RADII, with a table of radii when there are any"),
        ("d2", dict(n_radii=1), ERR_ARG, "0 <= n_radii <= SSDE_PROX_MAX_RADII, with a table of radii when there are any"),
        ("d2", dict(n_radii=9), ERR_ARG, "0 <= n_radii <= SSDE_PROX_MAX_RADII, with a table of radii when there are any"),
        ("d2", dict(radii=[1.0, -1.0]), ERR_ARG, "a radius that is NaN or negative"),
        ("d2", dict(radii=[np.nan]), ERR_ARG, "a radius that is NaN or negative"),
        ("d2", dict(weight=[1.0, -1e-300]), ERR_ARG, WEIGHT), ("d2", dict(weight=[np.nan, 1.0]), ERR_ARG, WEIGHT), ("d2", dict(weight=[1.0, np.inf]), ERR_ARG, WEIGHT),
        ("d2", dict(flags=1), ERR_ARG, FLAG),
        ("d3", dict(), ERR_MODEL, _width("distance", "position"))]),
}


def _text(name, text):
    return text[1:] if text.startswith("=") else f"{name}: {text}"


def _refused(engines, name, key, kw, status, text):
    fn = CALLS[name][0]
    E = engines[key]
    st = fn(E, **kw)
    msg = E[0].lib.ssde_last_error(E[0]._h)
    assert st == status and msg is not None and msg.decode() == _text(name, text), (name, kw, st, msg)


@pytest.mark.parametrize("name", list(CALLS))
def test_each_refusal(engines, name):
    for key, kw, status, text in CALLS[name][1]:
        _refused(engines, name, key, kw, status, text)
    # (the table's call without overrides is valid: the three-column handle's refusal, where there is one, has every check before it pass)
    assert name in ("ssde_smooth", "ssde_smooth_loo") or any(key == "d3" and not kw for key, kw, _, _ in CALLS[name][1])


def _groups(checks):
    """the table's entries grouped by the check they trip (consecutive entries with one text)"""
    out = []
    for c in checks:
        if out and out[-1][0][3] == c[3]:
            out[-1].append(c)
        else:
            out.append([c])
    return out


@pytest.mark.parametrize("name", list(CALLS))
def test_adjacent_checks_report_the_earlier(engines, name):
    """two wrong arguments at once, for each adjacent pair of checks: the last way to trip the earlier with the first way to trip the
    later (where both set one argument, the earlier's value stands: it trips the later check too, or the later is not reached).  A pair
    that needs the three-column handle runs there: both handles have 12 rows and 3 tracks, so every other argument means the same."""
    g = _groups(CALLS[name][1])
    n_pairs = 0
    for A, B in zip(g[:-1], g[1:]):
        (ka, kwa, sta, ta), (kb, kwb, _, _) = A[-1], B[0]
        if ka == "d3":
            # the width is refused before the later check: send the later's wrong argument to the three-column handle
            kw, key = dict(kwb), "d3"
        else:
            kw, key = dict(kwb, **kwa), kb
            if "grid" in kwa and "grid" in kwb:
                kw["grid"] = dict(kwb["grid"], **kwa["grid"])
        _refused(engines, name, key, kw, sta, ta)
        n_pairs += 1
    assert n_pairs == len(g) - 1


def test_query_order(engines):
    """the queries are checked one by one, the row before the offset: of two wrong queries the first is reported, whichever its fault"""
    for name in ("ssde_predict", "ssde_predict_draws", "ssde_path_proximity"):
        _refused(engines, name, "d2", dict(rows=[1, 12], offs=[-1.0, 0.2]), ERR_ARG, Q_OFF)
        _refused(engines, name, "d2", dict(rows=[12, 2], offs=[0.1, -1.0]), ERR_ARG, Q_ROW)
        _refused(engines, name, "d2", dict(rows=[12, 2], offs=[-1.0, 0.2]), ERR_ARG, Q_ROW)
    # ssde_path_proximity: side a's queries all before side b's
    _refused(engines, "ssde_path_proximity", "d2", dict(offs=[0.1, -1.0], rows_b=[12, 6]), ERR_ARG, Q_OFF)


def test_null_pointers(engines):
    eng, pb, par = engines["d2"]
    out = np.zeros(64)
    rows, offs = np.array([1, 2], dtype=np.int64), np.array([0.1, 0.2])
    G = capi.SsdeOccGrid(0.0, 1.0, 0.0, 1.0, 4, 3)
    P, O, n = _p(par), _p(out), eng.n_par_full
    lib, h = eng.lib, eng._h
    sent = [
        (lambda: lib.ssde_smooth(h, None, n, O, None, None), "ssde_smooth: no parameter vector, or no output asked for"),
        (lambda: lib.ssde_smooth(h, P, n, None, None, None), "ssde_smooth: no parameter vector, or no output asked for"),
        (lambda: lib.ssde_smooth_loo(h, P, n, None, None, None, None, None, 0, None, 0), "ssde_smooth_loo: no parameter vector, or no output asked for"),
        (lambda: lib.ssde_smooth_draws(h, P, n, 0, 0, 1, None, 0), "ssde_smooth_draws: no parameter vector, or no output"),
        (lambda: lib.ssde_path_stats(h, P, n, 0, 0, 1, None, 0, None, None, 0), "ssde_path_stats: no parameter vector, or no output"),
        (lambda: lib.ssde_path_speed(h, P, n, 0, 0, 1, None, 0, None, None, None, 0), "ssde_path_speed: no parameter vector, or no output"),
        (lambda: lib.ssde_path_occupancy(h, P, n, 0, 0, 1, None, None, None, 1, O, None, 0), "ssde_path_occupancy: no parameter vector, no grid, or no output"),
        (lambda: lib.ssde_path_occupancy_fine(h, P, n, 0, 0, 1, C.byref(G), np.inf, None, None, 1, None, None, 0),
         "ssde_path_occupancy_fine: no parameter vector, no grid, or no output"),
        (lambda: lib.ssde_predict(h, P, n, None, _p(offs), 2, O, None), "ssde_predict: no parameter vector, no queries, or no output"),
        (lambda: lib.ssde_predict_draws(h, P, n, _p(rows, _lp), None, 2, 0, 0, 1, O, 0), "ssde_predict_draws: no parameter vector, no queries, or no output"),
        (lambda: lib.ssde_path_proximity(h, P, n, 0, 0, 1, _p(rows, _lp), _p(offs), _p(rows, _lp), _p(offs), None, 1, None, None, 0, O, 0),
         "ssde_path_proximity: no parameter vector, no queries, no pair list, or no output"),
    ]
    for fn, text in sent:
        assert fn() == ERR_ARG and lib.ssde_last_error(h).decode() == text, text
    # ... and before the parameter length: both wrong, the NULL is reported
    assert lib.ssde_smooth_draws(h, P, 1, 0, 0, 1, None, 0) == ERR_ARG
    assert lib.ssde_last_error(h).decode() == "ssde_smooth_draws: no parameter vector, or no output"
