"""GPU suite (-m gpu): ssde_smooth on every handle layout, width and edge it serves, against the numpy reference
smoother of tests/smooth_ref.py (itself, and the host twin of the lane math, checked against the joint Gaussian on the CPU:
test_smooth_host.py, test_smooth_hostsim.py).  test_gpu_smooth.py holds the first dozen configurations; this file goes through what
the smoother has of its own -- the record layout, the second forward kernel, the backward kernel and its wide build, the chunk
arithmetic, the lattice map pad_row, the shard / pair scatter -- on the layouts ssde_report is compared on.

Every case asserts the layout it ran on (info(): path, const_coeff, n_rows_tiled, required_bytes_per_row, and kernel_id after one
eval where that identifies it) and goes through test_gpu_smooth._compare: mean 1e-10 (1 + max|ref|), covariance 1e-9 max|ref|,
residual 1e-9, NaN patterns identical.  Shapes: more than 64 tracks (two groups, the last partly filled), ragged lengths with a
one-row and a two-row track, an NA row ending a track; a few thousand rows at most (the reference loops over rows)."""
import ctypes as C

import numpy as np
import pytest

from cases import _tracks, make_spec, problem_from_spec
from smooth_ref import smooth_ref
from smoothsde_amd import capi
from smoothsde_amd.synth import bspline_basis, second_difference_penalty, simulate
from test_gpu_smooth import _compare, _run

pytestmark = pytest.mark.gpu

PATH_ISO, PATH_DENSE, PATH_TV = 1, 2, 3
MODELS = ["CTCRW", "OU_SSM", "BM_SSM"]
# 70 tracks: a full group and a partly filled one; a one-row track, a two-row track, and track 0 (rows 0 ... 19) for the NA rows
LENGTHS70 = [20, 35, 1, 14, 2, 27, 9] * 10


def _show(tag, info, **more):
    """the layout a case ran on (pytest -rA shows it)"""
    keys = ("path", "kernel_id", "const_coeff", "uniform_dt", "n_rows", "n_rows_tiled", "required_bytes_per_row", "n_groups",
            "n_clean_groups", "n_devices", "quiet_share", "lanes_per_track")
    print("LAYOUT", tag, {k: info[k] for k in keys}, more)


def _same(a, b):
    for k in ("mean", "cov", "resid"):
        if a[k] is not None or b[k] is not None:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def _states(pb):
    s = np.ones(pb.n, dtype=bool)
    s[pb.seg_start] = False
    return s


# ---- drift columns in the tiles (k_iso_drift layouts) ---------------------------------------------------------------------------
def _drift_problem(model, d, what, seed, fe_slope=False, smooth_dims=(0,), fix=()):
    rng = np.random.default_rng(seed)
    ID, times, obs = _tracks(rng, model, d, LENGTHS70, irregular=(what == "irregular"))
    n = len(ID)
    if what == "missing":
        obs[[3, 19, 40, 41, n - 1], 0] = np.nan                # column 0 decides; row 19 ends the first track
        obs[[3, 19, n - 1]] = np.nan
    q = capi.n_sde_par(model, d)
    x = np.clip((np.sin(np.linspace(0, 9, n)) + 1) / 2 + 0.05 * rng.standard_normal(n), 0, 1)
    X_fe, X_re, S = [None] * q, [None] * q, []
    if fe_slope:
        X_fe[0] = np.column_stack([np.ones(n), x])
    for a in smooth_dims:
        X_re[a] = bspline_basis(np.clip(x ** (1 + a), 0, 1), n_basis=4 + a)
        S.append(second_difference_penalty(4 + a))
    pb = capi.Problem(model, ID, times, obs, X_fe=X_fe, X_re=X_re if S else None, S_list=S or None)
    if fix:
        fixed = np.zeros(pb.n_par_full, dtype=np.uint8)
        fixed[list(fix)] = 1
        pb = capi.Problem(model, ID, times, obs, X_fe=X_fe, X_re=X_re if S else None, S_list=S or None, par_fixed=fixed)
    par = 0.25 * rng.standard_normal(pb.n_par_full)
    par[0] = rng.uniform(-1.5, 0.0)
    if model == "OU_SSM":
        par[pb.off_fe + pb.fe_off[:d]] += 3.0
    return pb, par, sum(4 + a for a in smooth_dims) + (2 if fe_slope else 0)      # streamed columns (mu_0 ~ 1 + x: the ones and x)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("what", ["clean", "missing", "irregular"])
def test_drift_columns_in_the_tiles(model, d, what, monkeypatch):
    monkeypatch.setenv("SSDE_DRIFT_MIN_TRACKS", "32")
    pb, par, ncols = _drift_problem(model, d, what, seed=60 + d, smooth_dims=(0, 1)[:d])
    got, info, eng = _run(pb, par)
    eng.eval(par)
    info = eng.info()
    eng.close()
    _show(f"drift {model} d={d} {what}", info)
    # iso_drift_kernel on complete tracks of a regular grid, iso_drift_general_kernel (the lanes' own covariance) otherwise
    assert info["path"] == PATH_ISO and info["const_coeff"] == 0 and info["kernel_id"] == (9 if what == "clean" else 10)
    assert info["required_bytes_per_row"] == 8.0 * (d + ncols + (1 if what == "irregular" else 0))
    assert info["n_rows_tiled"] == pb.n and info["n_groups"] == 2
    _compare(got, smooth_ref(pb, par))


@pytest.mark.parametrize("model,d,fix", [("CTCRW", 1, ()), ("OU_SSM", 2, ()), ("BM_SSM", 2, (0, 3))])
def test_drift_with_a_fixed_effect_slope_and_par_fixed(model, d, fix, monkeypatch):
    # mu_0 ~ 1 + x (+ a smooth on the last mu for d = 2); BM_SSM: sigma_obs and sigma held fixed (TMB's map)
    monkeypatch.setenv("SSDE_DRIFT_MIN_TRACKS", "32")
    pb, par, ncols = _drift_problem(model, d, "missing", seed=71, fe_slope=True, smooth_dims=() if d == 1 else (1,), fix=fix)
    got, info, eng = _run(pb, par)
    eng.eval(par)
    info = eng.info()
    eng.close()
    _show(f"drift fe {model} d={d} fix={fix}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 0 and info["kernel_id"] == 10
    assert info["required_bytes_per_row"] == 8.0 * (d + ncols) and info["n_rows_tiled"] == pb.n
    _compare(got, smooth_ref(pb, par))


# ---- basis-table drift: the tiles hold a covariate instead of columns -----------------------------------------------------------
@pytest.mark.parametrize("model,d,ks,what", [("OU_SSM", 1, (9,), "clean"), ("BM_SSM", 2, (0, 6), "clean"), ("CTCRW", 2, (6, 6), "clean"),
                                             ("OU_SSM", 2, (7, 5), "missing"), ("CTCRW", 1, (5,), "irregular")])
def test_basis_table_drift(model, d, ks, what, monkeypatch):
    from test_gpu_drift import _table_batch
    monkeypatch.setenv("SSDE_DRIFT_MIN_TRACKS", "32")
    if model == "CTCRW" or what != "clean":
        monkeypatch.setenv("SSDE_DRIFT_PP_ALL", "1")
    pb, par = _table_batch(model, d, 70, 60, ks, seed=31, what=what)
    got, info, eng = _run(pb, par)
    eng.close()
    _show(f"table {model} d={d} {what}", info)
    nb = sum(1 for k in ks if k)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 0 and info["n_rows_tiled"] == pb.n
    assert info["required_bytes_per_row"] == 8.0 * (d + nb + (1 if what == "irregular" else 0))       # the table form: 8 B per block
    # the reference on the twin problem with the materialised columns (Problem keeps them in X_re next to the table)
    twin = capi.Problem(model, pb.id, pb.times, pb.obs, X_re=pb.X_re, S_list=pb.S_list)
    _compare(got, smooth_ref(twin, par))


# ---- tau / nu columns on the register lanes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("variant", ["tv", "tv2"])
@pytest.mark.parametrize("cv_adj", ["0", "1"])
def test_row_varying_tau_nu_on_the_register_lanes(model, variant, cv_adj, monkeypatch):
    monkeypatch.setenv("SSDE_DRIFT_MIN_TRACKS", "32")
    monkeypatch.setenv("SSDE_CV_ADJ", cv_adj)
    n = sum(LENGTHS70)
    spec = make_spec(f"gl_{variant}_{model}", model, 2, seed=13, lengths=LENGTHS70, variant=variant, irregular=False,
                     na_rows=(5, 19, 60, n - 1))
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    eng.eval(spec["par"])
    info = eng.info()
    eng.close()
    _show(f"colvar {variant} {model} cv_adj={cv_adj}", info)
    # iso_colvar_kernel / iso_few_kernel, or the reverse sweep iso_adj_kernel under SSDE_CV_ADJ=1: the tiles are the same
    assert info["path"] == PATH_ISO and info["const_coeff"] == 0 and info["kernel_id"] in (11, 12, 17)
    assert info["n_rows_tiled"] == pb.n and info["required_bytes_per_row"] == 8.0 * (2 + (6 if variant == "tv" else 11))
    _compare(got, smooth_ref(pb, spec["par"]))


@pytest.mark.parametrize("with_h", [False, True])
def test_a_smooth_shared_by_tau_and_nu_and_per_row_h(with_h, monkeypatch):
    # one basis on tau and on nu (streamed once); with_h: per-row H_array, the full-covariance lanes' tile layout
    monkeypatch.setenv("SSDE_DRIFT_MIN_TRACKS", "32")
    rng = np.random.default_rng(9)
    ID, times, obs = _tracks(rng, "CTCRW", 2, LENGTHS70, irregular=False)
    n = len(ID)
    obs[[4, 19, n - 1]] = np.nan
    x = np.clip((np.sin(np.arange(n) * 0.11) + 1) / 2, 0, 1)
    B = bspline_basis(x, 5)
    H = None
    if with_h:
        A = rng.standard_normal((n, 2, 2)) * 0.2
        H = np.einsum("nij,nkj->ikn", A, A) + 0.05 * np.eye(2)[:, :, None]
    pb = capi.Problem("CTCRW", ID, times, obs, X_re=[None, None, B, B], S_list=[second_difference_penalty(5)] * 2, H=H)
    par = np.r_[-0.7, 0.05, -0.05, 0.3, 0.1, 0.2, 0.4, 0.2 * rng.standard_normal(10)]
    got, info, eng = _run(pb, par)
    eng.eval(par)
    info = eng.info()
    eng.close()
    _show(f"colvar shared basis with_h={with_h}", info)
    # the five columns once (not ten); per-row H: four more doubles per row (the full-covariance lanes' tiles)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 0 and info["n_rows_tiled"] == pb.n
    assert info["required_bytes_per_row"] == 8.0 * (2 + 5 + (4 if with_h else 0))
    _compare(got, smooth_ref(pb, par))


# ---- lanes dealt by where the tracks miss rows ----------------------------------------------------------------------------------
def _sparse_na_batch(model, d, seed, complete_share):
    """regular grid, ragged tracks; every track (but a share of complete ones) misses one or two rows"""
    rng = np.random.default_rng(seed)
    lengths = [int(v) for v in rng.integers(8, 40, size=200 if complete_share else 130)]
    lengths[2], lengths[4] = 1, 2
    ID, times, obs = _tracks(rng, model, d, lengths, irregular=False)
    starts = np.r_[0, np.cumsum(lengths)[:-1]]
    for k, (s, L) in enumerate(zip(starts, lengths)):
        if L < 3 or rng.random() < complete_share:
            continue
        for r in rng.integers(1, L, size=int(rng.integers(1, 3))):
            obs[s + r] = np.nan
    obs[lengths[0] - 1] = np.nan                                # the first track ends in an NA row
    return capi.Problem(model, ID, times, obs)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("mixed", [False, True])
def test_lanes_dealt_by_missing_rows(model, mixed, monkeypatch):
    """quiet-row handles (every wavefront holds missing rows) and mixed batches (complete wavefronts next to incomplete ones,
    kernel_id 7): lane order differs from track order, with the dealing and without it (SSDE_NO_REGROUP / SSDE_NO_NA_SORT)"""
    from test_gpu_lattice import _par
    monkeypatch.setenv("SSDE_QUIET_ALWAYS", "1")
    pb = _sparse_na_batch(model, 2, seed=77, complete_share=0.6 if mixed else 0.0)
    par = _par(model, 2, np.random.default_rng(3))
    got, info, eng = _run(pb, par)
    eng.eval(par)
    info = eng.info()
    eng.close()
    _show(f"na-dealt {model} mixed={mixed}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n
    if mixed:
        assert info["n_clean_groups"] >= 1 and info["n_clean_groups"] < info["n_groups"] and info["kernel_id"] == 7
    else:
        assert info["n_clean_groups"] == 0 and info["kernel_id"] in (4, 5, 6)
    ref = smooth_ref(pb, par)
    _compare(got, ref)
    monkeypatch.setenv("SSDE_NO_REGROUP", "1")
    monkeypatch.setenv("SSDE_NO_NA_SORT", "1")
    got2, info2, eng2 = _run(pb, par)
    eng2.close()
    _show(f"na-dealt {model} mixed={mixed} NO_REGROUP", info2)
    assert info2["path"] == PATH_ISO and info2["n_clean_groups"] != info["n_clean_groups"]      # the tracks sit on other lanes
    _compare(got2, ref)
    _compare(got2, got)


# ---- caller's a0, block and general P0 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p0", ["block", "general"])
def test_callers_a0_with_a_block_and_a_general_p0(p0):
    # the construction of test_gpu_edge_cases.py::test_user_a0_and_block_identical_p0_stay_on_register_path, every track its own a0
    M, T = 70, 30
    ID, times, obs = simulate("CTCRW", M, T, 2, seed=6)
    a0 = np.zeros((M, 4)); a0[:, 0] = obs[::T, 0] + 0.3; a0[:, 1] = 0.2; a0[:, 2] = obs[::T, 1]; a0[:, 3] = -0.1
    a0 += 0.01 * np.arange(M)[:, None]
    keep = np.ones(len(ID), dtype=bool)
    keep[2 * T + 1:3 * T] = False; keep[4 * T + 2:5 * T] = False      # a one-row and a two-row track
    ID, times, obs = ID[keep], times[keep], obs[keep]
    obs[T - 1] = np.nan
    if p0 == "block":
        P0 = np.kron(np.eye(2), np.array([[2.0, 0.3], [0.3, 4.0]]))
    else:
        A = np.random.default_rng(1).standard_normal((4, 4))
        P0 = A @ A.T + np.eye(4)
    pb = capi.Problem("CTCRW", ID, times, obs, a0=a0, P0=P0)
    par = np.array([-0.8, 0.05, -0.05, 0.4, 0.1])
    got, info, eng = _run(pb, par)
    eng.close()
    _show(f"a0 {p0} P0", info)
    assert info["path"] == (PATH_ISO if p0 == "block" else PATH_TV)      # a general P0: the full-covariance lanes of the TV route
    _compare(got, smooth_ref(pb, par))


@pytest.mark.parametrize("model", MODELS)
def test_callers_a0_on_the_tv_route_is_indexed_by_the_sorted_track(model):
    # a few tracks of different lengths with row-varying parameters: PATH_TV sorts them by length, a0 must follow
    spec = make_spec(f"gl_a0tv_{model}", model, 2, seed=19, lengths=[120, 300, 1, 210, 2, 260], variant="tv", na_rows=(7, 119))
    sd = 4 if model == "CTCRW" else 2
    rng = np.random.default_rng(4)
    starts = np.r_[0, np.cumsum([120, 300, 1, 210, 2, 260])[:-1]]
    a0 = np.zeros((6, sd))
    for a in range(2):
        a0[:, 2 * a if model == "CTCRW" else a] = spec["obs"][starts, a]
    a0 += 0.3 * rng.standard_normal(a0.shape)
    spec["a0"] = a0
    spec["P0"] = np.kron(np.eye(2), np.array([[2.0, 0.3], [0.3, 4.0]])) if model == "CTCRW" else 3.0 * np.eye(2)
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    eng.close()
    _show(f"a0 tv {model}", info)
    assert info["path"] == PATH_TV
    _compare(got, smooth_ref(pb, spec["par"]))


# ---- R's NA_real_ ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_r_na_in_column_0_only(model):
    n = sum(LENGTHS70)
    spec = make_spec(f"gl_rna_{model}", model, 2, seed=23, lengths=LENGTHS70, na_mode=0)
    rows = [5, 19, 30, n - 1]
    spec["obs"][rows, 0] = capi.na_real()                      # column 1 keeps its number
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    eng.close()
    _show(f"R-NA {model}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1
    assert np.all(np.isnan(got["resid"][rows])) and np.all(np.isfinite(got["mean"][rows]))   # residual NaN, state a prediction
    _compare(got, smooth_ref(pb, spec["par"]))


@pytest.mark.parametrize("model", MODELS)
def test_plain_nan_is_data_under_r_na_semantics(model):
    # na_mode = 0: a plain NaN takes the update (in column 0 too); that track's means are NaN, its covariances finite, the row's
    # residual NaN from the NaN column on -- and no other lane of the wavefront is touched
    spec = make_spec(f"gl_nan_{model}", model, 2, seed=27, lengths=LENGTHS70, na_mode=0)
    spec["obs"][5, 0] = capi.na_real()
    spec["obs"][25, 0] = np.nan                                # track 1 (rows 20 ... 54)
    spec["obs"][60, 1] = np.nan                                # track 3 (rows 56 ... 69)
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    eng.close()
    _show(f"plain NaN {model}", info)
    assert info["path"] == PATH_ISO and info["const_coeff"] == 1 and info["n_rows_tiled"] == pb.n
    with np.errstate(invalid="ignore"):
        ref = smooth_ref(pb, spec["par"])
    assert np.all(np.isnan(ref["mean"][21:55])) and np.all(np.isfinite(ref["cov"][21:55])) and np.all(np.isfinite(ref["mean"][1:20]))
    assert np.isfinite(ref["resid"][60, 0]) and np.isnan(ref["resid"][60, 1])
    _compare(got, ref)


# ---- PATH_TV with many tracks: groups, chunks, one-row tracks -------------------------------------------------------------------
def _tv_many(model, seed, **kw):
    rng = np.random.default_rng(seed)
    lengths = [int(v) for v in rng.integers(24, 65, size=150)]
    lengths[3], lengths[70], lengths[129] = 1, 1, 2
    starts = np.r_[0, np.cumsum(lengths)]
    return make_spec(f"gl_tvm_{model}", model, 2, seed=seed, lengths=lengths, variant="tv",
                     na_rows=(6, lengths[0] - 1, int(starts[50]) + 5, int(starts[-1]) - 1), **kw)


@pytest.mark.parametrize("model,extra", [("CTCRW", "H"), ("CTCRW", "P0"), ("OU_SSM", "H"), ("BM_SSM", "P0")])
def test_tv_route_with_more_than_one_group_and_chunks(model, extra, monkeypatch):
    monkeypatch.setenv("SSDE_NO_COLVAR", "1")
    monkeypatch.setenv("SSDE_NO_DRIFT", "1")
    spec = _tv_many(model, seed=29, with_H=extra == "H", with_P0=extra == "P0")
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"tv many {model} {extra}", info)
    assert info["path"] == PATH_TV and info["n_tracks"] == 150        # three groups of lanes by length, the last with 22 tracks
    one = eng.smooth(spec["par"])
    # 1 MiB = 131072 doubles.  CTCRW: 31 doubles x 64 lanes per step and groups of 63, 46 and 26 steps -- no two of them fit, each
    # group is its own chunk; the scalar models' 18-double records: the first two groups fit, the third starts a second chunk
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.smooth(spec["par"])
    eng.close()
    _same(one, many)
    _compare(one, smooth_ref(pb, spec["par"]))


# ---- chunking on ragged tiled groups --------------------------------------------------------------------------------------------
def test_chunks_on_ragged_tiled_groups_are_bitwise():
    # six groups of very different lengths (tracks go to lanes longest first).  1 MiB = 131072 doubles is below the first group's
    # records (>= 70 steps x 31 doubles x 64 lanes), and the second group's (>= 59 steps) do not fit next to the third's: three chunks,
    # [g0], [g1], [g2 ... g5], so rec_off[g] - rec_base differs from rec_off[g] and, in the last chunk, from 0
    rng = np.random.default_rng(31)
    lengths = np.r_[rng.integers(71, 90, 64), rng.integers(45, 61, 63), [60], rng.integers(10, 16, 64), rng.integers(3, 8, 64),
                    rng.integers(2, 4, 64), [1, 2, 5, 1, 3]]
    lengths = [int(v) for v in rng.permutation(lengths)]
    starts = np.r_[0, np.cumsum(lengths)]
    k5 = next(k for k, L in enumerate(lengths) if L >= 5)
    spec = make_spec("gl_chunks", "CTCRW", 2, seed=31, lengths=lengths, irregular=True,
                     na_rows=(int(starts[k5]) + 2, int(starts[k5]) + 3, int(starts[k5 + 1]) - 1))
    pb = problem_from_spec(spec)
    eng = capi.Engine(pb)
    info = eng.info()
    _show("chunks ragged", info)
    assert info["path"] == PATH_ISO and info["n_groups"] == 6
    one = eng.smooth(spec["par"])
    eng.set_option(capi.OPT_SMOOTH_BUDGET_MB, 1)
    many = eng.smooth(spec["par"])
    eng.close()
    _same(one, many)
    _compare(one, smooth_ref(pb, spec["par"]))


# ---- widths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,d", [("CTCRW", 5), ("CTCRW", 7), ("CTCRW", 8), ("OU_SSM", 5), ("OU_SSM", 8), ("BM_SSM", 5), ("BM_SSM", 8)])
def test_coupled_wide_responses(model, d):
    # a per-row H couples the columns: one filter of width d (k_dense_wide.hip records, k_smooth_wide.hip backward)
    spec = make_spec(f"glw_{model}_{d}", model, d, seed=30 + d, lengths=LENGTHS70[:67], with_H=True, na_rows=(2, 19))
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    eng.close()
    _show(f"wide coupled {model} d={d}", info)
    assert info["path"] == PATH_DENSE and info["sdim"] == pb.sdim and info["n_devices"] <= 1
    _compare(got, smooth_ref(pb, spec["par"]))


@pytest.mark.parametrize("model,d", [("CTCRW", 5), ("OU_SSM", 3), ("BM_SSM", 5)])
def test_uncoupled_odd_widths_run_as_column_pairs(model, d):
    # pairs plus a single column: r0 = c0 / per decides where a part's residual columns land
    spec = make_spec(f"glu_{model}_{d}", model, d, seed=40 + d, lengths=LENGTHS70[:67], na_rows=(2, 19))
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    eng.close()
    _show(f"wide uncoupled {model} d={d}", info)
    assert info["path"] == PATH_ISO and info["n_rows_tiled"] == pb.n * ((d + 1) // 2)       # the parts: pairs and a single column
    _compare(got, smooth_ref(pb, spec["par"]))
    per = 2 if model == "CTCRW" else 1
    pair = np.arange(pb.sdim) // (2 * per)
    cross = pair[:, None] != pair[None, :]
    st = _states(pb)
    assert np.all(got["cov"][st][:, cross] == 0.0)             # cross-pair blocks: exactly zero ...
    assert np.all(np.isnan(got["cov"][~st]))                   # ... and all NaN on a row without a state


# ---- shards x other layouts -----------------------------------------------------------------------------------------------------
def test_shards_of_a_lattice_handle():
    from test_gpu_lattice import _par, lattice_tracks
    ID, times, obs = lattice_tracks("CTCRW", 2, [40, 25, 1, 33, 2, 18] * 12, 0.5, 0.15, seed=8, na_frac=0.05)
    obs[39] = np.nan
    pb = capi.Problem("CTCRW", ID, times, obs)
    par = _par("CTCRW", 2, np.random.default_rng(2))
    got, info, eng = _run(pb, par, devices=[0, 0])
    eng.close()
    _show("shards lattice", info)
    assert info["n_devices"] == 2 and info["n_rows_tiled"] > pb.n
    _compare(got, smooth_ref(pb, par))


def test_shards_of_a_tv_handle(monkeypatch):
    monkeypatch.setenv("SSDE_NO_COLVAR", "1")
    monkeypatch.setenv("SSDE_NO_DRIFT", "1")
    spec = _tv_many("OU_SSM", seed=37)
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"], devices=[0, 0])
    eng.close()
    _show("shards tv", info)
    assert info["n_devices"] == 2 and info["path"] == PATH_TV
    _compare(got, smooth_ref(pb, spec["par"]))


def test_shards_of_column_pairs():
    spec = make_spec("gl_shard_pairs", "CTCRW", 4, seed=43, lengths=LENGTHS70, na_rows=(2, 19))
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"], devices=[0, 0])
    eng.close()
    _show("shards of pairs", info)
    assert info["n_devices"] == 2 and info["path"] == PATH_ISO and info["n_rows_tiled"] == 2 * pb.n
    _compare(got, smooth_ref(pb, spec["par"]))
    pair = np.arange(8) // 4
    assert np.all(got["cov"][_states(pb)][:, pair[:, None] != pair[None, :]] == 0.0)


# ---- det F <= 0 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("dense", [False, True])
def test_nonpositive_innovation_variance_branch(model, dense):
    """The negative-P0 construction of test_gpu_edge_cases.py (an ordinary finite computation): CTCRW skips the update while
    det F <= 0 and predicts without B mu; OU_SSM / BM_SSM update with a negative F, whose whitened innovation is NaN."""
    ID, times, obs = simulate(model, 70, 12, 1, seed=4)
    keep = np.ones(len(ID), dtype=bool)
    keep[2 * 12 + 1:3 * 12] = False; keep[4 * 12 + 2:5 * 12] = False
    ID, times, obs = ID[keep], times[keep], obs[keep]
    obs[11] = np.nan
    sdim = 2 if model == "CTCRW" else 1
    P0 = -np.eye(sdim) * 5.0 if sdim == 1 else np.diag([-5.0, 1.0])
    par = np.array([-2.0, 0.7, 0.3, 0.1] if model != "BM_SSM" else [-2.0, 0.7, 0.1])
    pb = capi.Problem(model, ID, times, obs, P0=P0, flags=capi.FLAG_FORCE_DENSE if dense else 0)
    got, info, eng = _run(pb, par)
    eng.close()
    _show(f"detF {model} dense={dense}", info)
    assert info["path"] == (PATH_DENSE if dense else PATH_ISO)
    ref = smooth_ref(pb, par)
    assert np.all(np.isfinite(ref["mean"][_states(pb)])) and np.all(np.isnan(ref["resid"][pb.seg_start[0] + 1]))
    _compare(got, ref)


# ---- device-resident data -------------------------------------------------------------------------------------------------------
def test_device_resident_inputs_are_bitwise_the_host_handles(monkeypatch):
    import torch
    from smoothsde_amd.synth import bspline_ppbasis
    from test_gpu_drift import _centre_of, _table_batch
    dev = "cuda:0"
    spec = make_spec("gl_dev", "CTCRW", 2, seed=47, lengths=LENGTHS70, irregular=False, na_rows=(5, 19))
    pb = problem_from_spec(spec)
    got, info, eng = _run(pb, spec["par"])
    eng.close()
    pbd = capi.Problem.from_torch("CTCRW", torch.tensor(pb.id, device=dev), torch.tensor(pb.times, device=dev), torch.tensor(pb.obs, device=dev))
    gd, infod, ed = _run(pbd, spec["par"])
    ed.close()
    _show("device const", infod)
    assert infod["path"] == info["path"] == PATH_ISO and infod["const_coeff"] == 1
    _same(got, gd)
    _compare(got, smooth_ref(pb, spec["par"]))
    # ... and a table-drift batch whose covariate lives in HBM
    monkeypatch.setenv("SSDE_DRIFT_MIN_TRACKS", "32")
    pbt, par = _table_batch("OU_SSM", 1, 70, 60, (9,), seed=5)
    gt, infot, et = _run(pbt, par)
    et.close()
    bd = bspline_ppbasis(torch.tensor(np.asarray(pbt.basis_re[0].x), device=dev), 9, centre=_centre_of(pbt.basis_re[0]))
    pbtd = capi.Problem.from_torch("OU_SSM", torch.tensor(pbt.id, device=dev), torch.tensor(pbt.times, device=dev),
                                   torch.tensor(pbt.obs, device=dev), basis_re=[bd, None, None], S_list=pbt.S_list)
    gtd, infotd, etd = _run(pbtd, par)
    etd.close()
    _show("device table", infotd)
    assert infotd["path"] == infot["path"] == PATH_ISO and infotd["required_bytes_per_row"] == infot["required_bytes_per_row"] == 16.0
    _same(gt, gtd)


# ---- ABI corners ----------------------------------------------------------------------------------------------------------------
def test_residuals_only_and_covariance_only_through_the_raw_call():
    from cases import eseal_spec
    spec = make_spec("gl_abi", "CTCRW", 2, seed=53, lengths=LENGTHS70, na_rows=(5, 19))
    pb = problem_from_spec(spec)
    full, info, eng = _run(pb, spec["par"])
    p = np.ascontiguousarray(spec["par"])
    dp = p.ctypes.data_as(C.POINTER(C.c_double))
    e = np.zeros((pb.n, 2), order="F")
    V = np.zeros((pb.n, 4, 4), order="F")
    assert eng.lib.ssde_smooth(eng._h, dp, pb.n_par_full, None, None, e.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert eng.lib.ssde_smooth(eng._h, dp, pb.n_par_full, None, V.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
    eng.close()
    assert np.array_equal(e, full["resid"], equal_nan=True) and np.array_equal(V, full["cov"], equal_nan=True)
    # ... and on a parent of column pairs (a_smooth = NULL through smooth_sharded)
    spec = make_spec("gl_abi3", "OU_SSM", 3, seed=54, lengths=LENGTHS70, na_rows=(5, 19))
    pb = problem_from_spec(spec)
    full, info, eng = _run(pb, spec["par"])
    p = np.ascontiguousarray(spec["par"])
    dp = p.ctypes.data_as(C.POINTER(C.c_double))
    e = np.zeros((pb.n, 3), order="F")
    V = np.zeros((pb.n, 3, 3), order="F")
    assert eng.lib.ssde_smooth(eng._h, dp, pb.n_par_full, None, None, e.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert eng.lib.ssde_smooth(eng._h, dp, pb.n_par_full, None, V.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
    eng.close()
    assert np.array_equal(e, full["resid"], equal_nan=True) and np.array_equal(V, full["cov"], equal_nan=True)
    for sp in (eseal_spec("gl_eseal", 211, [14, 9, 11]), make_spec("gl_cir", "CIR", 1, seed=221, lengths=[9, 2, 14])):
        ed = capi.Engine(problem_from_spec(sp))
        with pytest.raises(capi.EngineError) as ei:
            ed.smooth(sp["par"])
        assert ei.value.status == 2                                   # SSDE_ERR_MODEL
        ed.close()


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_sde_smooth_states_and_residuals_on_a_state_space_model():
    from smoothsde_amd.sde import SDE
    rng = np.random.default_rng(61)
    ID, times, obs = _tracks(rng, "CTCRW", 2, LENGTHS70, irregular=True)
    n = len(ID)
    obs[[5, 19]] = np.nan
    data = {"ID": ID, "time": times, "x": np.clip((np.sin(np.linspace(0, 7, n)) + 1) / 2, 0, 1), "z0": obs[:, 0], "z1": obs[:, 1]}
    sde = SDE(formulas={"mu1": "~1", "mu2": "~1", "tau": "~x", "nu": "~1"}, data=data, type="CTCRW", response=["z0", "z1"])
    sde.coeff_fe_ = np.array([0.05, -0.05, 0.3, 0.4, 0.1])
    sde.setup()
    st, res = sde.smooth_states(), sde.residuals()
    par = sde._current_par_full()
    direct = sde.engine_.smooth(par)
    assert np.array_equal(st["mean"], direct["mean"], equal_nan=True) and np.array_equal(st["cov"], direct["cov"], equal_nan=True)
    assert np.array_equal(res, direct["resid"], equal_nan=True)
    info = sde.engine_.info()
    _show("SDE tau ~ x", info)
    assert info["const_coeff"] == 0 and info["path"] == PATH_TV
    _compare({"mean": st["mean"], "cov": st["cov"], "resid": res}, smooth_ref(sde.problem_, par))


# ---- seeded fuzz ----------------------------------------------------------------------------------------------------------------
# Kalman-family seeds of test_gpu_fuzz.random_problem, picked on the CPU: smooth_ref is finite wherever a state exists and agrees with
# joint_track to 1e-9 on every one of them (test_smooth_hostsim.py::test_fuzz_seeds_are_sound keeps that true)
FUZZ_SEEDS = [1, 8, 10, 40, 41, 56, 57, 58, 88, 98, 105, 112]
FUZZ_WIDE_SEEDS = [7, 18, 109, 115, 122, 126]
# ... and the route each of them takes (info()["path"]; a wide parent reports its first part's)
FUZZ_PATH = {(1, False): 3, (8, False): 1, (10, False): 1, (40, False): 3, (41, False): 1, (56, False): 3, (57, False): 3, (58, False): 3,
             (88, False): 3, (98, False): 3, (105, False): 3, (112, False): 3,
             (7, True): 3, (18, True): 1, (109, True): 3, (115, True): 2, (122, True): 3, (126, True): 3}


@pytest.mark.parametrize("seed,wide", [(s, False) for s in FUZZ_SEEDS] + [(s, True) for s in FUZZ_WIDE_SEEDS])
def test_random_problem_smooth_matches_the_reference(seed, wide):
    from test_gpu_fuzz import random_problem
    pb, par = random_problem(seed, wide=wide)
    eng = capi.Engine(pb)
    info = eng.info()
    _show(f"fuzz {seed} wide={wide} {pb.model} d={pb.n_dim} n={pb.n} tracks={pb.n_seg}", info)
    got = eng.smooth(par)
    rep = eng.report(par)
    eng.close()
    assert info["path"] == FUZZ_PATH[(seed, wide)]
    _compare(got, smooth_ref(pb, par))
    # a track's trailing NA rows: the smoothed state there is the forward prediction (REPORT's aest_all row i is the state of row i + 1)
    bounds = list(pb.seg_start) + [pb.n]
    for k in range(pb.n_seg):
        i = bounds[k + 1] - 1
        while i > bounds[k] and np.isnan(pb.obs[i, 0]):
            assert np.allclose(got["mean"][i], rep[i - 1], rtol=0, atol=1e-10 * (1 + np.abs(rep[i - 1]).max())), (k, i)
            i -= 1
