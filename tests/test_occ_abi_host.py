"""CPU suite: the additive C ABI of ssde_path_occupancy (include/ssde.h against smoothsde_amd/capi.py) and the host-side plans of
the call (csrc/ssde_smooth_plan.hpp through the small entry points of tests/hostsim/hostsim_occ.cpp)."""
import ctypes as C
import os
import re

import numpy as np

import occsim_lib
from occ_ref import quantise, quantum_exp
from smoothsde_amd import capi

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssde.h")
NW, DRAW_CH, WAVE, TILE_CELLS, MIXED = 4, 4, 64, 8192, -2        # csrc/ssde_device.hpp: OCC_NW, DRAW_CH, WAVE, OCC_TILE_CELLS


def _header():
    with open(HEADER) as f:
        return f.read()


def test_the_header_declares_both_calls_and_capi_exports_them():
    text = _header()
    assert re.search(r"\bint\s+ssde_path_occupancy\s*\(\s*ssde_handle\s*\*h,\s*const double\s*\*par,\s*int32_t n_par_full,\s*uint64_t seed,"
                     r"\s*int64_t draw0,\s*int32_t n_draws,\s*const ssde_occ_grid\s*\*grid,\s*const double\s*\*weight,"
                     r"\s*const int32_t\s*\*group,\s*int32_t n_groups,\s*double\s*\*occ,\s*double\s*\*outside,\s*uint32_t flags\)\s*;", text)
    assert re.search(r"\bint\s+ssde_last_occupancy_form\s*\(\s*const ssde_handle\s*\*h\)\s*;", text)
    assert "ssde_path_occupancy" in capi.EXPORTED_SYMBOLS and "ssde_last_occupancy_form" in capi.EXPORTED_SYMBOLS


def test_the_abi_version_and_the_flag():
    text = _header()
    assert re.search(r"^#define SSDE_ABI_VERSION 12$", text, re.M) and capi.ABI_VERSION == 12
    assert re.search(r"^#define SSDE_OCC_FORCE_GLOBAL 1u$", text, re.M) and capi.OCC_FORCE_GLOBAL == 1


def test_the_grid_structure_matches_its_ctypes_mirror():
    m = re.search(r"typedef struct ssde_occ_grid \{([^}]*)\} ssde_occ_grid;", _header())
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == [("x0", "double"), ("dx", "double"), ("y0", "double"), ("dy", "double"), ("nx", "int32_t"), ("ny", "int32_t")]
    ctypes_of = {"double": C.c_double, "int32_t": C.c_int32}
    assert [(n, t) for n, t in capi.SsdeOccGrid._fields_] == [(n, ctypes_of[t]) for n, t in fields]
    assert C.sizeof(capi.SsdeOccGrid) == 40


def test_the_batch_rule_gives_whole_workgroups_within_one_launch():
    unit = NW * DRAW_CH
    for n_draws in (1, 4, 5, unit, unit + 1, 1000, 131072, 131073, 300000, (1 << 28) - 1):
        cap = occsim_lib.batch_cap(NW, DRAW_CH, n_draws)
        assert 1 <= cap <= n_draws
        n_batches = -(-n_draws // cap)
        assert n_batches >= 1 and (n_batches == 1 or cap % unit == 0)              # every batch but the last: whole workgroups
        assert -(-cap // DRAW_CH) <= 65535 and -(-cap // unit) <= 65535            # the second grid dimension of both forms
        assert cap == n_draws or cap == (DRAW_CH << 15)                           # as many as one launch takes: fewer record passes


def test_the_form_of_every_wavefront_group():
    pooled = np.zeros(130, dtype=np.int32)
    assert list(occsim_lib.plan_groups(pooled, WAVE, 192, TILE_CELLS)) == [0, 0, 0]
    assert list(occsim_lib.plan_groups(pooled, WAVE, 192, TILE_CELLS, force_global=True)) == [MIXED] * 3
    assert list(occsim_lib.plan_groups(pooled, WAVE, TILE_CELLS, TILE_CELLS)) == [0, 0, 0]
    assert list(occsim_lib.plan_groups(pooled, WAVE, TILE_CELLS + 1, TILE_CELLS)) == [MIXED] * 3
    split = np.r_[np.zeros(64), np.ones(66)].astype(np.int32)
    assert list(occsim_lib.plan_groups(split, WAVE, 192, TILE_CELLS)) == [0, 1, 1]
    alt = (np.arange(130) % 2).astype(np.int32)
    assert list(occsim_lib.plan_groups(alt, WAVE, 192, TILE_CELLS)) == [MIXED] * 3
    head = np.r_[np.zeros(64), np.arange(66) % 2].astype(np.int32)
    assert list(occsim_lib.plan_groups(head, WAVE, 192, TILE_CELLS)) == [0, MIXED, MIXED]
    some = pooled.copy(); some[[3, 70, 129]] = -1
    assert list(occsim_lib.plan_groups(some, WAVE, 192, TILE_CELLS)) == [0, 0, 0]
    none = np.r_[np.full(64, -1), np.full(2, 5)].astype(np.int32)
    assert list(occsim_lib.plan_groups(none, WAVE, 192, TILE_CELLS)) == [-1, 5]
    per_track = np.arange(70, dtype=np.int32)
    assert list(occsim_lib.plan_groups(per_track, WAVE, 192, TILE_CELLS)) == [MIXED, MIXED]
    assert list(occsim_lib.plan_groups(np.array([7], dtype=np.int32), WAVE, 1, TILE_CELLS)) == [7]


def test_the_quantum_rule_of_the_header_is_the_reference_s():
    rng = np.random.default_rng(3)
    for wmax in (1.0, 0.375, 0.0, 5e-324, 1e-310, 0.999, 123.456, 2.0 ** 60, 1e300):
        for n, nd in ((19, 8), (1, 1), (10 ** 7, 32), (4095, 4097), ((1 << 40) + 1, (1 << 28) - 1)):
            assert occsim_lib.twin_quantum_exp(wmax, n, nd) == quantum_exp(wmax, n, nd), (wmax, n, nd)
    w = np.r_[rng.random(200) * 3.7, [0.0, 0.5, 1.5, 2.5, 3.7, 5e-324, 1e-310, 2.0 ** -40 * 1.5, 2.0 ** -40 * 2.5]]
    for e in (quantum_exp(3.7, 209, 5), 0, -1, -30, -40, -41, 1, 2):
        for fast in (False, True):
            assert np.array_equal(occsim_lib.twin_quantise(w, e, fast=fast), quantise(w, e)), (e, fast)
    tiny = np.array([5e-324, 1e-310, 3e-308, 2.0 ** -1074 * 3, 0.0])
    for e in (-1074, -1073, -1030, -1023, -1022):
        for fast in (False, True):
            assert np.array_equal(occsim_lib.twin_quantise(tiny, e, fast=fast), quantise(tiny, e)), (e, fast)
    big = np.array([2.0 ** 60, 2.0 ** 60 * 1.5, 1e300])
    for e in (9, 40, 1000):
        if big.max() * 2.0 ** -e < 2.0 ** 63:
            assert np.array_equal(occsim_lib.twin_quantise(big[:2] if e < 900 else big, e), quantise(big[:2] if e < 900 else big, e))
