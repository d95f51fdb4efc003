"""CPU suite: the engine's SSDE_* environment variables.  csrc/ssde_knobs.hpp is the only file of the library that
reads the environment and names every variable once; DESIGN.md §8 lists the same names; and knobs_from_env -- compiled for the
host by tests/hostsim -- normalises the values the way the dispatch rules expect them."""
import os
import re

import pytest

import hostsim_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smoothsde_amd", "csrc")


def _read(*parts):
    with open(os.path.join(*parts), encoding="utf-8") as f:
        return f.read()


def _header_names():
    return re.findall(r'"(SSDE_[A-Z0-9_]+)"', _read(CSRC, "ssde_knobs.hpp"))


WIN_ALIGN = int(re.search(r"constexpr int WIN_ALIGN = (\d+);", _read(CSRC, "ssde_device.hpp")).group(1))


def test_only_the_knobs_header_reads_the_environment_and_names_each_variable_once():
    readers = sorted(f for f in os.listdir(CSRC) if "getenv" in _read(CSRC, f))
    assert readers == ["ssde_knobs.hpp"]
    names = _header_names()
    assert names and sorted(names) == sorted(set(names))


def test_design_section_8_lists_exactly_the_variables_of_the_header():
    section = re.search(r"^## 8\. .*?(?=^## |\Z)", _read(ROOT, "DESIGN.md"), re.S | re.M).group(0)
    rows = [r for r in section.splitlines() if r.startswith("| `SSDE_")]
    engine_rows = [r for r in rows if "not read by the library" not in r]
    assert len(engine_rows) == len(rows) - 1                  # (one row of Python-side / build-time names)
    documented = set()
    for r in engine_rows:
        documented |= set(re.findall(r"SSDE_[A-Z0-9_]+", r.split("|")[1]))
    assert documented == set(_header_names())


@pytest.fixture
def clean_env(monkeypatch):
    for name in _header_names():
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_no_variable_set_is_the_documented_default(clean_env):
    k = hostsim_lib.knobs(WIN_ALIGN)
    assert set(k) == set(_header_names())
    unset = {"SSDE_CHUNKS", "SSDE_WINDOW", "SSDE_ADJ_TAIL", "SSDE_TV_WAVES", "SSDE_TV_MINLEN", "SSDE_HESS_WINDOW", "SSDE_ISO_SPLIT",
             "SSDE_DRIFT_MIN_TRACKS", "SSDE_CV_ADJ", "SSDE_LAGSTATS", "SSDE_FUSED_FINALIZE", "SSDE_WAVE_CLOCK"}
    for name, v in k.items():
        if name in unset:
            assert v == "unset", (name, v)
        elif name == "SSDE_GRID_RTOL":
            assert float(v) == 1e-12
        else:
            assert v == "0", (name, v)                            # switches off, SSDE_QUIET_WINDOW / SSDE_ADJ_DIAG 0


@pytest.mark.parametrize("name, value, parsed", [
    ("SSDE_WINDOW", "0", "1"), ("SSDE_WINDOW", "48", "48"),
    ("SSDE_ADJ_TAIL", "-3", "1"), ("SSDE_TV_WAVES", "0", "1"),
    ("SSDE_TV_MINLEN", "1", str(WIN_ALIGN)), ("SSDE_TV_MINLEN", str(3 * WIN_ALIGN + 5), str(3 * WIN_ALIGN)),
    ("SSDE_HESS_WINDOW", "0", str(WIN_ALIGN)), ("SSDE_HESS_WINDOW", str(WIN_ALIGN), str(WIN_ALIGN)),
    ("SSDE_HESS_WINDOW", str(2 * WIN_ALIGN + 1), str(3 * WIN_ALIGN)), ("SSDE_HESS_WINDOW", "2147483647", str(1 << 24)),
    ("SSDE_QUIET_WINDOW", "-5", "0"), ("SSDE_QUIET_WINDOW", "32", "32"),
    ("SSDE_LAGSTATS", "0", "0"), ("SSDE_LAGSTATS", "1", "1"), ("SSDE_LAGSTATS", "2", "2"), ("SSDE_LAGSTATS", "7", "1"),
    ("SSDE_FUSED_FINALIZE", "0", "0"), ("SSDE_FUSED_FINALIZE", "1", "1"),
    ("SSDE_CV_ADJ", "0", "0"), ("SSDE_CV_ADJ", "2", "2"),
    ("SSDE_NO_QUIET", "0", "1"), ("SSDE_NO_SHARED", "", "1"),
    ("SSDE_CHUNKS", "1", "1"), ("SSDE_DRIFT_MIN_TRACKS", "32", "32"),
    ("SSDE_ADJ_DIAG", "5", "5"),
    ("SSDE_ISO_SPLIT", "3,4,8", "3,4,8"), ("SSDE_WAVE_CLOCK", "/tmp/w.txt", "/tmp/w.txt"),
])
def test_one_variable_set_is_normalised_and_leaves_the_others_alone(clean_env, name, value, parsed):
    base = hostsim_lib.knobs(WIN_ALIGN)
    clean_env.setenv(name, value)
    k = hostsim_lib.knobs(WIN_ALIGN)
    assert k[name] == parsed
    assert {n: v for n, v in k.items() if n != name} == {n: v for n, v in base.items() if n != name}


@pytest.mark.parametrize("value, parsed", [("-1", 0.0), ("0", 0.0), ("1e-9", 1e-9)])
def test_grid_rtol_is_clamped_at_zero(clean_env, value, parsed):
    clean_env.setenv("SSDE_GRID_RTOL", value)
    assert float(hostsim_lib.knobs(WIN_ALIGN)["SSDE_GRID_RTOL"]) == parsed
