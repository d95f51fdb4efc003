"""CPU suite: the gain table by value (smoothsde_amd/csrc/ssde_gain_feed.hpp) -- the packing the engine does and the LDS
slab wave 0 of iso_shared_wg_kernel expands it to, against stage_gain's clamping rule: tests/gainfeed/gainfeed_host.cpp, built here
with g++ into the test's own directory.  Rows = 1, a few, the capacity; the CTCRW and the scalar column sets; what must be refused."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gainfeed", "gainfeed_host.cpp")


def build_gainfeed(out_dir):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler for tests/gainfeed/gainfeed_host.cpp")
    exe = os.path.join(str(out_dir), "gainfeed_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC], check=True, cwd=str(out_dir))
    return exe


def test_packing_and_slab_against_stage_gains_rule(tmp_path):
    exe = build_gainfeed(tmp_path)
    r = subprocess.run([exe, "check"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("gainfeed: ok"), r.stdout + r.stderr


def test_the_row_counter_counts_the_transient(tmp_path):
    """`rows`: the covariance recursion until it has settled -- a longer transient with a larger observation variance, and one count per line"""
    exe = build_gainfeed(tmp_path)
    r = subprocess.run([exe, "rows", "2", "1.0", "0.6931471805599453", "0.0", "3", "0.0", "1.5", "1", "0", "10"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [int(line.split()[1]) for line in r.stdout.strip().splitlines()]
    assert len(rows) == 3 and 4 < rows[0] < rows[1] < rows[2] < 1000, rows
