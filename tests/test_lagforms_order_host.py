"""CPU suite: the order of the sums in the bulk's forms (ssde_lagforms.hpp: lag_forms_sums through ssde_lagforms_host
and ssde_lagforms_host_isa).  Both cuts come from one pass over the rows of M with eight partial sums per row (lane = tap index
modulo 8) and a tree over the rows that starts at the smallest power of two >= K + 1.

1. The raw sums against direct numpy.longdouble sums over the bulk rows, at the 1e-12 of tests/test_lagforms_host.py on its scale
   max(|sum|, sqrt(|S| n)), with its tracks and its theta.  K = 17 (a check cut of one tap, three blocks of eight of which the last
   holds two taps), 48 (the headline's), 64 (one tap past a whole block; the tree starts at 128) and 191 (every tap).
2. raw[1] of a call (K, K - 16) is raw[0] of a call whose K is that K - 16, by ==: past a cut the one loop adds exact zeros, the
   lanes are the same, and the tree's upper levels add zeros.  (K = 17: the entry refuses a cut of one tap, so there is no second
   call to compare with; that it refuses is asserted.)
3. Two calls give the same bits.
4. The baseline build of the sums and the AVX2 build give the same bits, where the host has AVX2; where it has not, the entry says so."""
import numpy as np
import pytest

from smoothsde_amd import capi
from test_lagforms_host import LENGTHS, TOL, _direct, _scale, _theta, _tracks

KS = [17, 48, 64, 191]
_CACHE = {}


def _setup(d, mu):
    key = (d, mu)
    if key not in _CACHE:
        tracks = _tracks(d, 31 + d)
        M, s, n, A = capi.lagstats_host(tracks)
        assert n == sum(max(0, L - A) for L in LENGTHS)
        _CACHE[key] = (tracks, M, s, n, A, _theta(d, mu))
    return _CACHE[key]


def _bits(f):
    return np.concatenate([f["raw"].reshape(-1), f["acc"], [f["chk"]]]).view(np.uint64)


def _has_wide(M, s, n, theta):
    try:
        capi.lagforms_host(M, s, n, theta, 1.0, 16, isa=1)
        return True
    except ValueError:
        return False


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mu", [0.0, 0.25])
@pytest.mark.parametrize("d", [1, 2])
def test_both_cuts_match_the_direct_sums(d, mu, K):
    tracks, M, s, n, A, theta = _setup(d, mu)
    f = capi.lagforms_host(M, s, n, theta, 1.0, K)
    taps = f["taps"]
    assert np.all(taps[:, K + 1:] == 0.0) and taps[0, 0] != 0.0
    cm = theta[1:1 + d] * 1.0
    for cut, Kc in enumerate((K, K - 16)):
        ref, nref = _direct(tracks, taps, Kc, cm, A, np.longdouble)
        assert nref == n
        for j in range(4 + d):
            err = abs(float(np.longdouble(f["raw"][cut, j]) - ref[j])) / _scale(ref[j], ref[0], n)
            print("d=%d mu=%g K=%d cut=%d sum %d: %.3e" % (d, mu, K, Kc, j, err))
            assert err <= TOL, (cut, j, err, f["raw"][cut, j], float(ref[j]))
        if d == 1:
            assert f["raw"][cut, 5] == 0.0


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("mu", [0.0, 0.25])
@pytest.mark.parametrize("d", [1, 2])
def test_the_check_cut_is_the_shorter_calls_cut_and_calls_repeat(d, mu, K):
    _, M, s, n, _, theta = _setup(d, mu)
    f = capi.lagforms_host(M, s, n, theta, 1.0, K)
    g = capi.lagforms_host(M, s, n, theta, 1.0, K)
    assert np.array_equal(_bits(f), _bits(g))
    if K - 16 < 16:
        with pytest.raises(ValueError):
            capi.lagforms_host(M, s, n, theta, 1.0, K - 16)
        return
    short = capi.lagforms_host(M, s, n, theta, 1.0, K - 16)
    assert np.array_equal(short["taps"][:, :K - 15], f["taps"][:, :K - 15])
    assert np.all(f["raw"][1] == short["raw"][0]), (f["raw"][1], short["raw"][0])


@pytest.mark.parametrize("d", [1, 2])
def test_the_baseline_and_the_wide_build_give_the_same_bits(d):
    _, M, s, n, _, theta = _setup(d, 0.25)
    base = {K: capi.lagforms_host(M, s, n, theta, 1.0, K, isa=0) for K in KS}
    for K in KS:
        assert np.all(np.isfinite(base[K]["raw"])) and base[K]["raw"][0, 0] > 0.0
    if not _has_wide(M, s, n, theta):
        with pytest.raises(ValueError):
            capi.lagforms_host(M, s, n, theta, 1.0, 48, isa=1)
        # the one build there is is the one an evaluation runs
        for K in KS:
            assert np.array_equal(_bits(base[K]), _bits(capi.lagforms_host(M, s, n, theta, 1.0, K)))
        return
    for K in KS:
        wide = capi.lagforms_host(M, s, n, theta, 1.0, K, isa=1)
        assert np.array_equal(_bits(base[K]), _bits(wide)), (K, base[K]["raw"], wide["raw"])
        assert np.array_equal(_bits(wide), _bits(capi.lagforms_host(M, s, n, theta, 1.0, K)))
    with pytest.raises(ValueError):
        capi.lagforms_host(M, s, n, theta, 1.0, 48, isa=2)
