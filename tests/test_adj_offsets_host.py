"""Where the reverse sweep's rows lie in the tile (smoothsde_amd/csrc/ssde_adj.hpp: adj_row_bytes, adj_row_offset, adj_window_span --
the arithmetic k_iso_adj.hip forms a row's buffer resource from), compiled by g++ into tests/hostsim and compared with Python's
integers.  A window over `rows` rows of C channels spans rows x C x 512 bytes whatever the number of tracks in its group; one
window per track is an ordinary plan, so the span passes 2^31 and 2^32 on long tracks (209 716 and 419 431 rows at C = 20).  The
kernel once formed the offset as a 32-bit int from one resource over the whole window: negative past 2^31, wrapped past 2^32 --
finite, wrong numbers and no fault.  There is no threshold in the present form (a resource per row, a 64-bit offset): what is
checked is that the product is the 64-bit one over the whole range of rows x C the engine accepts (ssde_create refuses a track of
more than INT32_MAX rows), and that what stays 32-bit -- a channel's offset within its row -- fits."""
import os
import re

import numpy as np
import pytest

import hostsim_lib

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smoothsde_amd", "csrc")
INT32_MAX = 2 ** 31 - 1
WAVE = 64
# channels of a tile row: from the narrowest reverse-sweep shape (regular grid, one response column, one streamed column) to the
# widest (a time stamp, two response columns, a 2 x 2 H_array, 18 streamed columns); 20 is the shape of the long-window GPU tests
CHANNELS = (2, 9, 20, 25)


def _rows_around(limit, C):
    """window lengths on both sides of a span of `limit` bytes"""
    r = limit // (C * WAVE * 8)
    return [r - 1, r, r + 1, r + 2]


CASES = sorted({(r, C) for C in CHANNELS for lim in (2 ** 31, 2 ** 32) for r in _rows_around(lim, C)} |
               {(INT32_MAX, C) for C in CHANNELS} | {(1, C) for C in CHANNELS} | {(430000, 20), (215000, 20), (209716, 20), (419431, 20)})


def _as_int32(v):
    return int(np.array([v & 0xFFFFFFFF], dtype=np.uint64).astype(np.uint32).view(np.int32)[0])


def test_the_cases_lie_on_both_sides_of_both_limits():
    for C in CHANNELS:
        spans = [r * C * WAVE * 8 for r, c in CASES if c == C]
        for lim in (2 ** 31, 2 ** 32):
            assert any(s < lim for s in spans) and any(s >= lim for s in spans), (C, lim)
            below = max(s for s in spans if s < lim)
            above = min(s for s in spans if s >= lim)
            assert above - below == C * WAVE * 8                   # adjacent window lengths: the limit falls between them
    assert 209716 * 20 * 512 >= 2 ** 31 > 209715 * 20 * 512 and 419431 * 20 * 512 >= 2 ** 32 > 419430 * 20 * 512


@pytest.mark.parametrize("rows,C", CASES)
def test_the_last_rows_address_is_the_64_bit_product(rows, C):
    lib = hostsim_lib.load()
    row_bytes = C * WAVE * 8
    assert lib.hostsim_adj_row_bytes(C) == row_bytes
    assert lib.hostsim_adj_window_span(rows, C) == rows * row_bytes
    for row in sorted(r for r in {0, 1, rows // 2, rows - 1} if 0 <= r < rows):
        assert lib.hostsim_adj_row_offset(row, C) == row * row_bytes, (row, C)
    # the last row ends where the window does, and a load's own 32-bit part -- channel x 512 + lane x 8 -- stays inside the row's records
    assert lib.hostsim_adj_row_offset(rows - 1, C) + lib.hostsim_adj_row_bytes(C) == lib.hostsim_adj_window_span(rows, C)
    assert ((C - 1) * WAVE + WAVE - 1) * 8 + 8 <= row_bytes < 2 ** 31
    # (what these cases are for: the 32-bit product is another number as soon as the last row's offset reaches 2^31)
    if (rows - 1) * row_bytes >= 2 ** 31:
        assert _as_int32((rows - 1) * row_bytes) != (rows - 1) * row_bytes


def test_nothing_overflows_at_the_widest_row_and_the_longest_track():
    lib = hostsim_lib.load()
    C = max(CHANNELS)
    assert lib.hostsim_adj_window_span(INT32_MAX, C) == INT32_MAX * C * 512 < 2 ** 63
    assert lib.hostsim_adj_row_offset(INT32_MAX - 1, C) == (INT32_MAX - 1) * C * 512


def test_the_kernel_addresses_its_rows_through_these_functions():
    with open(os.path.join(CSRC, "k_iso_adj.hip")) as f:
        src = f.read()
    buffer_form = src[src.index("#if ADJ_LOADS == 1"):src.index("#else", src.index("#if ADJ_LOADS == 1"))]
    assert re.search(r"make_buffer_rsrc\(\(void\*\)\(wbase \+ adj_row_offset\(s - s_begin, C\)\), 0, row_bytes,", buffer_form)
    assert re.search(r"const int row_bytes = \(int\)adj_row_bytes\(C\);", buffer_form)
    assert len(re.findall(r"make_buffer_rsrc", buffer_form)) == 1          # no second resource with an offset of its own
    assert re.search(r"raw_buffer_load_b64\(rsrc, voff\[i\], 0,", buffer_form)      # the scalar offset of every load is zero
    with open(os.path.join(CSRC, "ssde_device.hpp")) as f:
        assert int(re.search(r"constexpr int WAVE = (\d+);", f.read()).group(1)) == WAVE
