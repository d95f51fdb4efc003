// ssde_gain_feed.hpp -- the gain table of the lag-path head BY VALUE, in the launch's own argument block (iso_shared_wg_kernel,
// k_iso_shared.inc).  A short table -- the covariance transient is over after a handful of rows at the parameters a
// fit visits -- rides in the 4 KB argument block next to IsoArgs instead of going through a pinned slot and a copy of its own: the
// rows packed to the HEAD_GAIN_COLS columns any model writes (CTCRW 0-12, the scalar family fewer: the others are zero), the row count
// in front.  The engine packs (head_gain_pack), wave 0 of a workgroup expands into its LDS slab (head_gain_slab_at): exactly what
// stage_gain puts there from the copied table -- rows past the last one repeat it, the row stride in LDS stays GAIN_ROW, the unused
// columns are zero.  Host and device include this header, and so does the host test of the two (tests/gainfeed/).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "ssde_math.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SSDE_GF_HD __host__ __device__
#else
#define SSDE_GF_HD
#endif

namespace ssde {

constexpr int HEAD_GAIN_COLS = 13;       // columns of a table row that any model writes (build_gain_table)
constexpr int HEAD_GAIN_STRIDE = 16;     // doubles per row of the full table and of the LDS slab (== GAIN_ROW)
constexpr int HEAD_ARG_BLOCK = 4096;     // bytes of a launch's argument block

// rows that fit next to `other_args_bytes` of other arguments and the 8-byte row count
constexpr int head_gain_capacity(size_t other_args_bytes) {
    return (int)((HEAD_ARG_BLOCK - other_args_bytes - 8) / (HEAD_GAIN_COLS * sizeof(double)));
}

template <int ROWS>
struct HeadGainT {
    int32_t rows;                        // 0: the table was copied (IsoArgs.gain), nothing here is read
    int32_t pad_;
    double v[ROWS * HEAD_GAIN_COLS];     // [rows][HEAD_GAIN_COLS]
};

// table [rows][HEAD_GAIN_STRIDE] -> v [rows][HEAD_GAIN_COLS]; false (nothing written) when the table does not fit or a column past
// HEAD_GAIN_COLS is not zero (no model writes one: the expansion could not give it back)
inline bool head_gain_pack(const double* table, int rows, int capacity, double* v) {
    if (rows < 1 || rows > capacity) return false;
    for (int r = 0; r < rows; r++)
        for (int c = HEAD_GAIN_COLS; c < HEAD_GAIN_STRIDE; c++)
            if (table[r * HEAD_GAIN_STRIDE + c] != 0.0) return false;
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < HEAD_GAIN_COLS; c++) v[r * HEAD_GAIN_COLS + c] = table[r * HEAD_GAIN_STRIDE + c];
    return true;
}

// index into v of column c < HEAD_GAIN_COLS of table row `row`, under stage_gain's rule: rows past the last repeat it
SSDE_GF_HD inline int head_gain_index(int rows, int row, int c) {
    const int r = row < rows - 1 ? row : rows - 1;
    return r * HEAD_GAIN_COLS + c;
}
// element (row, c), c < HEAD_GAIN_STRIDE, of the table the packed rows stand for
// (the index stays inside the packed rows whatever c is: nothing is read past them)
SSDE_GF_HD inline double head_gain_slab_at(const double* v, int rows, int row, int c) {
    const double x = v[head_gain_index(rows, row, c < HEAD_GAIN_COLS ? c : HEAD_GAIN_COLS - 1)];
    return c < HEAD_GAIN_COLS ? x : 0.0;
}


// ---- how long the table is: the stationarity test of the covariance recursion, shared by the gain table (build_gain_table), the
// stationary gains of ssde_lagforms_host and the tests that choose parameters by the table's length.  In floating point the recursion
// ends in a last-bit limit cycle rather than a bitwise fixed point, so "settled" = every component moved by less than 2e-15
// relative; GAIN_SETTLED_ROWS such rows in a row end the recursion.
constexpr int GAIN_SETTLED_ROWS = 4;
inline bool gain_close(double a, double b) { return fabs(a - b) <= 2e-15 * (fabs(a) + fabs(b)) + 1e-300; }
inline bool ctcrw_cov_settled(const CtcrwCov<15>& C, const CtcrwCov<15>& prev) {
    bool same = gain_close(C.p11, prev.p11) && gain_close(C.p12, prev.p12) && gain_close(C.p22, prev.p22);
    for (int j = 0; j < NDIRP && same; j++)
        same = gain_close(C.d11[j], prev.d11[j]) && gain_close(C.d12[j], prev.d12[j]) && gain_close(C.d22[j], prev.d22[j]);
    return same;
}
// rows of the CTCRW table at these parameters (build_gain_table's loop without its outputs), at most tmax
template <int D>
inline int ctcrw_gain_rows(const CtcrwTrans& tr, double h, const double* p0, int tmax) {
    CtcrwCov<15> C;
    C.init(p0[0], p0[1], p0[2]);
    int last = 0, stable = 0;
    for (int t = 0; t < tmax; t++) {
        const CtcrwCov<15> prev = C;
        CtcrwGain G;
        ctcrw_cov_step<D, 15>(C, tr, h, false, G);
        last = t;
        stable = ctcrw_cov_settled(C, prev) ? stable + 1 : 0;
        if (stable >= GAIN_SETTLED_ROWS) break;
    }
    return last + 1;
}

}  // namespace ssde
