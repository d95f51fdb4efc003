// k_smooth_loo.hip -- leave-one-out residuals and predictive densities for gfx950 (ssde_smooth_loo; math in ssde_loo.hpp, definitions
// DESIGN.md §3.20).
//
// loo_back_kernel: smooth_back_kernel's walk (lane = track, one wave per group of 64 tracks, from the last record to the first) with
// smooth_back_row replaced by loo_back_row: the same r, N in registers, the deletion quantities of every row formed from their
// incoming values.  It reads the record doubles V, F^-1, K, T, E and the measured columns of A -- never P -- and stores straight to
// the long format, on served rows only (the outputs are preset to NaN).  The track's statistics stay in registers and leave once per
// lane after the walk: one lane owns each track, plain stores.  On a lattice-padded handle the row's entry of the lattice row ->
// caller row map is read per row, as path_speed_kernel does; a padded row is not served by construction (it is an NA row) and is
// kept out of every output and count all the same.  64-bit offsets throughout; every per-row store is at row + n_out * c with
// row = row0 + 1 + s < n_out (smooth_back_kernel's rows), every statistic at seg + n_trk * k with k < 4 + n_thr.
// k_smooth_loo_wide.hip compiles the same kernel with its loops kept as loops for five to eight columns.
#include "ssde_device.hpp"
#include "ssde_loo.hpp"

namespace ssde {

static_assert(LOO_NTHR * sizeof(double) == sizeof(LooArgs::thr), "threshold table");

template <int MODEL, int D>
__global__ __launch_bounds__(WAVE) void loo_back_kernel(const LooArgs A) {
    typedef SmoothRec<MODEL, D> RC;
    constexpr int SD = RC::SD;
    const RecLane L = rec_lane(A.s);
    double r[SD], N[SD][SD];
#pragma unroll
    for (int a = 0; a < SD; a++) {
        r[a] = 0.0;
#pragma unroll
        for (int b = 0; b < SD; b++) N[a][b] = 0.0;
    }
    LooAcc acc;
    loo_init(acc);
    const int64_t n = A.s.n_out;
    const int nthr = A.n_thr;
    for (int s = L.smax - 1; s >= 0; s--) {
        if (s >= L.ns) continue;
        const RecRow rec = L.row<RC::R>(s);
        LooRow<D> o;
        loo_back_row<MODEL, D, SD>(r, N, s == L.ns - 1, rec, o);
        const int64_t row = L.row0 + 1 + s;
        const int64_t crow = A.row_map ? A.row_map[row] : row;
        if (!o.served || crow < 0) continue;
        if (A.mean) {
#pragma unroll
            for (int i = 0; i < D; i++) A.mean[row + (int64_t)i * n] = o.mean[i];
        }
        if (A.cov) {
#pragma unroll
            for (int c = 0; c < D; c++)
#pragma unroll
                for (int q = 0; q < D; q++) A.cov[row + n * ((int64_t)q + (int64_t)D * c)] = o.cov[q][c];
        }
        if (!o.white) continue;
        if (A.resid) {
#pragma unroll
            for (int i = 0; i < D; i++) A.resid[row + (int64_t)i * n] = o.z[i];
        }
        if (A.lpd) A.lpd[row] = o.lpd;
        loo_fold(acc, o.q, o.lpd, crow, [&](int k) -> double { return A.thr[k]; }, nthr);
    }
    if (!A.stats || L.ns <= 0) return;                                // no state row: the preset values stay
    const int64_t seg = A.lane_trk[L.l];
    if (seg < 0 || seg >= A.n_trk) return;
    double st[LOO_NSTAT_MAX];
    loo_finish(acc, nthr, st);
    double* o = A.stats + seg;
#pragma unroll
    for (int k = 0; k < LOO_NSTAT_MAX; k++)
        if (k < 4 + nthr) o[A.n_trk * k] = st[k];
}

#define SSDE_LK(MODEL, D) \
    if (a.s.model == MODEL && a.s.d == D) { hipLaunchKernelGGL((loo_back_kernel<MODEL, D>), dim3(a.s.rc.n_groups), dim3(WAVE), 0, s, a); return hipGetLastError(); }

#ifndef SSDE_LOO_WIDE_TU
hipError_t launch_smooth_loo_wide(const LooArgs& a, hipStream_t s);

hipError_t launch_smooth_loo(const LooArgs& a, hipStream_t s) {
    if (a.s.rc.n_groups == 0) return hipSuccess;
    if (a.n_thr < 0 || a.n_thr > LOO_NTHR || (a.stats && !a.lane_trk)) return hipErrorInvalidValue;
    SSDE_LK(M_CTCRW, 1) SSDE_LK(M_CTCRW, 2) SSDE_LK(M_CTCRW, 3) SSDE_LK(M_CTCRW, 4)
    SSDE_LK(M_OU_SSM, 1) SSDE_LK(M_OU_SSM, 2) SSDE_LK(M_OU_SSM, 3) SSDE_LK(M_OU_SSM, 4)
    SSDE_LK(M_BM_SSM, 1) SSDE_LK(M_BM_SSM, 2) SSDE_LK(M_BM_SSM, 3) SSDE_LK(M_BM_SSM, 4)
    return launch_smooth_loo_wide(a, s);
}
#else
hipError_t launch_smooth_loo_wide(const LooArgs& a, hipStream_t s) {
    SSDE_LK(M_CTCRW, 5) SSDE_LK(M_CTCRW, 6) SSDE_LK(M_CTCRW, 7) SSDE_LK(M_CTCRW, 8)
    SSDE_LK(M_OU_SSM, 5) SSDE_LK(M_OU_SSM, 6) SSDE_LK(M_OU_SSM, 7) SSDE_LK(M_OU_SSM, 8)
    SSDE_LK(M_BM_SSM, 5) SSDE_LK(M_BM_SSM, 6) SSDE_LK(M_BM_SSM, 7) SSDE_LK(M_BM_SSM, 8)
    return hipErrorInvalidValue;
}
#endif
#undef SSDE_LK

}  // namespace ssde
