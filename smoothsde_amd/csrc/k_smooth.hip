// k_smooth.hip -- the fixed-interval smoother's kernels for gfx950 (ssde_smooth; math in ssde_smooth.hpp, definitions DESIGN.md §3.9).
//
// smooth_back_kernel: lane = track, one wave per group of 64 tracks, walking the records the forward pass wrote (dense_kernel in
// record mode, or smooth_tv_record_kernel below) from the last step to the first.  The records are time-major and lane-coalesced:
// every load of one record double is a 512-B wave load.  r and N stay in registers for d <= 4; k_smooth_wide.hip compiles the same
// kernel with its loops kept as loops for five to eight columns (scratch, the rare coverage path, as k_dense_wide.hip).
// Outputs go straight to the long format: lane l writes row row0_l + 1 + s, so a wave store touches 64 rows, but successive steps of
// a lane fill the same cache lines and the outputs are a third of the bytes moved (DESIGN.md §3.9 has the measurement).
#include "ssde_ahead.hpp"
#include "ssde_device.hpp"
#include "ssde_predict.hpp"
#include "ssde_smooth.hpp"

namespace ssde {

template <int MODEL, int D>
__global__ __launch_bounds__(WAVE) void smooth_back_kernel(const SmoothArgs A) {
    typedef SmoothRec<MODEL, D> RC;
    constexpr int SD = RC::SD;
    const RecLane L = rec_lane(A);
    double r[SD], N[SD][SD];
#pragma unroll
    for (int a = 0; a < SD; a++) {
        r[a] = 0.0;
#pragma unroll
        for (int b = 0; b < SD; b++) N[a][b] = 0.0;
    }
    const int64_t n = A.n_out;
    for (int s = L.smax - 1; s >= 0; s--) {
        if (s >= L.ns) continue;
        const RecRow rec = L.row<RC::R>(s);
        double am[SD], V[SD][SD];
        smooth_back_row<MODEL, D, SD>(r, N, s == L.ns - 1, rec, am, V);
        const int64_t row = L.row0 + 1 + s;
        if (A.am) {
#pragma unroll
            for (int c = 0; c < SD; c++) A.am[row + (int64_t)c * n] = am[c];
        }
        if (A.Vm) {
#pragma unroll
            for (int c = 0; c < SD; c++)
#pragma unroll
                for (int q = 0; q < SD; q++) A.Vm[row + n * ((int64_t)q + (int64_t)SD * c)] = V[q][c];
        }
        if (A.em) {
#pragma unroll
            for (int i = 0; i < D; i++) A.em[row + (int64_t)i * n] = rec(RC::E + i);
        }
    }
}

#ifndef SSDE_SMOOTH_WIDE_TU
// PATH_TV handles keep long-format rows (no tiles): lane = track of the length-sorted order, each lane reading its own rows (the
// route of a few long tracks -- once per fit, not a throughput path).  The row's linear predictors as k_tv.hip's pre-pass forms them.
template <int MODEL, int D>
__global__ __launch_bounds__(WAVE) void smooth_tv_record_kernel(const TvArgs T, const SmoothArgs A) {
    typedef DenseDims<MODEL, D> DM;
    typedef SmoothRec<MODEL, D> RC;
    constexpr int SD = DM::SD, Q = DM::Q;
    const int g = A.rc.g0 + blockIdx.x, lane = threadIdx.x;
    const int64_t trk = (int64_t)g * WAVE + lane;
    if (trk >= T.n_tracks) return;
    const int ns = T.trk_ns[trk];
    const int64_t row0 = T.trk_row0[trk];
    const int64_t goff = rec_group(A.rc, g);
    DenseLane<MODEL, D, 0> S;
    double a0[SD];
    for (int c = 0; c < SD; c++) a0[c] = T.a0[trk * SD + c];
    S.init(a0, T.p0f);
    const SlotTable* __restrict__ st = T.slots;
    for (int s = 0; s < ns; s++) {
        const int64_t i = row0 + 1 + s;
        const double dt = (i + 1 < T.n) ? T.times[i + 1] - T.times[i] : T.last_dt;
        double y[D];
#pragma unroll
        for (int a = 0; a < D; a++) y[a] = T.obs[i + (int64_t)a * T.n];
        DualN<0> H[D][D];
#pragma unroll
        for (int p = 0; p < D; p++)
#pragma unroll
            for (int q = 0; q < D; q++) H[p][q] = DualN<0>(T.has_h ? T.h_array[i * (D * D) + p + q * D] : (p == q ? T.h : 0.0));
        DualN<0> par[Q];
#pragma unroll
        for (int j = 0; j < Q; j++) par[j] = DualN<0>(0.0);
        for (int k = 0; k < T.n_slots; k++) {
            const int col = st->col[k], j = st->par_j[k];
            const double t = ((col >= 0) ? T.colbuf[(int64_t)col * T.col_stride + i] : 1.0) * T.par[st->pidx[k]];
#pragma unroll
            for (int jj = 0; jj < Q; jj++) par[jj].v += (j == jj) ? t : 0.0;
        }
        const bool na = is_na(y[0], T.any_nan);
        const bool upd = smooth_record_row<MODEL, D>(S, par, H, dt, y, na, rec_row<RC::R>(A.rc, goff, lane, s));
        if (A.rc.side && A.rc.side_kind == REC_SIDE_AHEAD)                       // ssde_forecast_scores: what a step through the row and a score at it need
            ahead_side_row<MODEL, D>(par, H, dt, y, na, rec_side_row<RC::R, AheadSide<MODEL, D>::SW>(A.rc, goff, lane, s));
        else if (A.rc.side)                                                      // ssde_predict: the row's linear predictors and interval
            predict_side_row<MODEL, D>(par, dt, na, upd, rec_side_row<RC::R, PredictPk<MODEL, D>::SW>(A.rc, goff, lane, s));
        dense_step<MODEL, D, 0>(S, par, H, dt, y, na);
    }
}
#endif

#define SSDE_SB(MODEL, D) \
    if (a.model == MODEL && a.d == D) { hipLaunchKernelGGL((smooth_back_kernel<MODEL, D>), dim3(a.rc.n_groups), dim3(WAVE), 0, s, a); return hipGetLastError(); }
#define SSDE_SR(MODEL, D) if (model == MODEL && d == D) return SmoothRec<MODEL, D>::R;

#ifndef SSDE_SMOOTH_WIDE_TU
hipError_t launch_smooth_back_wide(const SmoothArgs& a, hipStream_t s);
int smooth_rec_doubles_wide(int model, int d);

int smooth_rec_doubles(int model, int d) {
    SSDE_SR(M_CTCRW, 1) SSDE_SR(M_CTCRW, 2) SSDE_SR(M_CTCRW, 3) SSDE_SR(M_CTCRW, 4)
    SSDE_SR(M_OU_SSM, 1) SSDE_SR(M_OU_SSM, 2) SSDE_SR(M_OU_SSM, 3) SSDE_SR(M_OU_SSM, 4)
    SSDE_SR(M_BM_SSM, 1) SSDE_SR(M_BM_SSM, 2) SSDE_SR(M_BM_SSM, 3) SSDE_SR(M_BM_SSM, 4)
    return smooth_rec_doubles_wide(model, d);
}

hipError_t launch_smooth_back(const SmoothArgs& a, hipStream_t s) {
    if (a.rc.n_groups == 0) return hipSuccess;
    SSDE_SB(M_CTCRW, 1) SSDE_SB(M_CTCRW, 2) SSDE_SB(M_CTCRW, 3) SSDE_SB(M_CTCRW, 4)
    SSDE_SB(M_OU_SSM, 1) SSDE_SB(M_OU_SSM, 2) SSDE_SB(M_OU_SSM, 3) SSDE_SB(M_OU_SSM, 4)
    SSDE_SB(M_BM_SSM, 1) SSDE_SB(M_BM_SSM, 2) SSDE_SB(M_BM_SSM, 3) SSDE_SB(M_BM_SSM, 4)
    return launch_smooth_back_wide(a, s);
}

hipError_t launch_smooth_tv_record(const TvArgs& t, const SmoothArgs& a, hipStream_t s) {
    if (a.rc.n_groups == 0) return hipSuccess;
#define SSDE_TR(MODEL, D) \
    if (a.model == MODEL && a.d == D) { hipLaunchKernelGGL((smooth_tv_record_kernel<MODEL, D>), dim3(a.rc.n_groups), dim3(WAVE), 0, s, t, a); return hipGetLastError(); }
    SSDE_TR(M_CTCRW, 1) SSDE_TR(M_CTCRW, 2) SSDE_TR(M_OU_SSM, 1) SSDE_TR(M_OU_SSM, 2) SSDE_TR(M_BM_SSM, 1) SSDE_TR(M_BM_SSM, 2)
#undef SSDE_TR
    return hipErrorInvalidValue;
}
#else
int smooth_rec_doubles_wide(int model, int d) {
    SSDE_SR(M_CTCRW, 5) SSDE_SR(M_CTCRW, 6) SSDE_SR(M_CTCRW, 7) SSDE_SR(M_CTCRW, 8)
    SSDE_SR(M_OU_SSM, 5) SSDE_SR(M_OU_SSM, 6) SSDE_SR(M_OU_SSM, 7) SSDE_SR(M_OU_SSM, 8)
    SSDE_SR(M_BM_SSM, 5) SSDE_SR(M_BM_SSM, 6) SSDE_SR(M_BM_SSM, 7) SSDE_SR(M_BM_SSM, 8)
    return 0;
}

hipError_t launch_smooth_back_wide(const SmoothArgs& a, hipStream_t s) {
    SSDE_SB(M_CTCRW, 5) SSDE_SB(M_CTCRW, 6) SSDE_SB(M_CTCRW, 7) SSDE_SB(M_CTCRW, 8)
    SSDE_SB(M_OU_SSM, 5) SSDE_SB(M_OU_SSM, 6) SSDE_SB(M_OU_SSM, 7) SSDE_SB(M_OU_SSM, 8)
    SSDE_SB(M_BM_SSM, 5) SSDE_SB(M_BM_SSM, 6) SSDE_SB(M_BM_SSM, 7) SSDE_SB(M_BM_SSM, 8)
    return hipErrorInvalidValue;
}
#endif
#undef SSDE_SB
#undef SSDE_SR

}  // namespace ssde
