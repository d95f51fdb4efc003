// k_smooth_draws.hip -- joint posterior draws of the state path for gfx950 (ssde_smooth_draws; math in ssde_draws.hpp, definitions
// DESIGN.md §3.10).
//
// smooth_draws_kernel: lane = track, one wave per (group of 64 tracks, chunk of DRAW_CH draws), walking the records the smoother's
// forward pass wrote from the last step to the first (rec_draw_walk, ssde_records.hpp).  The row's factors (J, the Cholesky factor of C, a_f - J a_{j+1}) are formed once per step and
// applied to the chunk's DRAW_CH paths, which stay in registers with the hand-over of row j + 1; nothing but the records is read and
// nothing but the draws is written.  Draws are independent given the records, so the chunks are the grid's second dimension: a batch
// of 10^4 tracks fills 157 waves per chunk.  Outputs go straight to the long format, 64-bit offsets throughout.
#include "ssde_device.hpp"
#include "ssde_draws.hpp"

namespace ssde {

template <int MODEL, int D>
__global__ __launch_bounds__(WAVE) void smooth_draws_kernel(const DrawArgs A) {
    constexpr int SD = SmoothRec<MODEL, D>::SD;
    const RecLane L = rec_lane(A.s);
    const int k0 = blockIdx.y * DRAW_CH;
    const uint64_t trk = L.has ? (uint64_t)(A.track0 + A.lane_trk[L.l]) : 0;
    const int64_t n = A.s.n_out;
    int64_t row = 0;
    rec_draw_walk<MODEL, D, DRAW_CH>(
        L, A.seed, trk, A.draw0 + (uint32_t)k0, A.col0, [&](int64_t i) { row = i; },
        [&](int q, const double (&al)[SD]) {
            if (k0 + q < A.n_draws) {
                double* o = A.out + (int64_t)(k0 + q) * A.draw_stride + row;
#pragma unroll
                for (int c = 0; c < SD; c++) o[(int64_t)c * n] = al[c];
            }
        });
}

hipError_t launch_smooth_draws(const DrawArgs& a, hipStream_t s) {
    if (a.s.rc.n_groups == 0 || a.n_draws <= 0) return hipSuccess;
    const dim3 grid((unsigned)a.s.rc.n_groups, (unsigned)((a.n_draws + DRAW_CH - 1) / DRAW_CH));
    if (grid.y > 65535u) return hipErrorInvalidValue;
#define SSDE_DK(MODEL, D) \
    if (a.s.model == MODEL && a.s.d == D) { hipLaunchKernelGGL((smooth_draws_kernel<MODEL, D>), grid, dim3(WAVE), 0, s, a); return hipGetLastError(); }
    SSDE_DK(M_CTCRW, 1) SSDE_DK(M_CTCRW, 2) SSDE_DK(M_OU_SSM, 1) SSDE_DK(M_OU_SSM, 2) SSDE_DK(M_BM_SSM, 1) SSDE_DK(M_BM_SSM, 2)
#undef SSDE_DK
    return hipErrorInvalidValue;
}

}  // namespace ssde
