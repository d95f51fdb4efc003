// k_smooth_draws.hip -- joint posterior draws of the state path for gfx950 (ssde_smooth_draws; math in ssde_draws.hpp, definitions
// DESIGN.md §3.10).
//
// smooth_draws_kernel: lane = track, one wave per (group of 64 tracks, chunk of DRAW_CH draws), walking the records the smoother's
// forward pass wrote from the last step to the first, as smooth_back_kernel does (time-major, lane-coalesced: every load of one
// record double is a 512-B wave load).  The row's factors (J, the Cholesky factor of C, a_f - J a_{j+1}) are formed once per step and
// applied to the chunk's DRAW_CH paths, which stay in registers with the hand-over of row j + 1; nothing but the records is read and
// nothing but the draws is written.  Draws are independent given the records, so the chunks are the grid's second dimension: a batch
// of 10^4 tracks fills 157 waves per chunk.  Outputs go straight to the long format, 64-bit offsets throughout.
#include "ssde_device.hpp"
#include "ssde_draws.hpp"

namespace ssde {

template <int MODEL, int D>
__global__ __launch_bounds__(WAVE) void smooth_draws_kernel(const DrawArgs A) {
    typedef SmoothRec<MODEL, D> RC;
    typedef DrawFac<MODEL, D> FC;
    constexpr int SD = RC::SD;
    const int g = A.s.g0 + blockIdx.x, lane = threadIdx.x;
    const int k0 = blockIdx.y * DRAW_CH;
    const int64_t l = (int64_t)g * WAVE + lane;
    const bool has = l < A.s.n_lanes;
    const int ns = has ? A.s.lane_ns[l] : 0;
    const int64_t row0 = has ? A.s.lane_row0[l] : 0;
    const uint64_t trk = has ? (uint64_t)(A.track0 + A.lane_trk[l]) : 0;
    int smax = ns;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) smax = max(smax, __shfl_xor(smax, o, 64));
    smax = __builtin_amdgcn_readfirstlane(smax);
    const double* base = A.s.rec + (A.s.rec_off[g] - A.s.rec_base) + lane;
    double al[DRAW_CH][SD];
#pragma unroll
    for (int q = 0; q < DRAW_CH; q++)
#pragma unroll
        for (int c = 0; c < SD; c++) al[q][c] = 0.0;
    DrawNext<SD> nx;
#pragma unroll
    for (int r = 0; r < SD; r++) {
        nx.a[r] = 0.0; nx.id[r] = 0.0;
#pragma unroll
        for (int c = 0; c < SD; c++) nx.Lp[r][c] = 0.0;
    }
    const int64_t n = A.s.n_out;
    for (int s = smax - 1; s >= 0; s--) {
        if (s >= ns) continue;
        const double* rp = base + (int64_t)s * RC::R * WAVE;
        const bool tail = s == ns - 1;
        double fac[FC::R];
        draw_factor_row<MODEL, D, SD>([&](int k) -> double { return rp[(int64_t)k * WAVE]; }, tail, nx,
                                      [&](int k) -> double& { return fac[k]; });
        const int64_t row = row0 + 1 + s;
#pragma unroll
        for (int q = 0; q < DRAW_CH; q++) {
            double z[SD];
            draw_deviates<SD>(A.seed, trk, (uint32_t)s, A.draw0 + (uint32_t)(k0 + q), A.col0, z);
            draw_step<MODEL, D, SD>([&](int k) -> double { return fac[k]; }, tail, al[q], z);
            if (k0 + q < A.n_draws) {
                double* o = A.out + (int64_t)(k0 + q) * A.draw_stride + row;
#pragma unroll
                for (int c = 0; c < SD; c++) o[(int64_t)c * n] = al[q][c];
            }
        }
    }
}

hipError_t launch_smooth_draws(const DrawArgs& a, hipStream_t s) {
    if (a.s.n_groups == 0 || a.n_draws <= 0) return hipSuccess;
    const dim3 grid((unsigned)a.s.n_groups, (unsigned)((a.n_draws + DRAW_CH - 1) / DRAW_CH));
    if (grid.y > 65535u) return hipErrorInvalidValue;
#define SSDE_DK(MODEL, D) \
    if (a.s.model == MODEL && a.s.d == D) { hipLaunchKernelGGL((smooth_draws_kernel<MODEL, D>), grid, dim3(WAVE), 0, s, a); return hipGetLastError(); }
    SSDE_DK(M_CTCRW, 1) SSDE_DK(M_CTCRW, 2) SSDE_DK(M_OU_SSM, 1) SSDE_DK(M_OU_SSM, 2) SSDE_DK(M_BM_SSM, 1) SSDE_DK(M_BM_SSM, 2)
#undef SSDE_DK
    return hipErrorInvalidValue;
}

}  // namespace ssde
