// k_path_stats.hip -- summaries of posterior state paths for gfx950 (ssde_path_stats; math in ssde_path.hpp over ssde_draws.hpp,
// definitions DESIGN.md §3.12).
//
// path_stats_kernel: the walk of smooth_draws_kernel (rec_draw_walk, ssde_records.hpp: lane = track, one wave per (group of 64 tracks,
// chunk of DRAW_CH draws)) with the n x sdim stores of every draw replaced by path_step: the length, the end positions and the region
// sums of each (lane, draw) stay in registers, and after the walk the lane stores n_stat numbers per draw at its track's ordinal.  One wave owns each (track, draw): plain stores, no atomics, a deterministic result.  The only per-row reads
// beside the records are the row's weight and, on a lattice-padded handle, its entry of the lattice row -> caller row map: per-lane
// addresses, but a lane's successive rows share lines.  64-bit offsets throughout.
#include "ssde_device.hpp"
#include "ssde_path.hpp"

namespace ssde {

static_assert(PATH_NREG * 4 * sizeof(double) == sizeof(PathArgs::regions), "region table");

template <int MODEL, int D>
__global__ __launch_bounds__(WAVE) void path_stats_kernel(const PathArgs A) {
    constexpr int SD = SmoothRec<MODEL, D>::SD;
    const RecLane L = rec_lane(A.d.s);
    const int k0 = blockIdx.y * DRAW_CH;
    const int64_t seg = L.has ? A.d.lane_trk[L.l] : 0;
    PathAcc<D> acc[DRAW_CH];
#pragma unroll
    for (int q = 0; q < DRAW_CH; q++) path_init<D>(acc[q]);
    const int nreg = A.n_regions;
    bool is_row = false;
    double w = 1.0;
    rec_draw_walk<MODEL, D, DRAW_CH>(
        L, A.d.seed, (uint64_t)(A.d.track0 + seg), A.d.draw0 + (uint32_t)k0, A.d.col0,
        [&](int64_t row) {
            const int64_t crow = A.row_map ? A.row_map[row] : row;
            is_row = crow >= 0;
            w = (is_row && A.weight) ? A.weight[crow] : 1.0;
        },
        [&](int q, const double (&al)[SD]) {
            path_step<MODEL, D, SD>(acc[q], al, is_row, w, [&](int k) -> double { return A.regions[k]; }, nreg);
        });
    if (L.ns <= 0) return;                                            // no state row: the preset NaN stays
    const int nstat = 2 + nreg;
#pragma unroll
    for (int q = 0; q < DRAW_CH; q++) {
        if (k0 + q >= A.d.n_draws) continue;
        double st[PATH_NSTAT_MAX];
        path_finish<D>(acc[q], nreg, st);
        double* o = A.stats + seg + A.n_trk * ((int64_t)nstat * (k0 + q));
#pragma unroll
        for (int k = 0; k < PATH_NSTAT_MAX; k++)
            if (k < nstat) o[A.n_trk * k] = st[k];
    }
}

__global__ void path_row_map_kernel(const int64_t* pos, int64_t n, int64_t* map) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) map[pos[i]] = i;
}

hipError_t launch_path_row_map(const int64_t* pos, int64_t n, int64_t np, int64_t* map, hipStream_t s) {
    if (np <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(map, 0xff, (size_t)np * 8, s);    // -1
    if (e != hipSuccess || n <= 0) return e;
    hipLaunchKernelGGL(path_row_map_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pos, n, map);
    return hipGetLastError();
}

hipError_t launch_path_stats(const PathArgs& a, hipStream_t s) {
    if (a.d.s.rc.n_groups == 0 || a.d.n_draws <= 0) return hipSuccess;
    if (a.n_regions < 0 || a.n_regions > PATH_NREG) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.d.s.rc.n_groups, (unsigned)((a.d.n_draws + DRAW_CH - 1) / DRAW_CH));
    if (grid.y > 65535u) return hipErrorInvalidValue;
#define SSDE_PK(MODEL, D) \
    if (a.d.s.model == MODEL && a.d.s.d == D) { hipLaunchKernelGGL((path_stats_kernel<MODEL, D>), grid, dim3(WAVE), 0, s, a); return hipGetLastError(); }
    SSDE_PK(M_CTCRW, 1) SSDE_PK(M_CTCRW, 2) SSDE_PK(M_OU_SSM, 1) SSDE_PK(M_OU_SSM, 2) SSDE_PK(M_BM_SSM, 1) SSDE_PK(M_BM_SSM, 2)
#undef SSDE_PK
    return hipErrorInvalidValue;
}

}  // namespace ssde
