// k_path_occ.hip -- occupancy grids of posterior state paths for gfx950 (ssde_path_occupancy; math in ssde_occ.hpp over ssde_draws.hpp,
// definitions DESIGN.md §3.13).
//
// path_occ_kernel: the walk of smooth_draws_kernel (rec_draw_walk, ssde_records.hpp: lane = track, one wave per (group of 64 tracks,
// chunk of DRAW_CH draws)) with the n x sdim stores of every draw replaced by one integer add: the row's weight, a whole number of the
// call's quanta, into the cell of the drawn position.  Integer sums do not depend on the order of arrival, so the result is bitwise
// the same whatever ran where.  Two forms, one template (TILE):
//   TILE   a workgroup is OCC_NW waves on ONE group of 64 tracks whose lanes all feed one output grid; the waves take consecutive
//          chunks of draws (threadIdx.y), add into one zeroed LDS tile of nx * ny cells with LDS atomics and, after the walk, add the
//          tile's non-zero cells to the accumulator in HBM: consecutive lanes take consecutive cells, 512 contiguous bytes per wave
//          instruction.
//   global one wave per workgroup, as path_stats_kernel; every lane adds straight into its own grid's cell in HBM.
// A launch covers all groups of the chunk in one form; a workgroup whose group runs in the other form leaves at once (grp_of[g],
// uniform).  The weight that falls in no cell stays in a register of the lane and goes out in one add per lane at the end.  Per-row
// reads beside the records: the row's weight and, on a lattice-padded handle, its entry of the lattice row -> caller row map, as
// path_stats_kernel.  64-bit offsets throughout; every index into the accumulator is cell + nx * ny * group with cell < nx * ny from
// occ_cell and group < n_out_groups checked on the host.
#include "ssde_device.hpp"
#include "ssde_occ.hpp"

namespace ssde {

typedef unsigned long long occ_u64;
static_assert(sizeof(occ_u64) == sizeof(uint64_t), "accumulator cells");

template <int MODEL, int D, bool TILE>
__global__ __launch_bounds__(TILE ? WAVE * OCC_NW : WAVE) void path_occ_kernel(const OccArgs A) {
    typedef DenseDims<MODEL, D> DM;
    constexpr int SD = SmoothRec<MODEL, D>::SD;
    extern __shared__ occ_u64 occ_tile[];
    const int tile_grp = A.grp_of[A.d.s.rc.g0 + blockIdx.x];
    if ((tile_grp != OCC_GROUP_MIXED) != TILE) return;                // the other form's group (uniform: before any barrier)
    const int ncell = A.grid.nx * A.grid.ny;
    const int tid = threadIdx.x + WAVE * threadIdx.y;
    if (TILE) {
        for (int i = tid; i < ncell; i += WAVE * OCC_NW) occ_tile[i] = 0;
        __syncthreads();
    }
    const RecLane L = rec_lane(A.d.s);
    const int k0 = (blockIdx.y * (TILE ? OCC_NW : 1) + (TILE ? threadIdx.y : 0)) * DRAW_CH;
    const int64_t seg = L.has ? A.d.lane_trk[L.l] : 0;
    const int og = L.has ? A.lane_grp[L.l] : -1;                      // the lane's output grid, -1: it takes part in nothing
    occ_u64* const mine = A.acc + (int64_t)ncell * (og < 0 ? 0 : og);
    occ_u64 w = 0, w_out = 0;
    if (k0 < A.d.n_draws) {                                           // (a wave past the batch's last draw only keeps the barriers)
        rec_draw_walk<MODEL, D, DRAW_CH>(
            L, A.d.seed, (uint64_t)(A.d.track0 + seg), A.d.draw0 + (uint32_t)k0, A.d.col0,
            [&](int64_t row) {
                const int64_t crow = A.row_map ? A.row_map[row] : row;
                w = (crow < 0 || og < 0) ? 0 : (A.wq ? A.wq[crow] : A.unit);
            },
            [&](int q, const double (&al)[SD]) {
                if (w == 0 || k0 + q >= A.d.n_draws) return;
                double p[D];
#pragma unroll
                for (int c = 0; c < D; c++) p[c] = al[DM::z(c)];
                const int cell = occ_cell<D>(p, A.grid);
                if (cell < 0) w_out += w;
                else if (TILE) atomicAdd(&occ_tile[cell], w);
                else atomicAdd(&mine[cell], w);
            });
    }
    if (w_out) atomicAdd(&A.acc_out[og], w_out);                      // (w_out != 0 only where og >= 0)
    if (TILE) {
        __syncthreads();
        if (tile_grp < 0) return;
        occ_u64* const dst = A.acc + (int64_t)ncell * tile_grp;
        for (int i = tid; i < ncell; i += WAVE * OCC_NW) {
            const occ_u64 v = occ_tile[i];
            if (v) atomicAdd(&dst[i], v);
        }
    }
}

hipError_t launch_path_occ(const OccArgs& a, bool tile, hipStream_t s) {
    if (a.d.s.rc.n_groups == 0 || a.d.n_draws <= 0) return hipSuccess;
    const int64_t ncell = (int64_t)a.grid.nx * a.grid.ny;
    if (a.grid.nx < 1 || a.grid.ny < 1 || (tile && ncell > OCC_TILE_CELLS)) return hipErrorInvalidValue;
    const int per = tile ? OCC_NW * DRAW_CH : DRAW_CH;
    const dim3 grid((unsigned)a.d.s.rc.n_groups, (unsigned)((a.d.n_draws + per - 1) / per));
    if (grid.y > 65535u) return hipErrorInvalidValue;
#define SSDE_OK_(MODEL, D) \
    if (a.d.s.model == MODEL && a.d.s.d == D) { \
        if (tile) hipLaunchKernelGGL((path_occ_kernel<MODEL, D, true>), grid, dim3(WAVE, OCC_NW), (size_t)ncell * sizeof(occ_u64), s, a); \
        else hipLaunchKernelGGL((path_occ_kernel<MODEL, D, false>), grid, dim3(WAVE), 0, s, a); \
        return hipGetLastError(); \
    }
    SSDE_OK_(M_CTCRW, 1) SSDE_OK_(M_CTCRW, 2) SSDE_OK_(M_OU_SSM, 1) SSDE_OK_(M_OU_SSM, 2) SSDE_OK_(M_BM_SSM, 1) SSDE_OK_(M_BM_SSM, 2)
#undef SSDE_OK_
    return hipErrorInvalidValue;
}

}  // namespace ssde
