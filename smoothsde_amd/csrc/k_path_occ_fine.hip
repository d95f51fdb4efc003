// k_path_occ_fine.hip -- occupancy grids of posterior state paths refined between the rows, for gfx950 (ssde_path_occupancy_fine;
// math in ssde_bridge.hpp and ssde_occ.hpp, definitions DESIGN.md §3.15).
//
// predict_draws_walk_kernel (k_predict_draws.hip, unchanged) has left, for every state row that places weight (a slot), the draw's
// state at the row and at the next row (the ends, per draw) and the row's linear predictors and interval (the side packet, per slot),
// all slot-minor.  path_occ_fine_kernel: a workgroup of OCC_FINE_TB threads owns ONE wavefront group's slots of the chunk (the plan
// gives a group's lanes consecutive slots) and OCC_FINE_DRAWS draws of the batch; its threads stride over (slot, draw) with slots
// fastest, so a wave's loads of one packet double are consecutive, as in predict_draws_query_kernel.  A thread reads the side packet,
// its two ends and the slot's m, own and share; adds `own` at the cell of the left end; and, where share != 0 and m > 1, chains the
// m - 1 inner points with bridge_slot_walk at the offsets ((r + 1) * dt) / m and adds `share` at each one's cell.  A rank that the
// walk does not emit (the row rejected its update, a NaN end) sends its share outside.
// THREADS OF A WAVE WITH DIFFERENT m DIVERGE: the chain of a slot is sequential by definition and a lane with m = 1 waits for the
// lane with m = 5 next to it.  That is accepted, as the long forecasts of predict_draws_query_kernel are: irregular grids differ in
// m by small factors, and the waves of other slots and draws fill the SIMD.
// Accumulation is path_occ_kernel's.  TILE: the group's lanes all feed one output grid; one zeroed LDS tile of nx * ny u64 cells,
// LDS atomics, and after a barrier the non-zero cells go to HBM with consecutive lanes on consecutive cells.  global: every add goes
// straight to its grid's cell in HBM.  A launch covers the chunk's groups in one form and a workgroup of the other form's group
// leaves at once (grp_of[g], uniform).  The quanta outside every cell stay in one register per thread and leave in one add (in the
// global form one add per run of slots with the same output grid).  Only vector atomics on unsigned long long; 64-bit offsets; every
// index into the accumulator is cell + nx * ny * group with cell < nx * ny from occ_cell and group < n_out_groups checked on the
// host; every slot index is inside [slot0, slot0 + pk_stride) because the group's slots are a sub-range of the chunk's.
#include "ssde_device.hpp"
#include "ssde_bridge.hpp"
#include "ssde_occ.hpp"

namespace ssde {

typedef unsigned long long occ_u64;

template <int MODEL, int D, bool TILE>
__global__ __launch_bounds__(OCC_FINE_TB) void path_occ_fine_kernel(const OccFineArgs A) {
    typedef BridgePk<MODEL, D> BK;
    typedef DenseDims<MODEL, D> DM;
    constexpr int SD = BK::SD, Q = BK::Q;
    extern __shared__ occ_u64 occ_fine_tile[];
    const int g = A.p.d.s.rc.g0 + blockIdx.x;
    const int tile_grp = A.grp_of[g];
    if ((tile_grp != OCC_GROUP_MIXED) != TILE) return;                // the other form's group (uniform: before any barrier)
    if (TILE && tile_grp < 0) return;                                 // none of the group's lanes takes part: it has no slot
    const int ncell = A.grid.nx * A.grid.ny;
    const int tid = threadIdx.x;
    if (TILE) {
        for (int i = tid; i < ncell; i += OCC_FINE_TB) occ_fine_tile[i] = 0;
        __syncthreads();
    }
    const int64_t nl = A.p.d.s.n_lanes;
    const int64_t l0 = min((int64_t)g * WAVE, nl), l1 = min((int64_t)(g + 1) * WAVE, nl);
    const int64_t s_lo = A.p.want_off[l0], n_sl = A.p.want_off[l1] - s_lo, stride = A.p.pk_stride;
    const int q_lo = blockIdx.y * OCC_FINE_DRAWS;
    const int nq = min(OCC_FINE_DRAWS, A.p.d.n_draws - q_lo);
    const int64_t total = n_sl * (int64_t)(nq > 0 ? nq : 0);
    occ_u64 w_out = 0;
    int og_out = -1;                                                  // the output grid w_out belongs to
    for (int64_t t = tid; t < total; t += OCC_FINE_TB) {
        const int64_t slot = s_lo + t % n_sl, i = slot - A.p.slot0;
        const int q = q_lo + (int)(t / n_sl);
        const occ_u64 own = A.own[slot], share = A.share[slot];
        const int m = A.m[slot];
        if (own == 0 && (share == 0 || m <= 1)) continue;
        const int64_t lane = A.p.slot_lane[slot];
        const int og = TILE ? tile_grp : A.lane_grp[lane];
        if (og < 0) continue;                                          // (the plan gives such a lane no slot)
        if (og != og_out) {
            if (w_out) atomicAdd(&A.acc_out[og_out], w_out);
            w_out = 0; og_out = og;
        }
        occ_u64* const mine = A.acc + (int64_t)ncell * og;
        auto add = [&](const double (&x)[SD], occ_u64 w) {
            double p[D];
#pragma unroll
            for (int c = 0; c < D; c++) p[c] = x[DM::z(c)];
            const int cell = occ_cell<D>(p, A.grid);
            if (cell < 0) w_out += w;
            else if (TILE) atomicAdd(&occ_fine_tile[cell], w);
            else atomicAdd(&mine[cell], w);
        };
        const double* sp = A.p.sidepk + i;
        const double* e = A.p.ends + (int64_t)q * BK::EZ * stride + i;
        const double dt = sp[(int64_t)BK::DT * stride];
        double left[SD], right[SD];
#pragma unroll
        for (int c = 0; c < SD; c++) left[c] = e[(int64_t)(BK::L + c) * stride];
        if (own) add(left, own);
        if (share == 0 || m <= 1) continue;
#pragma unroll
        for (int c = 0; c < SD; c++) right[c] = dt < 0.0 ? 0.0 : e[(int64_t)(BK::R + c) * stride];   // (a tail has no right end)
        DualN<0> par[Q];
#pragma unroll
        for (int j = 0; j < Q; j++) par[j] = DualN<0>(sp[(int64_t)(BK::PAR + j) * stride]);
        const uint64_t trk = (uint64_t)(A.p.d.track0 + A.p.d.lane_trk[lane]);
        const uint32_t s = (uint32_t)A.p.want_step[slot], draw = A.p.d.draw0 + (uint32_t)q;
        const double dm = (double)m;
        int emitted = 0;
        bridge_slot_walk<MODEL, D>(
            par, dt, left, right, (int64_t)(m - 1), [&](int64_t r) -> double { return ((double)(r + 1) * dt) / dm; },
            [&](int64_t r, double (&z)[SD]) { bridge_deviates<SD>(A.p.d.seed, trk, s, (uint32_t)r, draw, A.p.d.col0, z); },
            [&](int64_t, const double (&x)[SD]) { emitted++; add(x, share); });
        w_out += share * (occ_u64)(m - 1 - emitted);
    }
    if (w_out) atomicAdd(&A.acc_out[og_out], w_out);                  // (w_out != 0 only after og_out >= 0 was set)
    if (TILE) {
        __syncthreads();
        occ_u64* const dst = A.acc + (int64_t)ncell * tile_grp;
        for (int i = tid; i < ncell; i += OCC_FINE_TB) {
            const occ_u64 v = occ_fine_tile[i];
            if (v) atomicAdd(&dst[i], v);
        }
    }
}

hipError_t launch_path_occ_fine(const OccFineArgs& a, bool tile, hipStream_t s) {
    if (a.p.d.s.rc.n_groups == 0 || a.p.d.n_draws <= 0 || a.p.pk_stride <= 0) return hipSuccess;
    const int64_t ncell = (int64_t)a.grid.nx * a.grid.ny;
    if (a.grid.nx < 1 || a.grid.ny < 1 || (tile && ncell > OCC_TILE_CELLS)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.p.d.s.rc.n_groups, (unsigned)((a.p.d.n_draws + OCC_FINE_DRAWS - 1) / OCC_FINE_DRAWS));
    if (grid.y > 65535u) return hipErrorInvalidValue;
#define SSDE_OF_(MODEL, D) \
    if (a.p.d.s.model == MODEL && a.p.d.s.d == D) { \
        if (tile) hipLaunchKernelGGL((path_occ_fine_kernel<MODEL, D, true>), grid, dim3(OCC_FINE_TB), (size_t)ncell * sizeof(occ_u64), s, a); \
        else hipLaunchKernelGGL((path_occ_fine_kernel<MODEL, D, false>), grid, dim3(OCC_FINE_TB), 0, s, a); \
        return hipGetLastError(); \
    }
    SSDE_OF_(M_CTCRW, 1) SSDE_OF_(M_CTCRW, 2) SSDE_OF_(M_OU_SSM, 1) SSDE_OF_(M_OU_SSM, 2) SSDE_OF_(M_BM_SSM, 1) SSDE_OF_(M_BM_SSM, 2)
#undef SSDE_OF_
    return hipErrorInvalidValue;
}

}  // namespace ssde
