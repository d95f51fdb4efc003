// k_iso_shared_cut.hip -- the head of the lag-statistics path when the bulk is cut at the transient's end (DESIGN.md §3.3d;
// ssde_windows.hpp: head_early_cut): the streamed rows are window 0 alone, [0, cut) of every track, and the waves of a workgroup are
// its DIRECTION PARTS.  CTCRW only.
//
// In SharedCtcrw::step_stat and ctcrw_mean_step every covariance direction j owns its state (tx[j], tv[j]) and its accumulator
// (sacc[j] / gq[j]) and reads only the value chain (x, v, u, su2); mu's direction likewise (mx, mv, macc / gmu).  A wave that walks
// the value chain and ONE direction performs, for that direction, the source operations of the wave that carries them all, in the
// same order, and issues well under half of its instructions.  That the BITS are the same is tested, not guaranteed: the table rows'
// step (ctcrw_mean_step) leaves its contractions to the compiler, which chooses per instantiation.  With two response coordinates
// value, gradient and check are bitwise the single wave's on every batch of tests/test_gpu_head_cut.py; with ONE the value was not
// (4 ulp on a one-track batch, with the step as it is and with every multiply-add of it an explicit fma alike; cause not found), so
// this entry exists for d = 2 only and the engine launches it for d = 2 only.  Workgroup b owns group b (padded to eight, the
// padding workgroups leave whole); wave p runs the lane code of k_iso_shared.inc instantiated for cut_part_mask(MASK, p): one
// covariance direction each, mu with the lightest (ssde_device.hpp).  Each wave leaves its wave sums in LDS; after ONE barrier
// wave 0 SELECTS every accumulator from the wave that owns it (the value from part 0) and sends the group's record out as
// iso_shared_wg_kernel does: to the host's mailbox for the synchronous single-device call, to partials (chk[g] = 0: one window has
// no hand-over) for a finalize launch otherwise.  The record is bitwise that of the single wave of iso_shared_kernel on the same
// window, so the reductions are untouched.
#define SSDE_SHARED_HAS_P2 1
#include "k_iso_shared.inc"

namespace ssde {

template <int MODEL, int D, int MASK, bool DEEP>
__global__ __launch_bounds__(WG_WAVES * WAVE, 1) void iso_shared_cut_kernel(const IsoArgs A, const HeadGain GV) {
    constexpr int NACC = 4 + D, NP = cut_n_parts(MASK);
    constexpr int M0 = cut_part_mask(MASK, 0), M1 = cut_part_mask(MASK, 1), M2 = cut_part_mask(MASK, 2);
    static_assert(NP >= 1 && NP <= 3 && NP <= WG_WAVES, "one wave per direction part");
    // (a part's gain slab is the static LDS of ITS instantiation of run_segment: the parts must be different lane types)
    static_assert((NP < 2 || M0 != M1) && (NP < 3 || (M0 != M2 && M1 != M2)), "direction parts: distinct masks");
    static_assert((M0 | (NP > 1 ? M1 : 0) | (NP > 2 ? M2 : 0)) == MASK, "direction parts: every direction has an owner");
    static_assert(NACC <= MBX_CHK && NACC < WAVE, "a group's record is one store of wave 0");
    static_assert(sizeof(double) * (WG_WAVES * NACC + 3 * GAIN_SLAB_ROWS * GAIN_ROW) <= 160 * 1024, "static LDS of a workgroup: the sums and one gain slab per part");
    __shared__ double wsum[WG_WAVES][NACC];
    if (blockIdx.x == 0 && threadIdx.x == 0 && A.chk_out && !A.mbx) *A.chk_out = 0.0;       // raised by the finalize launch
    const int g = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (g >= A.tv.n_groups) return;                            // (the whole workgroup: nobody is left at the barrier)
    const long long wc0 = A.wave_clock ? wall_clock64() : 0;
    double end[shared_nstate(2 * D, MASK, true)], acc[NACC];   // (end: one window hands nothing over; never written)
    int rows = 0;
#pragma unroll
    for (int k = 0; k < NACC; k++) acc[k] = 0.0;
    if (w == 0) rows = run_lane_shared<MODEL, D, M0, false, DEEP, true>(A, g, 0, 0, nullptr, end, acc, &GV);
    if constexpr (NP > 1) { if (w == 1) rows = run_lane_shared<MODEL, D, M1, false, DEEP, true>(A, g, 0, 0, nullptr, end, acc, &GV); }
    if constexpr (NP > 2) { if (w == 2) rows = run_lane_shared<MODEL, D, M2, false, DEEP, true>(A, g, 0, 0, nullptr, end, acc, &GV); }
    if (w < NP) {
#pragma unroll
        for (int k = 0; k < NACC; k++) {
            const double t = wave_sum(acc[k]);
            if (lane == 0) wsum[w][k] = t;
        }
    }
    __syncthreads();
    if (w == 0) {
        // accumulator k: [value | sigma_obs | mu_1 .. mu_D | par D | par D + 1] -- from the part that owns its direction
        const int k = lane < NACC ? lane : 0;
        const int owner = k == 0 ? 0 : k == 1 ? cut_part_of(MASK, DIR_SIG) : k < 2 + D ? cut_part_of(MASK, DIR_MU)
                        : k == 2 + D ? cut_part_of(MASK, DIR_P1) : cut_part_of(MASK, DIR_P2);
        const bool sum_lane = lane < NACC;
        const double v = sum_lane ? wsum[owner][k] : 0.0;
        if (A.mbx) {
            double* o = A.mbx + (int64_t)g * MBX_STRIDE;
            if (sum_lane || lane == MBX_CHK) __hip_atomic_store(o + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the record has left before its sequence word does
            if (lane == 0) __hip_atomic_store((unsigned long long*)(o + MBX_SEQ), A.mbx_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
            const int G = A.tv.n_groups;
            if (sum_lane) A.partials[(int64_t)k * G + g] = v;     // ([window 0][accumulator][group], as iso_shared_kernel)
            if (lane == NACC) A.chk[g] = 0.0;
        }
    }
    if (A.wave_clock && lane == 0 && rows > 0) {
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        double* o = A.wave_clock + 4 * (int64_t)(blockIdx.x * WG_WAVES + w);
        o[0] = (double)wc0; o[1] = (double)wall_clock64(); o[2] = (double)hw; o[3] = 1.0 + rows;
    }
}

template <int D, bool DEEP>
static hipError_t launch_cut_masks(const IsoArgs& a, dim3 grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, const HeadGain* hg) {
    dim3 block(WG_WAVES * WAVE);
    static const HeadGain no_table = {};                 // (rows == 0: the lanes stage from a.gain)
    const HeadGain& gv = hg ? *hg : no_table;
    switch (a.part_mask[0]) {
#define SSDE_CASE(M) case M: { if (ev0) hipExtLaunchKernelGGL((iso_shared_cut_kernel<M_CTCRW, D, M, DEEP>), grid, block, 0, s, ev0, ev1, 0, a, gv); \
                               else hipLaunchKernelGGL((iso_shared_cut_kernel<M_CTCRW, D, M, DEEP>), grid, block, 0, s, a, gv); } break;
        SSDE_CASE(0) SSDE_CASE(1) SSDE_CASE(2) SSDE_CASE(3) SSDE_CASE(4) SSDE_CASE(5) SSDE_CASE(6) SSDE_CASE(7)
        SSDE_CASE(8) SSDE_CASE(9) SSDE_CASE(10) SSDE_CASE(11) SSDE_CASE(12) SSDE_CASE(13) SSDE_CASE(14) SSDE_CASE(15)
#undef SSDE_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// d = 2 only (see above): the ping-pong pair of row blocks, as the other entries (k_iso_shared.inc: run_segment)
hipError_t launch_iso_shared_cut(int d, const IsoArgs& a, dim3 grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, const HeadGain* hg) {
    if (d == 2) return launch_cut_masks<2, false>(a, grid, s, ev0, ev1, hg);
    return hipErrorInvalidValue;
}

}  // namespace ssde
