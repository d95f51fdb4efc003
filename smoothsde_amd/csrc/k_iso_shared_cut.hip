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
//
// What a wave does BEFORE its first row (run_lane_cut) is this entry's own.  The rows of a part are ~6 us; ahead of them the lane code
// shared with the other entries (run_lane_shared) went through some twenty dependent memory round trips: the fields it reads lie all
// over the 2 KB of IsoArgs, and group_off[g] -> lane_nsteps -> six shuffles for ns_min -> a0 -> the first rows -> the gain slab
// followed one another.  Here the arguments are the hot block (HeadArgs, ssde_device.hpp) and the wave issues ONE round of loads: the
// group's length and ns_min (an array built at create), the lane's nsteps and a0, the first TWO row blocks (at an offset computed from
// the block for the leading groups, so that nothing waits for group_off) and the first gain slab; it drains them in the order of use.
// No floating-point operation differs from run_lane_shared's on the same window.
#define SSDE_SHARED_HAS_P2 1
#include "k_iso_shared.inc"

namespace ssde {

// The hot block in ONE batch at the kernel's entry.  Left to itself the compiler fetches each field where it is first used and waits
// for it there -- a dozen round trips to cold lines of the scalar cache in a row, where one is enough -- so the loads are written
// out, volatile, and the lane code reads the COPY (the by-value parameter itself is never touched: it only gives the block its place,
// offset 0 of the kernel's argument segment).  A wave has ~100 scalar registers and the block is 132 dwords, so it comes in two
// halves that are in flight together: the lines up to ctr's end by 16-dword scalar loads, statc and the ways out by ONE wave-wide
// vector load (lane i the i-th double from statc on), handed out with readlane where they are used -- the stationary constants of
// the directions a part does not walk are never handed out.  One wait for both.
typedef int head_line_t __attribute__((ext_vector_type(16)));
constexpr int HEAD_S_BYTES = (int)offsetof(HeadArgs, statc), HEAD_S_LINES = (HEAD_S_BYTES + 63) / 64;
constexpr int HEAD_V_DOUBLES = (int)((sizeof(HeadArgs) - HEAD_S_BYTES) / 8);
static_assert(HEAD_S_LINES == 5, "head_args_fetch spells its scalar loads out");
static_assert(HEAD_S_BYTES % 8 == 0 && sizeof(HeadArgs) % 8 == 0 && HEAD_V_DOUBLES <= WAVE, "one vector load covers statc and the ways out");
static_assert(offsetof(HeadArgs, mbx) == HEAD_S_BYTES + 8 * HEAD_STATC && offsetof(HeadArgs, wave_clock) == sizeof(HeadArgs) - 8, "the vector half: statc | ways out");
__device__ __forceinline__ double head_lane_double(double v, int i) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), i), hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
    return __hiloint2double(hi, lo);
}
template <class P>
__device__ __forceinline__ P head_lane_ptr(double v, int i) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane(__double2loint(v), i), hi = (unsigned)__builtin_amdgcn_readlane(__double2hiint(v), i);
    return (P)(((unsigned long long)hi << 32) | lo);
}
template <class T>
__device__ __forceinline__ T* head_lane_global(double v, int i) { return head_global(head_lane_ptr<T*>(v, i)); }
__device__ __forceinline__ void head_args_fetch(HeadArgs& H) {
    const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x & 63;
    const char* vp = ka + HEAD_S_BYTES + 8 * min(lane, HEAD_V_DOUBLES - 1);      // (inside the block on every lane)
    head_line_t r[HEAD_S_LINES];
    double t;
    asm volatile("global_load_dwordx2 %5, %7, off\n\t"
                 "s_load_dwordx16 %0, %6, 0x0\n\t"
                 "s_load_dwordx16 %1, %6, 0x40\n\t"
                 "s_load_dwordx16 %2, %6, 0x80\n\t"
                 "s_load_dwordx16 %3, %6, 0xc0\n\t"
                 "s_load_dwordx16 %4, %6, 0x100\n\t"
                 "s_waitcnt vmcnt(0) lgkmcnt(0)"
                 : "=&s"(r[0]), "=&s"(r[1]), "=&s"(r[2]), "=&s"(r[3]), "=&s"(r[4]), "=&v"(t)
                 : "s"(ka), "v"(vp)
                 : "memory");
    __builtin_memcpy(&H, r, HEAD_S_BYTES);
#pragma unroll
    for (int i = 0; i < HEAD_STATC; i++) H.statc[i] = head_lane_double(t, i);
    H.mbx = head_lane_global<double>(t, HEAD_STATC);
    H.mbx_seq = head_lane_ptr<unsigned long long>(t, HEAD_STATC + 1);
    H.partials = head_lane_global<double>(t, HEAD_STATC + 2);
    H.chk = head_lane_global<double>(t, HEAD_STATC + 3);
    H.chk_out = head_lane_global<double>(t, HEAD_STATC + 4);
    H.wave_clock = head_lane_global<double>(t, HEAD_STATC + 5);
    // (for the uses that no branch separates from the copy; run_lane_cut says it again at its own loads)
    H.tv.tiles = head_global(H.tv.tiles); H.tv.group_off = head_global(H.tv.group_off); H.tv.group_len = head_global(H.tv.group_len);
    H.tv.lane_nsteps = head_global(H.tv.lane_nsteps); H.tv.a0 = head_global(H.tv.a0);
    H.ns_min = head_global(H.ns_min); H.gain = head_global(H.gain);
}

// window 0 of group g, from row 0, for the directions of MASK: run_lane_shared<M_CTCRW, D, MASK, false, false, true> on one window
template <int D, int MASK>
__device__ __forceinline__ int run_lane_cut(const HeadArgs& A, const HeadGain& GV, int g, double* acc_out SSDE_STAMP_PARAM) {
    typedef SharedCtcrw<D, MASK> Lane;
    constexpr int NACC = 4 + D, SD = Lane::SD;
    const int lane = threadIdx.x & 63;
    const TileView& tv = A.tv;
    const int C = tv.C, c_obs = tv.c_obs, grows = A.gain_rows;
    const bool nt = A.stream_nt != 0;
    // ---- the one round of loads.  A leading group's rows lie at an offset that needs nothing from memory; the others wait for theirs.
    // (the OFFSET is what the two cases differ in: a pointer chosen between two branches would cost the loads their address space)
    // (head_global where a pointer of the copy is used, not where it is made: a branch in between loses it again)
    int64_t off;
    if (g < A.lead_n) off = (int64_t)g * A.lead_stride;
    else off = head_global(tv.group_off)[g];
    const double* base = head_global(tv.tiles) + off + lane;
    HeadPre<D> pre;
    load_obs_block<D>(pre.a, base, C, c_obs, nt);
    load_obs_block<D>(pre.b, base + (int64_t)SHARED_U * C * WAVE, C, c_obs, nt);       // (TILE_SPARE: inside the allocation whatever L is)
    const int L = head_global(tv.group_len)[g];
    const int ns_min = head_global(A.ns_min)[g];
    const int ns = head_global(tv.lane_nsteps)[g * WAVE + lane];
    double a0[SD];
#pragma unroll
    for (int c = 0; c < SD; c++) a0[c] = head_global(tv.a0)[((int64_t)g * SD + c) * WAVE + lane];
    if (grows > 0) gain_value_loads(GV, grows, 0, pre.gt);
    int s_begin, s_acc, s_end;
    window_bounds(L, A.n_chunks, A.window, A.t0, 0, s_begin, s_acc, s_end, A.t0_delta);      // (window 0: s_begin == s_acc == 0 under every plan)
    int s_stat = (A.gain_last + SHARED_U - 1) / SHARED_U * SHARED_U;
    if (A.gain_stat0 == 0.0) s_stat = INT32_MAX;                // ("never scored": the table path, as run_lane_shared)
    Lane S;
    S.setup(A);
    double mu[D];
#pragma unroll
    for (int a = 0; a < D; a++) mu[a] = A.mu[a];
    S.init(a0);
    const int m = min(max(s_stat, s_acc), s_end);
    run_segment<false, D, false, true, Lane, HeadArgs, true>(S, A, base, s_acc, m, ns, ns_min, mu, &GV, &pre SSDE_STAMP_ARG);
    SSDE_STAMP(1);
    run_segment<true, D, false, true>(S, A, base, m, s_end, ns, ns_min, mu);
    SSDE_STAMP(2);
    double out[NACC];
    S.finish(out);
    if (s_acc >= s_end || ns == 0) {
#pragma unroll
        for (int k = 0; k < NACC; k++) out[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < NACC; k++) acc_out[k] = out[k];
    return s_end - s_begin;
}

template <int MODEL, int D, int MASK, bool DEEP>
__global__ __launch_bounds__(WG_WAVES * WAVE, 1) void iso_shared_cut_kernel(const HeadArgs A_, const HeadGain GV) {
    static_assert(MODEL == M_CTCRW && !DEEP, "the cut's head: CTCRW, the ping-pong pair of row blocks");
#ifdef SSDE_HEAD_STAMPS
    const long long wc_entry = wall_clock64();                 // (the measuring build's wave start: the kernel's first instruction, ahead of the fetch)
#endif
    HeadArgs A;
    head_args_fetch(A);                                        // (A_: see head_args_fetch)
    constexpr int NACC = 4 + D, NP = cut_n_parts(MASK);
    constexpr int M0 = cut_part_mask(MASK, 0), M1 = cut_part_mask(MASK, 1), M2 = cut_part_mask(MASK, 2);
    static_assert(NP >= 1 && NP <= 3 && NP <= WG_WAVES, "one wave per direction part");
    // (a part's gain slab is the static LDS of ITS instantiation of run_segment: the parts must be different lane types)
    static_assert((NP < 2 || M0 != M1) && (NP < 3 || (M0 != M2 && M1 != M2)), "direction parts: distinct masks");
    static_assert((M0 | (NP > 1 ? M1 : 0) | (NP > 2 ? M2 : 0)) == MASK, "direction parts: every direction has an owner");
    static_assert(NACC <= MBX_CHK && NACC < WAVE, "a group's record is one store of wave 0");
    static_assert(sizeof(double) * (WG_WAVES * NACC + 3 * GAIN_SLAB_ROWS * GAIN_ROW) <= 160 * 1024, "static LDS of a workgroup: the sums and one gain slab per part");
    __shared__ double wsum[WG_WAVES][NACC];
    if (blockIdx.x == 0 && threadIdx.x == 0 && A.chk_out && !A.mbx) *head_global(A.chk_out) = 0.0;       // raised by the finalize launch
    const int g = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (g >= A.tv.n_groups) return;                            // (the whole workgroup: nobody is left at the barrier)
#ifdef SSDE_HEAD_STAMPS
    const long long wc0 = A.wave_clock ? wc_entry : 0;
    const long long wc_fetched = wall_clock64();
#else
    const long long wc0 = A.wave_clock ? wall_clock64() : 0;
#endif
    double acc[NACC];
    int rows = 0;
#pragma unroll
    for (int k = 0; k < NACC; k++) acc[k] = 0.0;
#ifdef SSDE_HEAD_STAMPS
    long long stamp[5] = {0, 0, 0, 0, wc_fetched};
#endif
    if (w == 0) rows = run_lane_cut<D, M0>(A, GV, g, acc SSDE_STAMP_ARG);
    if constexpr (NP > 1) { if (w == 1) rows = run_lane_cut<D, M1>(A, GV, g, acc SSDE_STAMP_ARG); }
    if constexpr (NP > 2) { if (w == 2) rows = run_lane_cut<D, M2>(A, GV, g, acc SSDE_STAMP_ARG); }
    if (w < NP) {
#pragma unroll
        for (int k = 0; k < NACC; k++) {
            const double t = wave_sum(acc[k]);
            if (lane == 0) wsum[w][k] = t;
        }
    }
    __syncthreads();
#ifdef SSDE_HEAD_STAMPS
    stamp[3] = wall_clock64();
#endif
    if (w == 0) {
        // accumulator k: [value | sigma_obs | mu_1 .. mu_D | par D | par D + 1] -- from the part that owns its direction
        const int k = lane < NACC ? lane : 0;
        const int owner = k == 0 ? 0 : k == 1 ? cut_part_of(MASK, DIR_SIG) : k < 2 + D ? cut_part_of(MASK, DIR_MU)
                        : k == 2 + D ? cut_part_of(MASK, DIR_P1) : cut_part_of(MASK, DIR_P2);
        const bool sum_lane = lane < NACC;
        const double v = sum_lane ? wsum[owner][k] : 0.0;
        if (A.mbx) {
            double* o = head_global(A.mbx) + (int64_t)g * MBX_STRIDE;
            if (sum_lane || lane == MBX_CHK) __hip_atomic_store(o + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the record has left before its sequence word does
            if (lane == 0) __hip_atomic_store((unsigned long long*)(o + MBX_SEQ), A.mbx_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
            const int G = A.tv.n_groups;
            if (sum_lane) head_global(A.partials)[(int64_t)k * G + g] = v;     // ([window 0][accumulator][group], as iso_shared_kernel)
            if (lane == NACC) head_global(A.chk)[g] = 0.0;
        }
    }
    if (A.wave_clock && lane == 0 && rows > 0) {
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        double* o = head_global(A.wave_clock) + 4 * (int64_t)(blockIdx.x * WG_WAVES + w);
        o[0] = (double)wc0; o[1] = (double)wall_clock64(); o[2] = (double)hw; o[3] = 1.0 + rows;
#ifdef SSDE_HEAD_STAMPS
        // the phase stamps ([4]: the argument block has arrived and the padding workgroups have left) as ticks since the wave's start,
        // 11 bits each (20 us; [4] in the low 8 bits: 2.5 us), in ONE double: component w of the record of the workgroup's fourth wave, which runs no part and writes
        // none of its own; its row count 0 makes the dump print it
        static_assert(cut_n_parts(MASK) < WG_WAVES, "the fourth wave's record is free");
        double* o3 = head_global(A.wave_clock) + 4 * (int64_t)(blockIdx.x * WG_WAVES + WG_WAVES - 1);
        double packed = 0.0;
        for (int k = 3; k >= 0; k--) packed = packed * 2048.0 + (double)min(max(stamp[k] - wc0, 0ll), 2047ll);
        packed = packed * 256.0 + (double)min(max(stamp[4] - wc0, 0ll), 255ll);
        o3[w] = packed;
        if (w == 0) o3[3] = 1.0;
#endif
    }
}

template <int D, bool DEEP>
static hipError_t launch_cut_masks(const IsoArgs& ia, const HeadLead& lead, dim3 grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, const HeadGain* hg) {
    dim3 block(WG_WAVES * WAVE);
    static const HeadGain no_table = {};                 // (rows == 0: the lanes stage from a.gain)
    const HeadGain& gv = hg ? *hg : no_table;
    if (!lead.ns_min) return hipErrorInvalidValue;       // (built at create with the cut's lane_nsteps)
    HeadArgs a;
    head_args_fill(a, ia, lead, gv.rows);
    switch (ia.part_mask[0]) {
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
hipError_t launch_iso_shared_cut(int d, const IsoArgs& a, const HeadLead& lead, dim3 grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, const HeadGain* hg) {
    if (d == 2) return launch_cut_masks<2, false>(a, lead, grid, s, ev0, ev1, hg);
    return hipErrorInvalidValue;
}

}  // namespace ssde
