// k_smooth_ahead.hip -- multi-step-ahead forecast errors and scores for gfx950 (ssde_forecast_scores; math in ssde_ahead.hpp, plan in
// ssde_smooth_plan.hpp, definitions DESIGN.md §3.21).
//
// ahead_kernel: lane = track as the records lay them out, one wave per (group of 64 tracks, block of AHEAD_BLOCK start rows).  For
// every start row of its block the wave loads the one-step prediction a_r, P_r from the row's record and walks it forward -- one
// chain for all horizons -- through the side rows the forward pass wrote next to the records (the row's linear predictors, interval,
// y, H and NA flag), scoring where the count of the caller's rows passed equals a listed horizon.  Starts are independent, so a
// group's start rows are spread over ceil(steps / AHEAD_BLOCK) waves; a chain may run past its block's end, never past its track's.
// Every record and side-row load is a 512-B wave access.  Per-row outputs go straight to the caller's row (on a lattice-padded handle
// through the lattice row -> caller row map, as loo_back_kernel; padded rows are stepped through and are never starts or targets).
// The sums of a (track, horizon) are kept per lane in LDS (slot-major, lane-minor: conflict-free, and no lane reads another's), and
// leave once per block as that block's partial record; ahead_finish_kernel adds a track's blocks in ascending order -- plain stores,
// no atomics -- which is what makes the statistics independent of the launch shape and of the chunking.
// 64-bit offsets throughout.  Bounds: steps u < ns of the lane only (records and side rows of the chunk); per-row stores at
// crow + n_rows * c with 0 <= crow < n_rows (the caller's rows of this engine); partials at block < blocks of the chunk; statistics
// at seg + n_trk * k with 0 <= seg < n_trk, k < n_h * n_stat.
#include "ssde_ahead.hpp"
#include "ssde_device.hpp"
#include "ssde_smooth_plan.hpp"

namespace ssde {

using ssde_plan::AHEAD_BLOCK;

static_assert(AHEAD_NTHR * sizeof(double) == sizeof(AheadArgs::thr) && AHEAD_NH * sizeof(int) == sizeof(AheadArgs::hz), "tables");

template <int MODEL, int D>
__global__ __launch_bounds__(WAVE) void ahead_kernel(const AheadArgs A) {
    typedef SmoothRec<MODEL, D> RC;
    typedef AheadSide<MODEL, D> AS;
    extern __shared__ double acc[];                                   // [n_h * n_stat][WAVE]
    const RecLane L = rec_lane(A.s);
    const int blk = blockIdx.y;
    if ((int64_t)blk >= A.blk_off[L.g + 1] - A.blk_off[L.g]) return;  // (wave-uniform)
    const int n_h = A.n_h, n_thr = A.n_thr, n_stat = AHEAD_NSTAT0 + n_thr, n_slot = n_h * n_stat;
    const bool sums = A.part != nullptr;
    if (sums)
        for (int k = 0; k < n_slot; k++) acc[k * WAVE + L.lane] = 0.0;
    const double* side0 = A.s.rc.side + L.goff / RC::R * AS::SW + L.lane;
    auto side_at = [&](int s) { return RecRow{const_cast<double*>(side0) + (int64_t)s * AS::SW * WAVE}; };
    auto caller_row = [&](int s) -> int64_t { const int64_t row = L.row0 + 1 + s; return A.row_map ? A.row_map[row] : row; };
    const int s_lo = blk * AHEAD_BLOCK, s_hi = min(s_lo + AHEAD_BLOCK, L.smax);
    const int64_t n = A.n_rows;

    // the intervals from the caller's row before s_lo up to s_lo: that row's own (the track's first row: lane_dt0) and, on a
    // lattice-padded handle, those of the padded rows between
    double gap = 0.0;
    if (s_lo < L.ns) {
        for (int u = s_lo - 1;; u--) {
            if (u < 0) { gap += A.lane_dt0[L.l]; break; }
            gap += side_at(u)(AS::DT);
            if (caller_row(u) >= 0) break;
        }
    }

    for (int s = s_lo; s < s_hi; s++) {
        const bool start = s < L.ns && caller_row(s) >= 0;
        DenseLane<MODEL, D, 0> S;
        bool live = start;
        double lead = gap;
        int kc = 0;
        if (live) ahead_load<MODEL, D>(L.row<RC::R>(s), S);
        for (int u = s; u < L.smax; u++) {
            if (!__any(live)) break;
            if (!live) continue;
            const RecRow sd = side_at(u);
            const int64_t crow = caller_row(u);
            if (crow >= 0) {
                kc++;
                int j = -1;
#pragma unroll
                for (int i = 0; i < AHEAD_NH; i++)
                    if (i < n_h && A.hz[i] == kc) j = i;
                if (j >= 0) {
                    AheadScore<D> o;
                    ahead_score<MODEL, D>(S, sd, o);
                    if (o.scored) {
                        if (A.z) {
#pragma unroll
                            for (int c = 0; c < D; c++) A.z[crow + n * ((int64_t)c + (int64_t)D * j)] = o.z[c];
                        }
                        if (A.lpd) A.lpd[crow + n * (int64_t)j] = o.lpd;
                        if (sums)
                            ahead_fold<D>([&](int k) -> double& { return acc[(k + n_stat * j) * WAVE + L.lane]; }, o, lead,
                                          [&](int r) -> double { return A.thr[r]; }, n_thr);
                    }
                }
            }
            if (kc >= A.hmax || u + 1 >= L.ns) live = false;
            else lead += ahead_step<MODEL, D>(S, sd);
        }
        if (s < L.ns) {
            const double dts = side_at(s)(AS::DT);
            gap = start ? dts : gap + dts;
        }
    }
    if (!sums) return;
    double* out = A.part + ((A.blk_off[L.g] - A.blk_base + blk) * (int64_t)n_slot) * WAVE + L.lane;
    for (int k = 0; k < n_slot; k++) out[(int64_t)k * WAVE] = acc[k * WAVE + L.lane];
}

// a track's statistics: its blocks' partial records added in ascending order by the lane that owns the track
__global__ __launch_bounds__(WAVE) void ahead_finish_kernel(const AheadArgs A) {
    const int g = A.s.rc.g0 + blockIdx.x, lane = threadIdx.x;
    const int64_t l = (int64_t)g * WAVE + lane;
    if (l >= A.s.n_lanes || A.s.lane_ns[l] <= 0) return;
    const int64_t seg = A.lane_trk[l];
    if (seg < 0 || seg >= A.n_trk) return;
    const int n_slot = A.n_h * (AHEAD_NSTAT0 + A.n_thr);
    const int64_t b0 = A.blk_off[g] - A.blk_base, nb = A.blk_off[g + 1] - A.blk_off[g];
    for (int k = 0; k < n_slot; k++) {
        double sum = 0.0;
        for (int64_t b = 0; b < nb; b++) sum += A.part[((b0 + b) * n_slot + k) * WAVE + lane];
        A.stats[seg + A.n_trk * (int64_t)k] = sum;
    }
}

// the interval the data hold for every lane's first row (the filter never uses it; the lead time of a forecast from that row does)
__global__ void ahead_dt0_kernel(const double* times, const int64_t* row0, int64_t n_lanes, int64_t n, double last_dt, double* out) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_lanes) return;
    const int64_t i = row0[l];
    out[l] = (i < 0 || i >= n) ? 0.0 : (i + 1 < n ? times[i + 1] - times[i] : last_dt);
}

hipError_t launch_ahead_dt0(const double* times, const int64_t* row0, int64_t n_lanes, int64_t n, double last_dt, double* out, hipStream_t s) {
    if (n_lanes <= 0) return hipSuccess;
    hipLaunchKernelGGL(ahead_dt0_kernel, dim3((unsigned)((n_lanes + 255) / 256)), dim3(256), 0, s, times, row0, n_lanes, n, last_dt, out);
    return hipGetLastError();
}

#define SSDE_AS(MODEL, D) if (model == MODEL && d == D) return AheadSide<MODEL, D>::SW;
int ahead_side_doubles(int model, int d) {
    SSDE_AS(M_CTCRW, 1) SSDE_AS(M_CTCRW, 2) SSDE_AS(M_OU_SSM, 1) SSDE_AS(M_OU_SSM, 2) SSDE_AS(M_BM_SSM, 1) SSDE_AS(M_BM_SSM, 2)
    return 0;
}
#undef SSDE_AS

#define SSDE_AK(MODEL, D) \
    if (a.s.model == MODEL && a.s.d == D) { hipLaunchKernelGGL((ahead_kernel<MODEL, D>), grid, dim3(WAVE), lds, s, a); launched = true; }

hipError_t launch_forecast_scores(const AheadArgs& a, hipStream_t s) {
    if (a.s.rc.n_groups == 0) return hipSuccess;
    if (a.n_h < 1 || a.n_h > AHEAD_NH || a.n_thr < 0 || a.n_thr > AHEAD_NTHR || a.hmax != a.hz[a.n_h - 1] || !a.s.rc.side ||
        a.s.rc.side_kind != REC_SIDE_AHEAD || !a.lane_dt0 || !a.blk_off || a.max_blocks > 65535 || (a.part && (!a.stats || !a.lane_trk)))
        return hipErrorInvalidValue;
    if (a.max_blocks < 1) return hipSuccess;
    const dim3 grid(a.s.rc.n_groups, a.max_blocks);
    const size_t lds = a.part ? (size_t)a.n_h * (AHEAD_NSTAT0 + a.n_thr) * WAVE * sizeof(double) : 0;
    bool launched = false;
    SSDE_AK(M_CTCRW, 1) SSDE_AK(M_CTCRW, 2) SSDE_AK(M_OU_SSM, 1) SSDE_AK(M_OU_SSM, 2) SSDE_AK(M_BM_SSM, 1) SSDE_AK(M_BM_SSM, 2)
    if (!launched) return hipErrorInvalidValue;
    if (hipError_t e = hipGetLastError()) return e;
    if (!a.part) return hipSuccess;
    hipLaunchKernelGGL(ahead_finish_kernel, dim3(a.s.rc.n_groups), dim3(WAVE), 0, s, a);
    return hipGetLastError();
}
#undef SSDE_AK

}  // namespace ssde
