// ssde_records.hpp -- the smoother's per-row records: their layout, and what every kernel that writes or walks them shares.
//
// The forward pass (dense_kernel in record mode on the tiled routes, smooth_tv_record_kernel on PATH_TV) writes one record of
// R = SmoothRec<MODEL, D>::R doubles per state row, one group (64 lanes = tracks) after another, time-major and lane-coalesced:
//
//     double k of step s of a lane of group g:   rec  + (rec_off[g] - rec_base)          + (s * R  + k) * 64 + lane
//     side row (SW doubles a row, by side_kind):  side + (rec_off[g] - rec_base) / R * SW + (s * SW + k) * 64 + lane
//
// so every load or store of one record double is a 512-B wave access.  rec_off counts doubles over ALL groups; a call produces and
// consumes the records chunk by chunk, and rec_base = rec_off[g0] makes the addresses chunk-relative.  Only this header spells
// those addresses.  The backward kernels open with rec_lane, and the two that draw paths share rec_draw_walk.
#ifndef SSDE_RECORDS_HPP
#define SSDE_RECORDS_HPP

#include <stdint.h>

#include "ssde_draws.hpp"

namespace ssde {

constexpr int REC_WAVE = 64;     // lanes of a group (ssde_device.hpp: WAVE)
constexpr int REC_SIDE_AHEAD = 1;

// the chunk of records being written or read
struct RecChunk {
    double* rec;
    double* side;                // the rows' side rows, or NULL (nothing is written) ...
    const int64_t* rec_off;      // [groups + 1] in doubles, over all groups
    int64_t rec_base;            // rec_off[g0]
    int g0, n_groups;            // this chunk's groups
    int side_kind;               // ... 0: ssde_predict's (ssde_predict.hpp), REC_SIDE_AHEAD: ssde_forecast_scores' (ssde_ahead.hpp)
};

// one row of a lane: rec(k) is its double k
struct RecRow {
    double* p;
    SSDE_HD double& operator()(int k) const { return p[(int64_t)k * REC_WAVE]; }
};

// where group g's records start inside the chunk (goff, in record doubles), and step s of a lane there
SSDE_HD int64_t rec_group(const RecChunk& c, int g) { return c.rec_off[g] - c.rec_base; }
template <int R>
SSDE_HD RecRow rec_row(const RecChunk& c, int64_t goff, int lane, int64_t s) { return RecRow{c.rec + goff + s * R * REC_WAVE + lane}; }
template <int R, int SW>
SSDE_HD RecRow rec_side_row(const RecChunk& c, int64_t goff, int lane, int64_t s) { return RecRow{c.side + goff / R * SW + s * SW * REC_WAVE + lane}; }

#if defined(__HIPCC__)
// A backward kernel's lane (one wave per group, lane = track): ns is 0 past the last track, smax the wave's longest track (uniform)
struct RecLane {
    int g, lane, ns, smax;
    int64_t l, row0, goff;
    bool has;
    double* base;                // the lane's double 0 of step 0
    template <int R>
    __device__ __forceinline__ RecRow row(int s) const { return RecRow{base + (int64_t)s * R * REC_WAVE}; }
};

// S: a SmoothArgs (rc, lane_row0, lane_ns, n_lanes)
template <class S>
__device__ __forceinline__ RecLane rec_lane(const S& A) {
    RecLane L;
    L.g = A.rc.g0 + blockIdx.x; L.lane = threadIdx.x;
    L.l = (int64_t)L.g * REC_WAVE + L.lane;
    L.has = L.l < A.n_lanes;
    L.ns = L.has ? A.lane_ns[L.l] : 0;
    L.row0 = L.has ? A.lane_row0[L.l] : 0;
    int smax = L.ns;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) smax = max(smax, __shfl_xor(smax, o, 64));
    L.smax = __builtin_amdgcn_readfirstlane(smax);
    L.goff = rec_group(A.rc, L.g);
    L.base = A.rc.rec + L.goff + L.lane;
    return L;
}

// The draws' walk from the lane's last step to its first: the row's factors once per step, then CH paths (draws draw_first + q of
// the stream `seed`, counted by `trk`) one step each.  on_row(row) runs once per state row, on_path(q, alpha) with path q's state
// there.  smin (wave-uniform): the walk stops below that step (ssde_predict_draws: nothing under the lowest wanted step is asked for).
// Pass lambdas over the kernel's own locals: accumulators behind a functor's members cost path_stats_kernel its occupancy.
template <int MODEL, int D, int CH, class Row, class Path>
__device__ __forceinline__ void rec_draw_walk(const RecLane& L, uint64_t seed, uint64_t trk, uint32_t draw_first, int col0,
                                              Row&& on_row, Path&& on_path, int smin = 0) {
    typedef SmoothRec<MODEL, D> RC;
    typedef DrawFac<MODEL, D> FC;
    constexpr int SD = RC::SD;
    double al[CH][SD];
#pragma unroll
    for (int q = 0; q < CH; q++)
#pragma unroll
        for (int c = 0; c < SD; c++) al[q][c] = 0.0;
    DrawNext<SD> nx;
    draw_next_init<SD>(nx);
    for (int s = L.smax - 1; s >= smin; s--) {
        if (s >= L.ns) continue;
        const RecRow rec = L.row<RC::R>(s);
        const bool tail = s == L.ns - 1;
        double fac[FC::R];
        draw_factor_row<MODEL, D, SD>(rec, tail, nx, [&](int k) -> double& { return fac[k]; });
        on_row(L.row0 + 1 + s);
#pragma unroll
        for (int q = 0; q < CH; q++) {
            double z[SD];
            draw_deviates<SD>(seed, trk, (uint32_t)s, draw_first + (uint32_t)q, col0, z);
            draw_step<MODEL, D, SD>([&](int k) -> double { return fac[k]; }, tail, al[q], z);
            on_path(q, al[q]);
        }
    }
}
#endif

}  // namespace ssde
#endif
