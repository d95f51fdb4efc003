// k_path_speed.hip -- speed along posterior state paths for gfx950 (ssde_path_speed; math in ssde_speed.hpp over ssde_draws.hpp,
// definitions DESIGN.md §3.17).
//
// path_speed_kernel: the walk of smooth_draws_kernel (rec_draw_walk, ssde_records.hpp: lane = track, one wave per (group of 64 tracks,
// chunk of DRAW_CH draws)) with the n x sdim stores of every draw replaced by speed_step.  Two outputs:
//   stats      the sum, the maximum and its row, the resultant and the band sums of each (lane, draw) stay in registers, and after the
//              walk the lane stores n_stat numbers per draw at its track's ordinal.  One wave owns each (track, draw): plain stores.
//   row_below  per state row the lane adds the chunk's 0 / 1 indicators into one count 0 .. DRAW_CH per threshold and, where it is not
//              zero, adds it to the row's entry in HBM with a 32-bit integer atomicAdd whose result is not used (the way
//              k_path_occ.hip's global form adds its quanta).  Integer sums do not depend on the order of arrival, so the table is
//              bitwise the same whatever chunks, batches and shards ran where.
// Either output may be absent (a uniform branch).  Per-row reads beside the records: the row's weight and, on a lattice-padded
// handle, its entry of the lattice row -> caller row map, as path_stats_kernel.  64-bit offsets throughout; every index into row_below
// is crow + n_rows * r with 0 <= crow < n_rows (the map's entries, or the handle's own rows) and r < n_thr.
#include "ssde_device.hpp"
#include "ssde_speed.hpp"

namespace ssde {

static_assert(SPEED_NTHR * sizeof(double) == sizeof(SpeedArgs::thr), "threshold table");

template <int MODEL, int D>
__global__ __launch_bounds__(WAVE) void path_speed_kernel(const SpeedArgs A) {
    constexpr int SD = SmoothRec<MODEL, D>::SD;
    const RecLane L = rec_lane(A.d.s);
    const int k0 = blockIdx.y * DRAW_CH;
    const int64_t seg = L.has ? A.d.lane_trk[L.l] : 0;
    SpeedAcc<D> acc[DRAW_CH];
#pragma unroll
    for (int q = 0; q < DRAW_CH; q++) speed_init<D>(acc[q]);
    const int nthr = A.n_thr;
    const int live = A.d.n_draws - k0;                                // draws of this chunk that are the batch's (uniform)
    bool is_row = false;
    double w = 1.0;
    int64_t crow = -1;
    int cnt[SPEED_NTHR];
    rec_draw_walk<MODEL, D, DRAW_CH>(
        L, A.d.seed, (uint64_t)(A.d.track0 + seg), A.d.draw0 + (uint32_t)k0, A.d.col0,
        [&](int64_t row) {
            crow = A.row_map ? A.row_map[row] : row;
            is_row = crow >= 0;
            w = (is_row && A.weight) ? A.weight[crow] : 1.0;
#pragma unroll
            for (int r = 0; r < SPEED_NTHR; r++) cnt[r] = 0;
        },
        [&](int q, const double (&al)[SD]) {
            int below[SPEED_NTHR];
            speed_step<MODEL, D, SD>(acc[q], al, is_row, crow, w, [&](int r) -> double { return A.thr[r]; }, nthr, below);
            if (q < live) {
#pragma unroll
                for (int r = 0; r < SPEED_NTHR; r++) cnt[r] += below[r];
            }
            if (q == DRAW_CH - 1 && A.row_below) {                    // the chunk's last path of this row: its counts go out
#pragma unroll
                for (int r = 0; r < SPEED_NTHR; r++)
                    if (r < nthr && cnt[r]) atomicAdd(&A.row_below[crow + A.n_rows * r], (uint32_t)cnt[r]);
            }
        });
    if (L.ns <= 0 || !A.stats) return;                                // no state row: the preset NaN stays
    const int nstat = 5 + nthr;
#pragma unroll
    for (int q = 0; q < DRAW_CH; q++) {
        if (q >= live) continue;
        double st[SPEED_NSTAT_MAX];
        speed_finish<D>(acc[q], nthr, st);
        double* o = A.stats + seg + A.n_trk * ((int64_t)nstat * (k0 + q));
#pragma unroll
        for (int k = 0; k < SPEED_NSTAT_MAX; k++)
            if (k < nstat) o[A.n_trk * k] = st[k];
    }
}

hipError_t launch_path_speed(const SpeedArgs& a, hipStream_t s) {
    if (a.d.s.rc.n_groups == 0 || a.d.n_draws <= 0) return hipSuccess;
    if (a.n_thr < 0 || a.n_thr > SPEED_NTHR || (a.row_below && a.n_thr == 0)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.d.s.rc.n_groups, (unsigned)((a.d.n_draws + DRAW_CH - 1) / DRAW_CH));
    if (grid.y > 65535u) return hipErrorInvalidValue;
#define SSDE_SK(MODEL, D) \
    if (a.d.s.model == MODEL && a.d.s.d == D) { hipLaunchKernelGGL((path_speed_kernel<MODEL, D>), grid, dim3(WAVE), 0, s, a); return hipGetLastError(); }
    SSDE_SK(M_CTCRW, 1) SSDE_SK(M_CTCRW, 2)
#undef SSDE_SK
    return hipErrorInvalidValue;
}

}  // namespace ssde
