// ssde_prox.hpp -- proximity of posterior paths between tracks (ssde_path_proximity): the per-point step, the combine of two
// accumulators, the finish and the host's tile plan, DESIGN.md §3.16.  The kernels (k_path_prox.hip), the engine and the host twin
// (tests/hostsim/hostsim_prox.cpp) all take them from here.  Host- and device-compilable, like ssde_path.hpp; the tile plan runs on
// the host only.
//
// A ProxAcc holds, for some of one pair's points under one draw: the smallest distance and the index inside the pair of the first
// point that attains it -- compared as the pair (distance, index) --, a flag for a position that was not finite, and per radius the
// quanta of the points within it.  min under a total order, OR and integer addition are associative and commutative, so the result
// of combining any set of accumulators does not depend on the order or the grouping: lanes, waves, tiles, batches and devices may cut
// a pair's points in any way.  That is why nothing here is a floating-point sum and why the kernels need no atomics.
#ifndef SSDE_PROX_HPP
#define SSDE_PROX_HPP

#include <math.h>
#include <stdint.h>

#include "ssde_path.hpp"

#ifndef SSDE_PROX_MAX_RADII
#define SSDE_PROX_MAX_RADII 8
#endif

#include <vector>

namespace ssde {

constexpr int PROX_NRAD = SSDE_PROX_MAX_RADII;
constexpr int PROX_NSTAT_MAX = 2 + PROX_NRAD;
constexpr int PROX_TILE = 256;                                      // points per tile: one workgroup's lanes
constexpr int PROX_REC = 3 + PROX_NRAD;                             // 64-bit words of a stored accumulator: dist | idx | bad | sums
constexpr int64_t PROX_NO_IDX = 0x7fffffffffffffffLL;

struct ProxAcc {
    double dist;                                                    // +inf: no point yet
    int64_t idx;                                                    // PROX_NO_IDX: no point yet
    uint64_t bad;                                                   // 1: a position that was not finite
    uint64_t sum[PROX_NRAD];
};

SSDE_HD void prox_init(ProxAcc& a) {
    a.dist = __builtin_inf(); a.idx = PROX_NO_IDX; a.bad = 0;
    SSDE_PLOOP for (int r = 0; r < PROX_NRAD; r++) a.sum[r] = 0;
}

// (distance, index) of a before that of b
SSDE_HD bool prox_before(double da, int64_t ia, double db, int64_t ib) { return da < db || (da == db && ia < ib); }

// One point: the positions pa / pb of the two sides, its index inside the pair, its weight in quanta; radius(r) the r-th radius.  A
// point with a position that is not finite sets the flag and enters nothing else (every statistic of its pair and draw is NaN).
template <int D, class G>
SSDE_HD void prox_step(ProxAcc& a, const double (&pa)[D], const double (&pb)[D], int64_t idx, uint64_t wq, G&& radius, int n_radii) {
    bool ok = true;
    SSDE_PLOOP for (int c = 0; c < D; c++)
        ok = ok && fabs(pa[c]) <= 1.7976931348623157e308 && fabs(pb[c]) <= 1.7976931348623157e308;     // NaN or +-inf fail
    if (!ok) { a.bad = 1; return; }
    const double dist = path_dist<D>(pa, pb);
    if (prox_before(dist, idx, a.dist, a.idx)) { a.dist = dist; a.idx = idx; }
    SSDE_PLOOP for (int r = 0; r < PROX_NRAD; r++)
        if (r < n_radii && dist <= radius(r)) a.sum[r] += wq;
}

SSDE_HD void prox_combine(ProxAcc& a, const ProxAcc& b) {
    if (prox_before(b.dist, b.idx, a.dist, a.idx)) { a.dist = b.dist; a.idx = b.idx; }
    a.bad |= b.bad;
    SSDE_PLOOP for (int r = 0; r < PROX_NRAD; r++) a.sum[r] += b.sum[r];
}

// out[0 .. 2 + n_radii): the smallest distance, the index of the first point that attains it, the sums as ldexp((double)sum, e);
// every one NaN where a position was not finite or the accumulator saw no point.  Elements past 2 + n_radii are 0 and mean nothing.
SSDE_HD void prox_finish(const ProxAcc& a, int n_radii, int e, double (&out)[PROX_NSTAT_MAX]) {
    const bool nan = a.bad != 0 || a.idx == PROX_NO_IDX;
    const double qn = __builtin_nan("");
    out[0] = nan ? qn : a.dist;
    out[1] = nan ? qn : (double)a.idx;
    SSDE_PLOOP for (int r = 0; r < PROX_NRAD; r++) out[2 + r] = r >= n_radii ? 0.0 : (nan ? qn : ldexp((double)a.sum[r], e));
}

// An accumulator as PROX_REC words, word k of record i at base + k * stride + i (records fastest: neighbouring lanes store and load
// neighbouring words)
SSDE_HD void prox_store(const ProxAcc& a, uint64_t* base, int64_t stride) {
    union { double d; uint64_t u; } v;
    v.d = a.dist;
    base[0] = v.u; base[stride] = (uint64_t)a.idx; base[2 * stride] = a.bad;
    SSDE_PLOOP for (int r = 0; r < PROX_NRAD; r++) base[(int64_t)(3 + r) * stride] = a.sum[r];
}
SSDE_HD void prox_load(ProxAcc& a, const uint64_t* base, int64_t stride) {
    union { double d; uint64_t u; } v;
    v.u = base[0];
    a.dist = v.d; a.idx = (int64_t)base[stride]; a.bad = base[2 * stride];
    SSDE_PLOOP for (int r = 0; r < PROX_NRAD; r++) a.sum[r] = base[(int64_t)(3 + r) * stride];
}

// The tile plan (host only): every pair's points pair_ptr[p] .. pair_ptr[p + 1] are cut into tiles of at most `tile` consecutive points.  A tile
// never spans pairs and an empty pair has none.  tile -> (pair, first point, index of that point inside the pair, points);
// pair p owns the tiles pair_tile[p] .. pair_tile[p + 1].
struct ProxPlan {
    std::vector<int64_t> tile_pair, tile_first, tile_idx0, pair_tile;
    std::vector<int32_t> tile_count;
    int64_t n_tiles = 0, tiles_max = 0;
};

inline ProxPlan plan_prox_tiles(const int64_t* pair_ptr, int64_t n_pairs, int tile = PROX_TILE) {
    ProxPlan P;
    P.pair_tile.assign((size_t)n_pairs + 1, 0);
    for (int64_t p = 0; p < n_pairs; p++) {
        const int64_t a = pair_ptr[p], b = pair_ptr[p + 1];
        int64_t nt = 0;
        for (int64_t i = a; i < b; i += tile, nt++) {
            P.tile_pair.push_back(p);
            P.tile_first.push_back(i);
            P.tile_idx0.push_back(i - a);
            P.tile_count.push_back((int32_t)(b - i < tile ? b - i : tile));
        }
        P.pair_tile[(size_t)p + 1] = P.pair_tile[(size_t)p] + nt;
        if (nt > P.tiles_max) P.tiles_max = nt;
    }
    P.n_tiles = (int64_t)P.tile_pair.size();
    return P;
}

// ssde_path_proximity's draws per batch through batch_cap's rule (ssde_smooth_plan.hpp: budget / per_draw, at least one, at most ch
// << 15): per draw the ends of every slot (2 SD doubles each), its rows of the query output (2 n_point x SD), the tiles' partial
// records and the pairs' statistics.  Returns the doubles one draw costs.
inline int64_t prox_per_draw_doubles(int64_t n_slots, int sd, int64_t n_point, int64_t n_tiles, int64_t n_pairs, int n_stat) {
    return n_slots * 2 * sd + 2 * n_point * sd + n_tiles * PROX_REC + n_pairs * n_stat;
}

}  // namespace ssde
#endif
