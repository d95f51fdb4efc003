// ssde_smooth_plan.hpp -- the host-side plans of the calls that consume the smoother's records (ssde_engine_smooth.hip): how the
// groups are cut into chunks under the budget, how many draws go into one batch, which form every wavefront group of
// ssde_path_occupancy runs, where every query of ssde_predict lands, the distinct offsets of every slot of ssde_predict_draws, and the
// slots, sub-steps and shares of ssde_path_occupancy_fine; and, for a parent of several engines, which queries go to which engine and
// where an engine's outputs land in the parent's arrays.
// Plain C++17, no HIP: the engine uploads and launches what these return, tests/hostsim/hostsim_predict.cpp exports them to
// tests/test_smooth_plan_host.py (hostsim_predict_draws.cpp the offsets to tests/test_predict_draws_plan_host.py, hostsim_occ_fine.cpp
// the last to tests/test_occ_fine_plan_host.py).
#ifndef SSDE_SMOOTH_PLAN_HPP
#define SSDE_SMOOTH_PLAN_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "ssde_predict.hpp"

namespace ssde_plan {

// chunk the groups [0, G) so that each chunk's records fit `budget` doubles (at least one group per chunk); goff: the groups'
// record offsets, G + 1 of them
inline std::vector<int> chunk_groups(const std::vector<int64_t>& goff, int64_t budget) {
    const int G = (int)goff.size() - 1;
    std::vector<int> cut(1, 0);
    int g0 = 0;
    for (int g = 0; g < G; g++)
        if (g > g0 && goff[g + 1] - goff[g0] > budget) { cut.push_back(g); g0 = g; }
    cut.push_back(G);
    return cut;
}

// Draws per batch: what fits `budget` doubles at per_draw doubles a draw, in whole multiples of `unit` (one unit always goes), at
// most what one launch's second grid dimension takes (ch draws per wave), and no more than the call asks for.  ssde_smooth_draws
// takes any number of draws (unit 1), ssde_path_stats whole waves (unit ch).
inline int batch_cap(int64_t budget, int64_t per_draw, int unit, int ch, int n_draws) {
    int64_t nb = std::min<int64_t>(std::max<int64_t>(budget / std::max<int64_t>(per_draw, 1), unit), (int64_t)ch << 15);
    return (int)std::min<int64_t>(nb - nb % unit, n_draws);
}

// ---- ssde_path_occupancy -----------------------------------------------------------------------------------------
// Draws per batch: the call keeps nothing per draw, so the only bound is one launch's second grid dimension -- batch_cap's, at ch
// draws per wave -- in whole workgroups of nw * ch draws, and no more than the call asks for.
inline int occ_batch_cap(int nw, int ch, int n_draws) {
    return batch_cap(std::numeric_limits<int64_t>::max(), 1, nw * ch, ch, n_draws);
}

// The form of every wavefront group: lane_grp[l] is lane l's output grid (-1: the lane takes part in nothing; n_lanes of them, `wave`
// a group).  A group whose lanes all feed ONE grid (or none) runs the tile form and gets that grid (-1: none) -- unless the grid's
// cells pass tile_cells or the caller forces the global form; every other group gets `mixed`: the global form.
inline std::vector<int32_t> plan_occ_groups(const std::vector<int32_t>& lane_grp, int wave, int64_t n_cells, int64_t tile_cells,
                                            bool force_global, int32_t mixed) {
    const int64_t nl = (int64_t)lane_grp.size();
    std::vector<int32_t> grp_of((size_t)((nl + wave - 1) / wave), mixed);
    if (force_global || n_cells > tile_cells) return grp_of;
    for (size_t g = 0; g < grp_of.size(); g++) {
        int32_t one = -1;
        bool same = true;
        for (int64_t l = (int64_t)g * wave; l < std::min<int64_t>((int64_t)(g + 1) * wave, nl); l++) {
            if (lane_grp[l] < 0) continue;
            if (one < 0) one = lane_grp[l];
            same = same && lane_grp[l] == one;
        }
        if (same) grp_of[g] = one;
    }
    return grp_of;
}

// ---- ssde_predict's queries --------------------------------------------------------------------------------------
// Every query goes to the state row (lane, step) that starts its interval in the handle's resident layout, plus a residual offset.
// The wanted steps become one ascending list per lane (slots: want_step[want_off[l] .. want_off[l + 1])) and the planned queries
// are ordered by slot: order[i] is the caller's index of the i-th, q_slot[i] its slot, off[i] its residual.  A query without a state
// (a track's first row, a one-row track, past the next fix of a lattice handle) is not planned.
struct QueryPlan {
    std::vector<int64_t> order, q_slot, want_off;
    std::vector<int32_t> want_step;
    std::vector<double> off;
};

// row0 / ns: the lanes' first row and state rows in the resident layout (any order; ns <= 0: no track); pad_row: the lattice row of
// every caller row and pad_step the lattice step, or NULL when the rows ARE the caller's
inline QueryPlan plan_queries(const std::vector<int64_t>& row0, const std::vector<int32_t>& ns, const int64_t* pad_row, double pad_step,
                              const int64_t* q_row, const double* q_off, int64_t nq) {
    const int64_t nl = (int64_t)row0.size();
    std::vector<int64_t> by_row;
    for (int64_t l = 0; l < nl; l++) if (ns[l] > 0) by_row.push_back(l);
    std::sort(by_row.begin(), by_row.end(), [&](int64_t a, int64_t b) { return row0[a] < row0[b]; });
    std::vector<int64_t> start(by_row.size());
    for (size_t k = 0; k < by_row.size(); k++) start[k] = row0[by_row[k]];

    // queries -> (lane, step, residual); key = lane * 2^31 + step orders them by slot
    std::vector<int64_t> key((size_t)nq, -1);
    std::vector<double> res((size_t)nq, 0.0);
    for (int64_t k = 0; k < nq; k++) {
        const int64_t p = pad_row ? pad_row[q_row[k]] : q_row[k];
        const size_t t = std::upper_bound(start.begin(), start.end(), p) - start.begin();
        if (t == 0) continue;
        const int64_t l = by_row[t - 1], r0 = row0[l], n = ns[l];
        if (p > r0 + n) continue;                                   // (a one-row track: no lane holds it)
        int64_t st = p - r0 - 1;
        if (st < 0) continue;                                       // a track's first row carries no state
        double off = q_off[k];
        if (pad_row && st < n - 1) {
            // a caller's interval may span several lattice steps: the whole steps inside `off` move the row, the rest is the residual
            int64_t w = (int64_t)std::floor(off / pad_step + ssde::PREDICT_DT_RTOL);
            double rest = off - (double)w * pad_step;
            if (rest < 0.0) rest = 0.0;
            const int64_t pn = pad_row[q_row[k] + 1];               // the caller's next row (same track: row j is not its last)
            if (p + w > pn || (p + w == pn && rest > ssde::PREDICT_DT_RTOL * pad_step)) continue;   // past the next fix: NaN
            if (p + w == pn) rest = 0.0;
            st += w; off = rest;
        }
        key[k] = (l << 31) | st;
        res[k] = off;
    }
    QueryPlan P;
    for (int64_t k = 0; k < nq; k++) if (key[k] >= 0) P.order.push_back(k);
    std::stable_sort(P.order.begin(), P.order.end(), [&](int64_t a, int64_t b) { return key[a] < key[b]; });
    const int64_t nv = (int64_t)P.order.size();
    P.want_off.assign((size_t)nl + 1, 0);
    P.q_slot.resize((size_t)nv);
    P.off.resize((size_t)nv);
    for (int64_t i = 0; i < nv; i++) {
        const int64_t kk = key[P.order[i]];
        if (i == 0 || kk != key[P.order[i - 1]]) {
            P.want_step.push_back((int32_t)(kk & 0x7fffffff));
            P.want_off[(size_t)(kk >> 31) + 1]++;
        }
        P.q_slot[i] = (int64_t)P.want_step.size() - 1;
        P.off[i] = res[P.order[i]];
    }
    for (int64_t l = 0; l < nl; l++) P.want_off[l + 1] += P.want_off[l];
    return P;
}

// the slots [s0, s1) of the chunk of groups [g_lo, g_hi) (a chunk's lanes hold consecutive slots) and its queries [q0, q1)
struct QueryRange { int64_t s0, s1, q0, q1; };
inline QueryRange chunk_queries(const QueryPlan& P, int g_lo, int g_hi, int wave) {
    const int64_t nl = (int64_t)P.want_off.size() - 1;
    const int64_t l0 = std::min<int64_t>((int64_t)g_lo * wave, nl), l1 = std::min<int64_t>((int64_t)g_hi * wave, nl);
    const int64_t s0 = P.want_off[l0], s1 = P.want_off[l1];
    return QueryRange{s0, s1, std::lower_bound(P.q_slot.begin(), P.q_slot.end(), s0) - P.q_slot.begin(),
                      std::lower_bound(P.q_slot.begin(), P.q_slot.end(), s1) - P.q_slot.begin()};
}

// ---- ssde_predict_draws' offsets ----------------------------------------------------------------------------------
// Per slot, the distinct residual offsets of its queries in ascending order (a CSR list: slot i holds off_val[off_ptr[i] ..
// off_ptr[i + 1]), entry r of it is the offset of rank r); per planned query, its rank in its slot's list; and per distinct offset
// the queries that carry it: the caller's indices q_dest[q_ptr[g] .. q_ptr[g + 1]) for entry g of off_val.  Offsets compare as
// doubles: equal ones (+0.0 and -0.0 too) share one rank and one answer.
struct SlotOffsets {
    std::vector<int64_t> off_ptr, q_rank, q_ptr, q_dest;
    std::vector<double> off_val;
    int64_t most = 0;                                               // the longest list
};

inline SlotOffsets plan_slot_offsets(const QueryPlan& P) {
    const int64_t nv = (int64_t)P.order.size(), n_slots = (int64_t)P.want_step.size();
    SlotOffsets S;
    S.off_ptr.assign((size_t)n_slots + 1, 0);
    S.q_rank.resize((size_t)nv);
    S.q_dest.resize((size_t)nv);
    S.q_ptr.push_back(0);
    std::vector<int64_t> idx;
    for (int64_t i0 = 0; i0 < nv;) {
        int64_t i1 = i0;
        while (i1 < nv && P.q_slot[i1] == P.q_slot[i0]) i1++;
        idx.resize((size_t)(i1 - i0));
        for (int64_t i = i0; i < i1; i++) idx[(size_t)(i - i0)] = i;
        std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return P.off[a] < P.off[b]; });
        int64_t rank = -1;
        for (size_t k = 0; k < idx.size(); k++) {
            const int64_t i = idx[k];
            if (k == 0 || P.off[i] != P.off[idx[k - 1]]) {
                if (k > 0) S.q_ptr.push_back((int64_t)(i0 + k));
                S.off_val.push_back(P.off[i]);
                rank++;
            }
            S.q_rank[(size_t)i] = rank;
            S.q_dest[(size_t)(i0 + k)] = P.order[(size_t)i];
        }
        S.q_ptr.push_back(i1);
        S.off_ptr[(size_t)P.q_slot[i0] + 1] = rank + 1;
        S.most = std::max(S.most, rank + 1);
        i0 = i1;
    }
    for (int64_t i = 0; i < n_slots; i++) S.off_ptr[i + 1] += S.off_ptr[i];
    return S;
}

// ssde_predict_draws' draws per batch through batch_cap: a draw costs the ends of every slot (2 SD doubles each) and its rows of the
// output, next to the records and side rows the budget already pays for; any number of draws goes (unit 1), one always
inline int predict_draws_batch_cap(int64_t budget, int64_t n_slots, int sd, int64_t n_query, int ch, int n_draws) {
    return batch_cap(budget, n_slots * 2 * sd + n_query * sd, 1, ch, n_draws);
}

// ---- ssde_path_occupancy_fine ------------------------------------------------------------------------------------
// The wanted steps of a call that places weight at EVERY state row: lane l's list is 0 .. ns[l] - 1 when the lane takes part
// (lane_grp[l] >= 0 and ns[l] > 0) and empty otherwise.  Written arithmetically into a QueryPlan's want_off / want_step (its other
// lists stay empty): O(lanes + slots), no sort.
inline QueryPlan plan_all_slots(const std::vector<int32_t>& ns, const std::vector<int32_t>& lane_grp) {
    const int64_t nl = (int64_t)ns.size();
    QueryPlan P;
    P.want_off.assign((size_t)nl + 1, 0);
    for (int64_t l = 0; l < nl; l++) P.want_off[l + 1] = P.want_off[l] + ((lane_grp[l] >= 0 && ns[l] > 0) ? ns[l] : 0);
    P.want_step.resize((size_t)P.want_off[nl]);
    for (int64_t l = 0; l < nl; l++) {
        int32_t* w = P.want_step.data() + P.want_off[l];
        for (int64_t s = 0, m = P.want_off[l + 1] - P.want_off[l]; s < m; s++) w[s] = (int32_t)s;
    }
    return P;
}

// sub-steps of an interval dt: min(max_sub, max(1, ceil(dt / max_step))), the division IEEE; an interval that is NaN or <= 0 has one;
// *capped is set where the cap cut it
inline int32_t occ_fine_substeps(double dt, double max_step, int max_sub, bool* capped = nullptr) {
    const double c = std::ceil(dt / max_step);
    if (capped) *capped = c > (double)max_sub;
    if (!(c >= 1.0)) return 1;
    return c > (double)max_sub ? max_sub : (int32_t)c;
}

// Per slot of plan_all_slots' lists: its sub-steps m, the quanta `own` of the point at its row and `share` of each of the m - 1
// points inside it.  slot_dt: the interval of every slot (unread at a lane's last step, which has one point: m = 1); row0: the lanes'
// first rows in the resident layout (step s of lane l is row row0[l] + 1 + s); row_map: the caller's row of every resident row, -1 on
// a padded row, or NULL when the rows ARE the caller's; wq: the quantised weights by the caller's row, or NULL: every row weighs
// `unit`.  A caller's row j with W quanta owns the N points of the slots from its own up to, not including, the next caller row's
// slot: each gets W div N quanta and the row's own point W mod N more.  A padded row before a lane's first caller row belongs to no
// state row and gets nothing.  n_points: the sum of N over the caller's rows of the lanes that take part; n_capped: their
// intervals whose m the cap cut.
struct FineWeights {
    std::vector<int32_t> m;
    std::vector<uint64_t> own, share;
    int64_t n_points = 0, n_capped = 0;
};

inline FineWeights plan_fine_weights(const QueryPlan& P, const std::vector<int64_t>& row0, const std::vector<double>& slot_dt,
                                     double max_step, int max_sub, const int64_t* row_map, const uint64_t* wq, uint64_t unit) {
    const int64_t nl = (int64_t)P.want_off.size() - 1, n_slots = (int64_t)P.want_step.size();
    FineWeights F;
    F.m.assign((size_t)n_slots, 1);
    F.own.assign((size_t)n_slots, 0);
    F.share.assign((size_t)n_slots, 0);
    for (int64_t l = 0; l < nl; l++) {
        const int64_t w0 = P.want_off[l], w1 = P.want_off[l + 1];
        for (int64_t i = w0; i + 1 < w1; i++) {                        // (the last step keeps m = 1)
            bool capped = false;
            F.m[(size_t)i] = occ_fine_substeps(slot_dt[(size_t)i], max_step, max_sub, &capped);
            F.n_capped += capped ? 1 : 0;
        }
        for (int64_t i = w0; i < w1;) {
            const int64_t row = row0[l] + 1 + (i - w0);
            const int64_t crow = row_map ? row_map[row] : row;
            int64_t i1 = i + 1;
            while (row_map && i1 < w1 && row_map[row0[l] + 1 + (i1 - w0)] < 0) i1++;   // the padded rows that follow
            if (crow >= 0) {
                uint64_t np = 0;
                for (int64_t k = i; k < i1; k++) np += (uint64_t)F.m[(size_t)k];
                const uint64_t W = wq ? wq[crow] : unit, sh = W / np;
                for (int64_t k = i; k < i1; k++) F.own[(size_t)k] = F.share[(size_t)k] = sh;
                F.own[(size_t)i] += W % np;
                F.n_points += (int64_t)np;
            }
            i = i1;
        }
    }
    return F;
}

// ssde_path_occupancy_fine's draws per batch through batch_cap: a draw costs the ends of every slot (ez = BridgePk::EZ doubles
// each), next to the records and side rows the budget already pays for; any number of draws goes (unit 1), one always
inline int occ_fine_batch_cap(int64_t budget, int64_t n_slots, int ez, int ch, int n_draws) {
    return batch_cap(budget, n_slots * ez, 1, ch, n_draws);
}

// ---- ssde_forecast_scores ----------------------------------------------------------------------------------------
// The start rows of a wavefront group are cut into blocks of AHEAD_BLOCK consecutive state rows, one wave each; a block's partial
// sums are one record of n_h * n_stat doubles per lane.  The block length is part of the result's definition (a track's sums are
// added block by block, ascending), so it is a constant and no tunable.
constexpr int AHEAD_BLOCK = 32;

// blocks of a group whose longest track has `steps` state rows
inline int64_t ahead_blocks(int64_t steps) { return steps > 0 ? (steps + AHEAD_BLOCK - 1) / AHEAD_BLOCK : 0; }

// the doubles of the partial sums of a group of `wave` lanes: what a group costs the budget beside its records and side rows
inline int64_t ahead_partial_doubles(int64_t steps, int n_h, int n_stat, int wave) {
    return ahead_blocks(steps) * (int64_t)n_h * n_stat * wave;
}

// every group's first block, counted over ALL groups (G + 1 entries), from the groups' state rows
inline std::vector<int64_t> ahead_block_offsets(const std::vector<int64_t>& steps) {
    std::vector<int64_t> off(steps.size() + 1, 0);
    for (size_t g = 0; g < steps.size(); g++) off[g + 1] = off[g] + ahead_blocks(steps[g]);
    return off;
}

// the horizon list of one call: 0 accepted; 1: n_h outside 1 .. max_h (or no list); 2: a horizon outside 1 .. max_step; 3: not
// strictly increasing
inline int check_horizons(const int32_t* horizon, int n_h, int max_h, int max_step) {
    if (!horizon || n_h < 1 || n_h > max_h) return 1;
    for (int j = 0; j < n_h; j++) {
        if (horizon[j] < 1 || horizon[j] > max_step) return 2;
        if (j > 0 && horizon[j] <= horizon[j - 1]) return 3;
    }
    return 0;
}

// ---- a parent of several engines: track shards own rows [lo, lo + m), column pairs own state columns from c0 -----------------------
// Every array is column-major over its rows: element (i, c) of an [n x NCOL] array at i + n * c.
// The queries on an engine's rows: idx their places in the caller's list, rows counted from lo, offs as given.
struct QueryDeal {
    std::vector<int64_t> idx, rows;
    std::vector<double> offs;
};
inline QueryDeal deal_queries(int64_t lo, int64_t m, const int64_t* q_row, const double* q_off, int64_t nq) {
    QueryDeal D;
    for (int64_t i = 0; i < nq; i++)
        if (q_row[i] >= lo && q_row[i] < lo + m) { D.idx.push_back(i); D.rows.push_back(q_row[i] - lo); D.offs.push_back(q_off[i]); }
    return D;
}

// An engine's columns src [m x ncol] into columns c0 .. of dst [n x .]: its row i is the parent's row lo + i, or -- the dealt
// queries -- row idx[i].
inline void place_columns(double* dst, int64_t n, int c0, const double* src, int64_t m, int ncol, int64_t lo, const int64_t* idx = nullptr) {
    for (int c = 0; c < ncol && m > 0; c++) {
        double* to = dst + (size_t)n * (c0 + c);
        const double* from = src + (size_t)m * c;
        if (!idx) { memcpy(to + lo, from, (size_t)m * 8); continue; }
        for (int64_t i = 0; i < m; i++) to[idx[i]] = from[i];
    }
}

// An engine's covariances src [m x sd x sd] into the diagonal block (c0, c0) of dst [n x SD x SD] (the caller has zeroed dst: the
// cross-pair blocks are exactly zero), rows as place_columns'.
inline void place_block(double* dst, int64_t n, int SD, int c0, const double* src, int64_t m, int sd, int64_t lo, const int64_t* idx = nullptr) {
    for (int c = 0; c < sd; c++) place_columns(dst + (size_t)n * SD * (c0 + c), n, c0, src + (size_t)m * sd * c, m, sd, lo, idx);
}
// ... and a row without a state (the engine left its block NaN) has no covariance at all: every element of the parent's row is NaN
inline void place_cov_block(double* dst, int64_t n, int SD, int c0, const double* src, int64_t m, int sd, int64_t lo, const int64_t* idx = nullptr) {
    place_block(dst, n, SD, c0, src, m, sd, lo, idx);
    for (int64_t i = 0; i < m; i++)
        if (std::isnan(src[i]))
            for (int q = 0; q < SD * SD; q++) dst[(size_t)n * q + (idx ? idx[i] : lo + i)] = std::numeric_limits<double>::quiet_NaN();
}

// A track shard's statistics src [mt x n_stat x n_rep] at its tracks' places, track0 .., of dst [NT x n_stat x n_rep].  row_stat >= 0:
// that statistic is the row of a maximum, which the shard counted in its own rows; its first row lo is added (whole numbers below 2^53,
// so the sum is exact; NaN stays NaN).
inline void place_track_stats(double* dst, int64_t NT, int64_t track0, const double* src, int64_t mt, int n_stat, int64_t n_rep, int row_stat,
                              int64_t lo) {
    for (int64_t q = 0; q < (int64_t)n_stat * n_rep && mt > 0; q++) {
        double* to = dst + (size_t)NT * q + track0;
        memcpy(to, src + (size_t)mt * q, (size_t)mt * 8);
        if (row_stat >= 0 && q % n_stat == row_stat)
            for (int64_t i = 0; i < mt; i++) to[i] += (double)lo;
    }
}

// The most distinct offsets the queries of one caller's row hold.  (The distinct offsets of a slot of ssde_predict_draws are at most
// those of one caller's row, and one more; the bridge deviates' counter holds the rank of an offset in 32 bits.)
inline int64_t max_distinct_offsets(const int64_t* q_row, const double* q_off, int64_t nq) {
    std::vector<int64_t> by((size_t)nq);
    for (int64_t k = 0; k < nq; k++) by[(size_t)k] = k;
    std::sort(by.begin(), by.end(), [&](int64_t a, int64_t b) { return q_row[a] != q_row[b] ? q_row[a] < q_row[b] : q_off[a] < q_off[b]; });
    int64_t run_len = 0, most = 0;
    for (int64_t k = 0; k < nq; k++) {
        if (k == 0 || q_row[by[k]] != q_row[by[k - 1]]) run_len = 1;
        else if (q_off[by[k]] != q_off[by[k - 1]]) run_len++;
        most = std::max(most, run_len);
    }
    return most;
}

}  // namespace ssde_plan
#endif
