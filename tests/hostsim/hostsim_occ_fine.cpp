// hostsim_occ_fine.cpp -- TEST INFRASTRUCTURE, not an engine.
//
// The lane math of ssde_path_occupancy_fine end to end with g++, one track after the other: the record pass with side rows
// (hostsim_records.hpp), the draws' walk from the last record to the first with predict_draws_walk_kernel's store rule -- a path's
// state at step s is the LEFT end of slot(s) and the RIGHT end of slot(s - 1), every step being wanted (plan_all_slots) --, the side
// packet per slot, then per (slot, draw) what one thread of path_occ_fine_kernel does (hostsim_occ_fine.hpp) with the m, own and share
// of the real plan_fine_weights, added into integers.  tests/test_occ_fine_hostsim.py compares it bitwise with tests/occ_fine_ref.py;
// tests/test_occ_fine_plan_host.py reaches the plans of ssde_smooth_plan.hpp through the small entry points below.
#include <cstring>

#include "../../smoothsde_amd/csrc/ssde_smooth_plan.hpp"
#include "hostsim_occ_fine.hpp"
#include "hostsim_records.hpp"

using namespace ssde;

namespace {

// is_row: n flags (the row is a row of the caller's data) or NULL (every row is); wq: n quantised weights by pb's rows; group:
// n_tracks labels or NULL (0).  counts: nx * ny * n_groups cells, then n_groups for the outside.  pts: n_points, n_capped.
template <int MODEL, int D>
void run_occ_fine(const TwinProblem& pb, uint64_t seed, int64_t draw0, int n_draws, const uint8_t* is_row, const uint64_t* wq,
                  const int32_t* group, int n_groups, const OccGrid& grid, double max_step, int max_sub, uint64_t* counts, int64_t* pts) {
    typedef SmoothRec<MODEL, D> RC;
    typedef DrawFac<MODEL, D> FC;
    typedef BridgePk<MODEL, D> BK;
    constexpr int SD = RC::SD, R = RC::R, SW = BK::SW;
    const int64_t ncell = (int64_t)grid.nx * grid.ny, nt = pb.n_tracks;
    std::vector<int64_t> row0(pb.row0, pb.row0 + nt), row_map;
    std::vector<int32_t> nsv((size_t)nt), lgrp((size_t)nt, -1);
    for (int64_t m = 0; m < nt; m++) {
        nsv[(size_t)m] = (int32_t)(pb.nrows[m] - 1);
        if (nsv[(size_t)m] > 0) lgrp[(size_t)m] = group ? group[m] : 0;
    }
    const ssde_plan::QueryPlan P = ssde_plan::plan_all_slots(nsv, lgrp);
    std::vector<double> sdt(P.want_step.size(), 0.0);
    for (int64_t m = 0; m < nt; m++)
        for (int64_t i = P.want_off[(size_t)m]; i < P.want_off[(size_t)m + 1]; i++) {
            const int64_t row = row0[(size_t)m] + 1 + P.want_step[(size_t)i];
            sdt[(size_t)i] = row + 1 < pb.n ? pb.times[row + 1] - pb.times[row] : 1.0;
        }
    if (is_row) {
        row_map.resize((size_t)pb.n);
        for (int64_t i = 0; i < pb.n; i++) row_map[(size_t)i] = is_row[i] ? i : -1;
    }
    const ssde_plan::FineWeights F = ssde_plan::plan_fine_weights(P, row0, sdt, max_step, max_sub, is_row ? row_map.data() : nullptr, wq, 0);
    pts[0] = F.n_points; pts[1] = F.n_capped;
    std::vector<double> recs, side;
    for (int64_t m = 0; m < nt; m++) {
        const int64_t w0 = P.want_off[(size_t)m], w1 = P.want_off[(size_t)m + 1];
        if (w1 == w0) continue;
        const int og = lgrp[(size_t)m];
        const int64_t ns = twin_record_track<MODEL, D>(pb, m, recs, &side);
        const int64_t nw = w1 - w0;
        std::vector<double> ends((size_t)nw * n_draws * BK::EZ, 0.0), sidepk((size_t)nw * SW, 0.0);
        std::vector<double> al((size_t)n_draws * SD, 0.0);
        DrawNext<SD> nx;
        draw_next_init<SD>(nx);
        int64_t cur = w1 - 1;
        for (int64_t s = ns - 1; s >= P.want_step[(size_t)w0]; s--) {
            const double* rp = &recs[(size_t)s * R];
            const bool tail = s == ns - 1;
            double fac[FC::R];
            draw_factor_row<MODEL, D, SD>([&](int k) -> double { return rp[k]; }, tail, nx, [&](int k) -> double& { return fac[k]; });
            int64_t il = -1, ir = -1;
            if (cur >= w0 && P.want_step[(size_t)cur] == s) {
                il = cur - w0;
                const double* sp = &side[(size_t)s * SW];
                double* pk = &sidepk[(size_t)il * SW];
                bridge_side_row<MODEL, D>([&](int k) -> double { return sp[k]; }, tail, [&](int k) -> double& { return pk[k]; });
                cur--;
            }
            if (cur >= w0 && P.want_step[(size_t)cur] == s - 1) ir = cur - w0;
            for (int q = 0; q < n_draws; q++) {
                double z[SD], a[SD];
                draw_deviates<SD>(seed, (uint64_t)m, (uint32_t)s, (uint32_t)(draw0 + q), 0, z);
                for (int c = 0; c < SD; c++) a[c] = al[(size_t)q * SD + c];
                draw_step<MODEL, D, SD>([&](int k) -> double { return fac[k]; }, tail, a, z);
                for (int c = 0; c < SD; c++) {
                    al[(size_t)q * SD + c] = a[c];
                    if (il >= 0) ends[((size_t)il * n_draws + q) * BK::EZ + BK::L + c] = a[c];
                    if (ir >= 0) ends[((size_t)ir * n_draws + q) * BK::EZ + BK::R + c] = a[c];
                }
            }
        }
        for (int64_t i = 0; i < nw; i++) {
            const int64_t slot = w0 + i;
            for (int q = 0; q < n_draws; q++) {
                const double* e = &ends[((size_t)i * n_draws + q) * BK::EZ];
                occ_fine_slot<MODEL, D>(&sidepk[(size_t)i * SW], e + BK::L, e + BK::R, F.m[(size_t)slot], F.own[(size_t)slot],
                                        F.share[(size_t)slot], seed, (uint64_t)m, (uint32_t)P.want_step[(size_t)slot],
                                        (uint32_t)(draw0 + q), grid, counts + ncell * og, counts + ncell * n_groups + og);
            }
        }
    }
}

template <class T>
void copy_out(const std::vector<T>& v, T* dst) { if (!v.empty()) memcpy(dst, v.data(), v.size() * sizeof(T)); }

}  // namespace

extern "C" {

int hostsim_occ_fine(int model, int d, TWIN_PARAMS, uint64_t seed, int64_t draw0, int n_draws, const uint8_t* is_row, const uint64_t* wq,
                     const int32_t* group, int n_groups, const double* grid4, int nx, int ny, double max_step, int max_sub, uint64_t* counts,
                     int64_t* pts) {
    if (nx < 1 || ny < 1 || n_groups < 1 || (d == 1 && ny != 1) || !(max_step > 0.0)) return 2;
    const OccGrid g{grid4[0], grid4[1], grid4[2], grid4[3], nx, ny};
#define OF(MODEL, D) if (model == MODEL && d == D) { run_occ_fine<MODEL, D>(TWIN_ARGS, seed, draw0, n_draws, is_row, wq, group, n_groups, g, max_step, max_sub, counts, pts); return 0; }
    TWIN_D12(OF)
#undef OF
    return 1;
}

// plan_all_slots over nl lanes: want_off [nl + 1]; want_step: room for the sum of the positive ns
void hostsim_plan_all_slots(int64_t nl, const int32_t* ns, const int32_t* lane_grp, int64_t* want_off, int32_t* want_step) {
    const ssde_plan::QueryPlan P = ssde_plan::plan_all_slots(std::vector<int32_t>(ns, ns + nl), std::vector<int32_t>(lane_grp, lane_grp + nl));
    copy_out(P.want_off, want_off); copy_out(P.want_step, want_step);
}

// plan_all_slots then plan_fine_weights: slot_dt, m, own, share per slot; row_map / wq may be NULL; pts: n_points, n_capped
void hostsim_plan_fine_weights(int64_t nl, const int32_t* ns, const int32_t* lane_grp, const int64_t* row0, const double* slot_dt,
                               double max_step, int max_sub, const int64_t* row_map, const uint64_t* wq, uint64_t unit, int32_t* m,
                               uint64_t* own, uint64_t* share, int64_t* pts) {
    const ssde_plan::QueryPlan P = ssde_plan::plan_all_slots(std::vector<int32_t>(ns, ns + nl), std::vector<int32_t>(lane_grp, lane_grp + nl));
    const ssde_plan::FineWeights F = ssde_plan::plan_fine_weights(P, std::vector<int64_t>(row0, row0 + nl),
                                                                  std::vector<double>(slot_dt, slot_dt + P.want_step.size()), max_step,
                                                                  max_sub, row_map, wq, unit);
    copy_out(F.m, m); copy_out(F.own, own); copy_out(F.share, share);
    pts[0] = F.n_points; pts[1] = F.n_capped;
}

int hostsim_occ_fine_substeps(double dt, double max_step, int max_sub) { return ssde_plan::occ_fine_substeps(dt, max_step, max_sub); }

int hostsim_occ_fine_batch_cap(int64_t budget, int64_t n_slots, int ez, int ch, int n_draws) {
    return ssde_plan::occ_fine_batch_cap(budget, n_slots, ez, ch, n_draws);
}

}  // extern "C"
