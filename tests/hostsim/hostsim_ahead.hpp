// hostsim_ahead.hpp -- TEST INFRASTRUCTURE, not an engine.
//
// The host twin of k_smooth_ahead.hip, shared by hostsim_ahead.cpp (the library tests/aheadsim_lib.py loads) and ahead_san.cpp (the
// stand-alone sanitizer program): smoothsde_amd/csrc/ssde_ahead.hpp over ssde_smooth.hpp, each track walked the way one lane of the
// kernels walks it: smooth_record_row + ahead_side_row -> dense_step per state row, then per block of ssde_plan::AHEAD_BLOCK start
// rows every start's chain (ahead_load, ahead_score at the listed horizons, ahead_step) with the block's partial sums, and the
// blocks' partial sums added in ascending order.
#ifndef HOSTSIM_AHEAD_HPP
#define HOSTSIM_AHEAD_HPP

#include <algorithm>

#include "../../smoothsde_amd/csrc/ssde_ahead.hpp"
#include "../../smoothsde_amd/csrc/ssde_smooth_plan.hpp"
#include "hostsim_records.hpp"

// the problem as hostsim_records.hpp has it; crow: per row of the problem the caller's row, -1 where the row is not the caller's
// (a padded lattice row: stepped through, never a start or a target), or NULL (every row is its own); hz: n_h strictly increasing
// horizons; thr: n_thr thresholds.  Per-row outputs on the problem's rows, row-major (z n x n_h x D, lpd n x n_h), each may be NULL,
// written on scored targets only.  stats (n_tracks x n_h x n_stat, row-major, n_stat = 5 + n_thr, or NULL) is written for tracks with
// a state row only.
template <int MODEL, int D>
void hostsim_ahead_run(const TwinProblem& pb, const int64_t* crow, const int32_t* hz, int n_h, const double* thr, int n_thr, double* z,
                       double* lpd, double* stats) {
    using namespace ssde;
    typedef DenseDims<MODEL, D> DM;
    typedef SmoothRec<MODEL, D> RC;
    typedef AheadSide<MODEL, D> AS;
    constexpr int SD = DM::SD, Q = DM::Q, R = RC::R, SW = AS::SW;
    const int n_stat = AHEAD_NSTAT0 + n_thr, n_slot = n_h * n_stat, hmax = hz[n_h - 1];
    const int64_t n = pb.n;
    std::vector<double> recs, side, part((size_t)n_slot), sum((size_t)n_slot);
    for (int64_t m = 0; m < pb.n_tracks; m++) {
        const int64_t ns = pb.nrows[m] - 1, r0 = pb.row0[m];
        if (ns <= 0) continue;
        // the forward pass in record mode
        DenseLane<MODEL, D, 0> L;
        L.init(pb.a0 + m * SD, pb.p0f);
        recs.assign((size_t)ns * R, 0.0);
        side.assign((size_t)ns * SW, 0.0);
        for (int64_t s = 0; s < ns; s++) {
            const int64_t i = r0 + 1 + s;
            const double dt = (i + 1 < n) ? pb.times[i + 1] - pb.times[i] : 1.0;
            double y[D];
            for (int c = 0; c < D; c++) y[c] = pb.obs[i + c * n];
            DualN<0> H[D][D], par[Q];
            for (int p = 0; p < D; p++)
                for (int q = 0; q < D; q++) H[p][q] = DualN<0>(pb.harr ? pb.harr[(i * D + p) * D + q] : (p == q ? pb.h : 0.0));
            for (int j = 0; j < Q; j++) par[j] = DualN<0>(pb.parmat[i * Q + j]);
            const bool na = is_na(y[0], pb.any_nan);
            double* rp = &recs[(size_t)s * R];
            double* sp = &side[(size_t)s * SW];
            smooth_record_row<MODEL, D>(L, par, H, dt, y, na, [&](int k) -> double& { return rp[k]; });
            ahead_side_row<MODEL, D>(par, H, dt, y, na, [&](int k) -> double& { return sp[k]; });
            dense_step<MODEL, D, 0>(L, par, H, dt, y, na);
        }
        auto side_at = [&](int64_t s) { const double* sp = &side[(size_t)s * SW]; return [sp](int k) -> double { return sp[k]; }; };
        auto caller_row = [&](int64_t s) -> int64_t { const int64_t i = r0 + 1 + s; return crow ? crow[i] : i; };
        std::fill(sum.begin(), sum.end(), 0.0);
        const int64_t n_blk = ssde_plan::ahead_blocks(ns);
        for (int64_t blk = 0; blk < n_blk; blk++) {
            std::fill(part.begin(), part.end(), 0.0);
            const int64_t s_lo = blk * ssde_plan::AHEAD_BLOCK, s_hi = std::min<int64_t>(s_lo + ssde_plan::AHEAD_BLOCK, ns);
            double gap = 0.0;
            for (int64_t u = s_lo - 1;; u--) {
                if (u < 0) { gap += pb.times[r0 + 1] - pb.times[r0]; break; }
                gap += side_at(u)(AS::DT);
                if (caller_row(u) >= 0) break;
            }
            for (int64_t s = s_lo; s < s_hi; s++) {
                const bool start = caller_row(s) >= 0;
                if (start) {
                    DenseLane<MODEL, D, 0> S;
                    const double* rp = &recs[(size_t)s * R];
                    ahead_load<MODEL, D>([&](int k) -> double { return rp[k]; }, S);
                    double lead = gap;
                    int kc = 0;
                    for (int64_t u = s; u < ns; u++) {
                        const auto sd = side_at(u);
                        const int64_t i = r0 + 1 + u;
                        if (caller_row(u) >= 0) {
                            kc++;
                            int j = -1;
                            for (int q = 0; q < n_h; q++) if (hz[q] == kc) j = q;
                            if (j >= 0) {
                                AheadScore<D> o;
                                ahead_score<MODEL, D>(S, sd, o);
                                if (o.scored) {
                                    for (int c = 0; z && c < D; c++) z[(i * n_h + j) * D + c] = o.z[c];
                                    if (lpd) lpd[i * n_h + j] = o.lpd;
                                    double* pp = &part[(size_t)n_stat * j];
                                    ahead_fold<D>([&](int k) -> double& { return pp[k]; }, o, lead, [&](int r) -> double { return thr[r]; }, n_thr);
                                }
                            }
                        }
                        if (kc >= hmax || u + 1 >= ns) break;
                        lead += ahead_step<MODEL, D>(S, sd);
                    }
                }
                const double dts = side_at(s)(AS::DT);
                gap = start ? dts : gap + dts;
            }
            for (int k = 0; k < n_slot; k++) sum[(size_t)k] += part[(size_t)k];
        }
        for (int k = 0; stats && k < n_slot; k++) stats[m * n_slot + k] = sum[(size_t)k];
    }
}

#endif
