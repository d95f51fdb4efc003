// hostsim_speed.hpp -- TEST INFRASTRUCTURE, not an engine.
//
// The host twin of k_path_speed.hip, shared by hostsim_speed.cpp (the library tests/speedsim_lib.py loads) and speed_san.cpp (the
// stand-alone sanitizer program): smoothsde_amd/csrc/ssde_speed.hpp over ssde_draws.hpp / ssde_smooth.hpp, each track walked the way
// one lane of the kernels walks it: smooth_record_row -> dense_step per state row, then draw_factor_row, draw_step and speed_step per
// draw from the last record to the first, speed_finish at the end; the rows' 0 / 1 indicators are added over the draws.
#ifndef HOSTSIM_SPEED_HPP
#define HOSTSIM_SPEED_HPP

#include "../../smoothsde_amd/csrc/ssde_speed.hpp"
#include "hostsim_records.hpp"

// the problem as hostsim_records.hpp has it; crow: per row of the problem the caller's row, -1 where the row is not the caller's, or
// NULL (every row is its own); weight: by the caller's row, or NULL (1); thr: n_thr thresholds.  stats (n_draws x n_tracks x n_stat,
// row-major, or NULL) is written for tracks with a state row only; below (n_out x n_thr, element (j, r) at j + n_out r, or NULL)
// is ADDED to.
template <int MODEL, int D>
void hostsim_speed_run(const TwinProblem& pb, uint64_t seed, int64_t draw0, int n_draws, const int64_t* crow, int64_t n_out,
                       const double* weight, const double* thr, int n_thr, double* stats, uint32_t* below) {
    using namespace ssde;
    typedef SmoothRec<MODEL, D> RC;
    typedef DrawFac<MODEL, D> FC;
    constexpr int SD = RC::SD, R = RC::R;
    const int n_stat = 5 + n_thr;
    std::vector<double> recs;
    for (int64_t m = 0; m < pb.n_tracks; m++) {
        const int64_t ns = twin_record_track<MODEL, D>(pb, m, recs);
        if (ns <= 0) continue;
        std::vector<double> al((size_t)n_draws * SD, 0.0);
        std::vector<SpeedAcc<D>> acc((size_t)n_draws);
        for (auto& a : acc) speed_init<D>(a);
        DrawNext<SD> nx;
        draw_next_init<SD>(nx);
        for (int64_t s = ns - 1; s >= 0; s--) {
            const double* rp = &recs[(size_t)s * R];
            const bool tail = s == ns - 1;
            double fac[FC::R];
            draw_factor_row<MODEL, D, SD>([&](int k) -> double { return rp[k]; }, tail, nx, [&](int k) -> double& { return fac[k]; });
            const int64_t i = pb.row0[m] + 1 + s;
            const int64_t j = crow ? crow[i] : i;
            const bool is_row = j >= 0;
            const double w = (is_row && weight) ? weight[j] : 1.0;
            for (int q = 0; q < n_draws; q++) {
                double z[SD], a[SD];
                int ind[SPEED_NTHR];
                draw_deviates<SD>(seed, (uint64_t)m, (uint32_t)s, (uint32_t)(draw0 + q), 0, z);
                for (int c = 0; c < SD; c++) a[c] = al[(size_t)q * SD + c];
                draw_step<MODEL, D, SD>([&](int k) -> double { return fac[k]; }, tail, a, z);
                for (int c = 0; c < SD; c++) al[(size_t)q * SD + c] = a[c];
                speed_step<MODEL, D, SD>(acc[(size_t)q], a, is_row, j, w, [&](int k) -> double { return thr[k]; }, n_thr, ind);
                for (int r = 0; below && is_row && r < n_thr; r++) below[j + n_out * r] += (uint32_t)ind[r];
            }
        }
        for (int q = 0; stats && q < n_draws; q++) {
            double st[SPEED_NSTAT_MAX];
            speed_finish<D>(acc[(size_t)q], n_thr, st);
            for (int k = 0; k < n_stat; k++) stats[((int64_t)q * pb.n_tracks + m) * n_stat + k] = st[k];
        }
    }
}

#endif
