// hostsim_loo.hpp -- TEST INFRASTRUCTURE, not an engine.
//
// The host twin of k_smooth_loo.hip, shared by hostsim_loo.cpp (the library tests/loosim_lib.py loads) and loo_san.cpp (the
// stand-alone sanitizer program): smoothsde_amd/csrc/ssde_loo.hpp over ssde_smooth.hpp, each track walked the way one lane of the
// kernels walks it: smooth_record_row -> dense_step per state row (hostsim_records.hpp), then loo_back_row from the last record to
// the first with the served rows stored and folded into the track's statistics, loo_finish at the end.
#ifndef HOSTSIM_LOO_HPP
#define HOSTSIM_LOO_HPP

#include "../../smoothsde_amd/csrc/ssde_loo.hpp"
#include "hostsim_records.hpp"

// the problem as hostsim_records.hpp has it; crow: per row of the problem the caller's row, -1 where the row is not the caller's, or
// NULL (every row is its own); thr: n_thr thresholds.  Per-row outputs on the problem's rows, row-major (mean, resid n x D; cov
// n x D x D; lpd n), each may be NULL; they are written on served rows only.  stats (n_tracks x n_stat, row-major, or NULL) is
// written for tracks with a state row only.
template <int MODEL, int D>
void hostsim_loo_run(const TwinProblem& pb, const int64_t* crow, const double* thr, int n_thr, double* mean, double* cov, double* resid,
                     double* lpd, double* stats) {
    using namespace ssde;
    typedef SmoothRec<MODEL, D> RC;
    constexpr int SD = RC::SD, R = RC::R;
    const int n_stat = 4 + n_thr;
    std::vector<double> recs;
    for (int64_t m = 0; m < pb.n_tracks; m++) {
        const int64_t ns = twin_record_track<MODEL, D>(pb, m, recs);
        if (ns <= 0) continue;
        double r[SD], N[SD][SD];
        for (int a = 0; a < SD; a++) { r[a] = 0.0; for (int b = 0; b < SD; b++) N[a][b] = 0.0; }
        LooAcc acc;
        loo_init(acc);
        for (int64_t s = ns - 1; s >= 0; s--) {
            const double* rp = &recs[(size_t)s * R];
            LooRow<D> o;
            loo_back_row<MODEL, D, SD>(r, N, s == ns - 1, [&](int k) -> double { return rp[k]; }, o);
            const int64_t i = pb.row0[m] + 1 + s;
            const int64_t j = crow ? crow[i] : i;
            if (!o.served || j < 0) continue;
            for (int a = 0; a < D; a++) {
                if (mean) mean[i * D + a] = o.mean[a];
                for (int b = 0; cov && b < D; b++) cov[(i * D + a) * D + b] = o.cov[a][b];
            }
            if (!o.white) continue;
            for (int a = 0; resid && a < D; a++) resid[i * D + a] = o.z[a];
            if (lpd) lpd[i] = o.lpd;
            loo_fold(acc, o.q, o.lpd, j, [&](int k) -> double { return thr[k]; }, n_thr);
        }
        if (!stats) continue;
        double st[LOO_NSTAT_MAX];
        loo_finish(acc, n_thr, st);
        for (int k = 0; k < n_stat; k++) stats[m * n_stat + k] = st[k];
    }
}

#endif
