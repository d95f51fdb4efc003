// hostsim_simrows.hpp -- TEST INFRASTRUCTURE: ssde_simulate_rows by the lane math of csrc/ssde_simrows.hpp on the host, one (track,
// replicate) after the other -- the walk of k_sim_rows.hip without a device: the coefficient row behind an accessor, the parameters of
// intercept-only blocks once, the others per row through bands_dot, the factors, the step, the statistics.  Shared by
// hostsim_simrows.cpp (the library tests/simrowsim_lib.py loads) and simrows_san.cpp (the stand-alone sanitizer program).
#ifndef HOSTSIM_SIMROWS_HPP
#define HOSTSIM_SIMROWS_HPP

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../smoothsde_amd/csrc/ssde_simrows.hpp"

namespace ssde {

struct TwinSimrows {
    int kind, d, n_par;
    int64_t n, n_tracks;
    const int64_t* row0;
    const double* times;
    const int32_t* ncol_fe;
    const double* const* x_fe;
    const int32_t* ncol_re;
    const double* const* x_re;
    const uint8_t* link;
    const double* coeff;       // n_coeff_rows x n_coef row-major
    int n_coeff_rows, n_coef;
    const double* sigma_obs;   // NULL or [n_coeff_rows]
    const double* z0;
    uint64_t seed;
    int64_t rep0, n_rep;
    const double* thr;
    int n_thr;
};

template <int KIND>
inline void hostsim_simrows_item(const TwinSimrows& T, int64_t trk, int64_t k, double* obs, double* stats) {
    constexpr int D = SIMROWS_MAX_DIM;
    const int d = T.d, n_stat = 3 * d + 2 + T.n_thr;
    const int64_t r0 = T.row0[trk], len = T.row0[trk + 1] - r0;
    const int64_t crow = T.n_coeff_rows == 1 ? 0 : k;
    const double* cf = T.coeff + crow * T.n_coef;
    const double so = T.sigma_obs ? T.sigma_obs[crow] : 0.0;
    const uint32_t k0 = (uint32_t)T.seed, k1 = (uint32_t)(T.seed >> 32), rep = (uint32_t)(T.rep0 + k);
    double parv[SIMROWS_MAX_PAR];
    int off[SIMROWS_MAX_PAR], o = 0;
    unsigned varying = 0;
    for (int j = 0; j < T.n_par; j++) {
        off[j] = o; o += T.ncol_fe[j] + T.ncol_re[j];
        if (T.ncol_fe[j] + T.ncol_re[j] == 1 && !T.x_fe[j]) parv[j] = bands_ginv(1.0 * cf[off[j]], T.link[j], 1);
        else varying |= 1u << j;
    }
    double z[D], v[D], y[D];
    for (int c = 0; c < D; c++) { z[c] = c < d ? T.z0[c] : 0.0; v[c] = 0.0; y[c] = 0.0; }
    SimrowsAcc<D> acc;
    simrows_stat_init(acc);
    auto thr = [&](int r) -> double { return T.thr[r]; };
    for (int64_t p = 0; p < len; p++) {
        SimrowsFac F{};
        if (p > 0) {
            const int64_t i1 = r0 + p - 1;
            for (int j = 0; j < T.n_par; j++) {
                if (!((varying >> j) & 1u)) continue;
                const int kf = T.ncol_fe[j], K = kf + T.ncol_re[j];
                const double* xf = T.x_fe[j];
                const double* xr = T.x_re[j];
                const double* cj = cf + off[j];
                const double lp = bands_dot<BANDS_MAX_COLS>(
                    [&](int c) -> double { return c < kf ? (xf ? xf[i1 + T.n * c] : 1.0) : xr[i1 + T.n * (c - kf)]; },
                    [&](int c) -> double { return cj[c]; }, K);
                parv[j] = bands_ginv(lp, T.link[j], 1);
            }
            const double p1 = parv[d], p2 = T.n_par > d + 1 ? parv[d + 1] : 0.0;
            if (!bands_finite(p1) || !bands_finite(p2)) acc.bad = 1;
            F = simrows_factors<KIND>(T.times[i1 + 1] - T.times[i1], p1, p2);
        }
        for (int c = 0; c < d; c++) {
            double na, nb, no;
            simrows_deviates<KIND>(k0, k1, (uint32_t)p, (uint32_t)trk, rep, c, so > 0.0, na, nb, no);
            if (p > 0) {
                if (!bands_finite(parv[c])) acc.bad = 1;
                simrows_step<KIND>(F, parv[c], na, nb, z[c], v[c]);
            }
            y[c] = fma(so, no, z[c]);
            if (obs) obs[(r0 + p) + T.n * (c + (int64_t)d * k)] = y[c];
        }
        simrows_stat_row(acc, y, d, (uint32_t)p, thr, T.n_thr);
    }
    if (stats) {
        double* st = stats + trk + T.n_tracks * ((int64_t)n_stat * k);
        simrows_finish(acc, d, T.n_thr, len, [&](int s, double x) { st[T.n_tracks * s] = x; });
    }
}

// obs [n x d x n_rep] and stats [n_tracks x n_stat x n_rep] in the layouts of include/ssde.h; either may be NULL
inline int hostsim_simrows_run(const TwinSimrows& T, double* obs, double* stats) {
    if (T.kind < 0 || T.kind > 2 || T.d < 1 || T.d > SIMROWS_MAX_DIM || T.n_par != T.d + (T.kind == SIMROWS_BM ? 1 : 2)) return 1;
    if (T.n_thr < 0 || T.n_thr > SIMROWS_NTHR || T.n_rep < 1 || (T.n_coeff_rows != 1 && T.n_coeff_rows != T.n_rep)) return 2;
    int n_coef = 0;
    for (int j = 0; j < T.n_par; j++) {
        if (T.ncol_fe[j] < 1 || T.ncol_re[j] < 0 || T.ncol_fe[j] + T.ncol_re[j] > BANDS_MAX_COLS) return 3;
        n_coef += T.ncol_fe[j] + T.ncol_re[j];
    }
    if (n_coef != T.n_coef) return 4;
    for (int64_t t = 0; t < T.n_tracks; t++)
        for (int64_t k = 0; k < T.n_rep; k++) {
            if (T.kind == SIMROWS_CTCRW) hostsim_simrows_item<SIMROWS_CTCRW>(T, t, k, obs, stats);
            else if (T.kind == SIMROWS_OU) hostsim_simrows_item<SIMROWS_OU>(T, t, k, obs, stats);
            else hostsim_simrows_item<SIMROWS_BM>(T, t, k, obs, stats);
        }
    return 0;
}

}  // namespace ssde
#endif
