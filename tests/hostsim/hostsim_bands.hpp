// hostsim_bands.hpp -- TEST INFRASTRUCTURE: ssde_par_bands by the lane math of csrc/ssde_bands.hpp on the host, one row after the
// other (pass 1), one draw after the other (pass 2), then crit and pass 3 -- the walk of k_par_bands.hip without a device.  Shared by
// hostsim_bands.cpp (the library tests/bandsim_lib.py loads) and bands_san.cpp (the stand-alone sanitizer program).
#ifndef HOSTSIM_BANDS_HPP
#define HOSTSIM_BANDS_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../smoothsde_amd/csrc/ssde_bands.hpp"

namespace ssde {

struct TwinBands {
    int64_t n;
    int q;
    const int32_t* ncol_fe;
    const double* const* x_fe;
    const int32_t* ncol_re;
    const double* const* x_re;
    const uint8_t* link;
    const double* coeff;       // (1 + n_post) x n_coef row-major
    int n_post, resp;
    double level, z;
};

// `after_insert(buf, cnt)`: called after every insert with the buffer's accessor and its count (bands_san checks the order there)
template <class Hook>
inline int hostsim_bands_run(const TwinBands& T, double* est, double* pw_low, double* pw_upp, double* se_out, double* sim_low,
                             double* sim_upp, double* crit, double* max_dev, Hook&& after_insert) {
    if (T.n < 1 || T.q < 1 || T.q > BANDS_MAX_PAR || T.n_post < 2) return 1;
    const BandsPlan P = bands_plan(T.n_post, T.level);
    if (P.m_lo > BANDS_MAX_TAIL || P.m_up > BANDS_MAX_TAIL) return 2;
    const int m = P.m;
    int off[BANDS_MAX_PAR], n_coef = 0;
    for (int j = 0; j < T.q; j++) {
        if (T.ncol_fe[j] < 1 || T.ncol_re[j] < 0 || T.ncol_fe[j] + T.ncol_re[j] > BANDS_MAX_COLS) return 3;
        off[j] = n_coef; n_coef += T.ncol_fe[j] + T.ncol_re[j];
    }
    const int64_t n = T.n;
    std::vector<double> lp0v((size_t)n * T.q), sev((size_t)n * T.q), tails((size_t)2 * m), md((size_t)T.q * T.n_post, 0.0);
    for (int j = 0; j < T.q; j++) {
        const int kf = T.ncol_fe[j], K = kf + T.ncol_re[j];
        const double* c0 = T.coeff + off[j];
        for (int64_t i = 0; i < n; i++) {
            double x[BANDS_MAX_COLS];
            for (int c = 0; c < BANDS_MAX_COLS; c++)
                x[c] = c >= K ? 0.0 : (c < kf ? (T.x_fe[j] ? T.x_fe[j][i + n * c] : 1.0) : T.x_re[j][i + n * (c - kf)]);
            auto xv = [&](int c) -> double { return x[c]; };
            auto lo = [&](int s) -> double& { return tails[(size_t)s]; };
            auto up = [&](int s) -> double& { return tails[(size_t)(m + s)]; };
            const double lp0 = bands_dot<BANDS_MAX_COLS>(xv, [&](int c) -> double { return c0[c]; }, K);
            bool bad = !bands_finite(lp0);
            int n_lo = 0, n_up = 0;
            double cut_lo = INFINITY, cut_up = INFINITY;
            for (int k = 1; k <= T.n_post; k++) {
                const double* cf = c0 + (int64_t)k * n_coef;
                const double lp = bands_dot<BANDS_MAX_COLS>(xv, [&](int c) -> double { return cf[c]; }, K);
                if (!bands_finite(lp)) bad = true;
                if (lp < cut_lo) { tail_insert(lo, m, n_lo, cut_lo, lp); after_insert(lo, n_lo); }
                const double nl = -lp;
                if (nl < cut_up) { tail_insert(up, m, n_up, cut_up, nl); after_insert(up, n_up); }
            }
            if (n_lo < m || n_up < m) bad = true;
            const BandsRow r = bands_finish(lo, up, P, lp0, bad, T.link[j], T.resp, T.z);
            if (est) est[i + n * j] = r.est;
            if (pw_low) pw_low[i + n * j] = r.pw_low;
            if (pw_upp) pw_upp[i + n * j] = r.pw_upp;
            lp0v[(size_t)(i + n * j)] = r.lp0;
            sev[(size_t)(i + n * j)] = r.se;
            if (se_out) se_out[i + n * j] = r.se;
        }
        for (int k = 1; k <= T.n_post; k++) {
            const double* ck = c0 + (int64_t)k * n_coef;
            double dc[BANDS_MAX_COLS];
            for (int c = 0; c < BANDS_MAX_COLS; c++) dc[c] = c < K ? ck[c] - c0[c] : 0.0;
            double mx = 0.0;
            for (int64_t i = 0; i < n; i++) {
                const double s = sev[(size_t)(i + n * j)];
                const double dev = bands_dot<BANDS_MAX_COLS>(
                    [&](int c) -> double { return c < kf ? (T.x_fe[j] ? T.x_fe[j][i + n * c] : 1.0) : T.x_re[j][i + n * (c - kf)]; },
                    [&](int c) -> double { return dc[c]; }, K);
                const double a = bands_ratio(dev, s);
                if (s == s && a > mx) mx = a;
            }
            md[(size_t)j * T.n_post + (k - 1)] = mx;
        }
    }
    const BandsQ Q = bands_q(T.n_post, T.level);
    std::vector<double> sorted((size_t)T.n_post);
    for (int j = 0; j < T.q; j++) {
        std::copy(md.begin() + (size_t)j * T.n_post, md.begin() + (size_t)(j + 1) * T.n_post, sorted.begin());
        std::sort(sorted.begin(), sorted.end());
        double c = bands_lerp(sorted[(size_t)Q.lo], sorted[(size_t)Q.hi], Q.frac);
        if (!(c == c)) c = 0.0;
        if (crit) crit[j] = c;
        for (int64_t i = 0; i < n; i++) {
            const double l0 = lp0v[(size_t)(i + n * j)], s = sev[(size_t)(i + n * j)];
            const bool nan = !(s == s);
            const double qn = __builtin_nan("");
            if (sim_low) sim_low[i + n * j] = nan ? qn : bands_ginv(bands_sim(l0, s, c, 0), T.link[j], T.resp);
            if (sim_upp) sim_upp[i + n * j] = nan ? qn : bands_ginv(bands_sim(l0, s, c, 1), T.link[j], T.resp);
        }
    }
    if (max_dev) std::copy(md.begin(), md.end(), max_dev);
    return 0;
}

}  // namespace ssde
#endif
