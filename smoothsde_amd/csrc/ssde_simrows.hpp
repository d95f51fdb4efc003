// ssde_simrows.hpp -- replicate data sets simulated on the data's own rows (ssde_simulate_rows): the per-lane math, DESIGN.md §3.19.
//
// One lane owns one (track, replicate).  The transition into row position p >= 1 of the track uses the SDE parameters of the row
// before it (the reference's sub_par[i - 1, ], R/sde.R:1434-1478) and dt = times[i] - times[i - 1]: simrows_factors forms what the
// columns of the row share, simrows_step moves one column, simrows_stat_row folds the row's written observations into the check
// statistics and simrows_finish writes them.  A parameter is g(lp) with lp the fma chain bands_dot of ssde_bands.hpp over the row's
// design values and the replicate's coefficient row.
//
// The forms.  With x = dt / tau (the reference's beta dt):
//   e = exp(-x), 1 - e = -expm1(-x), 1 - e^2 = -expm1(-2 x)                             -- never 1 - exp(.)
//   OU     sd = sqrt(kappa (1 - e^2)),  z' = fma(e, z, fma(1 - e, mu, sd na))
//   BM     sd = sigma sqrt(dt),         z' = fma(sd, na, fma(mu, dt, z))
//   CTCRW  h = 2 nu^2 / pi (= sigma^2 / (2 beta) with sigma = 2 nu / sqrt(pi tau), beta = 1 / tau)
//          qvv = h (1 - e^2),  qvz = h tau (1 - e)^2,  qzz = 2 h tau^2 G(x)              (CTCRW_cov, R/utility.R:188-196)
//          G(x) = x + (1 - e^2) / 2 - 2 (1 - e): as written for x >= 1 / 4, and for x < 1 / 4 its series
//                 sum_{k = 3 .. 14} (-1)^(k + 1) (2^(k - 1) - 2) / k! x^k  (x^3 / 3 - x^4 / 4 + ...: the written form cancels to 3 u / x^2)
//          l11 = sqrt(qvv), l21 = qvz / l11, l22 = sqrt(max(fma(-l21, l21, qzz), 0))     (the Cholesky factor in (v, z) order)
//          z' = fma(l22, nb, fma(l21, na, fma(v - mu, tau (1 - e), fma(mu, dt, z)))),  v' = fma(e, v, fma(1 - e, mu, l11 na))
//   written observation y = fma(sigma_obs, no, z).
// Every fma is written out and nothing else may become one (fp contract is off in every function here), so a host build with
// -ffp-contract=off and the device build run the same operations; exp, expm1, log, sqrt and sin / cos are each platform's.
// Host- and device-compilable, like ssde_speed.hpp and ssde_bands.hpp.
#ifndef SSDE_SIMROWS_HPP
#define SSDE_SIMROWS_HPP

#include <math.h>
#include <stdint.h>

#include "ssde_bands.hpp"
#include "ssde_philox.hpp"

#ifndef SSDE_SIMROWS_MAX_THR
#define SSDE_SIMROWS_MAX_THR 8
#endif
#ifndef SSDE_SIMROWS_MAX_COEF
#define SSDE_SIMROWS_MAX_COEF 128
#endif

#if defined(__clang__)
#define SSDE_RLOOP _Pragma("unroll")
#define SSDE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SSDE_RLOOP
#define SSDE_NO_CONTRACT
#endif

namespace ssde {

constexpr int SIMROWS_NTHR = SSDE_SIMROWS_MAX_THR;
constexpr int SIMROWS_MAX_COEF = SSDE_SIMROWS_MAX_COEF;
constexpr int SIMROWS_MAX_DIM = 8;
constexpr int SIMROWS_MAX_PAR = SIMROWS_MAX_DIM + 2;
constexpr int SIMROWS_NSTAT_MAX = 3 * SIMROWS_MAX_DIM + 2 + SIMROWS_NTHR;
enum { SIMROWS_CTCRW = 0, SIMROWS_OU = 1, SIMROWS_BM = 2 };

// G(x) = x + (1 - e^(-2x)) / 2 - 2 (1 - e^(-x)), given ome = 1 - e^(-x) and ome2 = 1 - e^(-2x)
SSDE_HD double simrows_g(double x, double ome, double ome2) {
    SSDE_NO_CONTRACT
    if (x < 0.25) {
        // c_k = (-1)^(k + 1) (2^(k - 1) - 2) / k!, k = 14 .. 3, by Horner; the first term left out is 1.3e-8 x^15: below 3e-15 G at 1 / 4
        double s = -8190.0 / 87178291200.0;
        s = fma(s, x, 4094.0 / 6227020800.0);
        s = fma(s, x, -2046.0 / 479001600.0);
        s = fma(s, x, 1022.0 / 39916800.0);
        s = fma(s, x, -510.0 / 3628800.0);
        s = fma(s, x, 254.0 / 362880.0);
        s = fma(s, x, -126.0 / 40320.0);
        s = fma(s, x, 62.0 / 5040.0);
        s = fma(s, x, -30.0 / 720.0);
        s = fma(s, x, 14.0 / 120.0);
        s = fma(s, x, -6.0 / 24.0);
        s = fma(s, x, 2.0 / 6.0);
        return s * (x * x * x);
    }
    return fma(-2.0, ome, fma(0.5, ome2, x));
}

// what the columns of one transition share
struct SimrowsFac {
    double dt, e, ome, a, l11, l21, l22, sd;
};

// p1, p2: the two parameters after mu_1 .. mu_d on the natural scale -- CTCRW (tau, nu), OU (tau, kappa), BM (sigma, unused)
template <int KIND>
SSDE_HD SimrowsFac simrows_factors(double dt, double p1, double p2) {
    SSDE_NO_CONTRACT
    SimrowsFac F;
    F.dt = dt; F.e = 0.0; F.ome = 0.0; F.a = 0.0; F.l11 = 0.0; F.l21 = 0.0; F.l22 = 0.0; F.sd = 0.0;
    if (KIND == SIMROWS_BM) {
        F.sd = p1 * sqrt(dt);
        return F;
    }
    const double x = dt / p1;
    F.e = exp(-x);
    F.ome = -expm1(-x);
    const double ome2 = -expm1(-2.0 * x);
    if (KIND == SIMROWS_OU) {
        F.sd = sqrt(p2 * ome2);
        return F;
    }
    const double h = 2.0 * (p2 * p2) / 3.141592653589793;
    F.a = p1 * F.ome;
    F.l11 = sqrt(h * ome2);
    F.l21 = (h * p1) * (F.ome * F.ome) / F.l11;
    const double qzz = (2.0 * h) * (p1 * p1) * simrows_g(x, F.ome, ome2);
    F.l22 = sqrt(fmax(fma(-F.l21, F.l21, qzz), 0.0));
    return F;
}

// one column over one transition: z (and the velocity v of a CTCRW column) at the row before -> at the row
template <int KIND>
SSDE_HD void simrows_step(const SimrowsFac& F, double mu, double na, double nb, double& z, double& v) {
    SSDE_NO_CONTRACT
    if (KIND == SIMROWS_BM) {
        z = fma(F.sd, na, fma(mu, F.dt, z));
    } else if (KIND == SIMROWS_OU) {
        z = fma(F.e, z, fma(F.ome, mu, F.sd * na));
    } else {
        const double zn = fma(F.l22, nb, fma(F.l21, na, fma(v - mu, F.a, fma(mu, F.dt, z))));
        v = fma(F.e, v, fma(F.ome, mu, F.l11 * na));
        z = zn;
    }
}

// The deviates of column c at row position p of track ordinal `trk`, replicate NUMBER `rep` (k_sim.hip's stream assignment): stream
// 2c is (na, no) -- for a CTCRW (na, nb), and the first deviate of stream 2c + 1 is no, drawn only where an error is added.
template <int KIND>
SSDE_HD void simrows_deviates(uint32_t k0, uint32_t k1, uint32_t p, uint32_t trk, uint32_t rep, int c, bool with_error,
                              double& na, double& nb, double& no) {
    na = 0.0; nb = 0.0; no = 0.0;
    if (KIND == SIMROWS_CTCRW) {
        double unused;
        if (p > 0) philox_normal_pair(k0, k1, p, trk, rep, (uint32_t)(2 * c), na, nb);
        if (with_error) philox_normal_pair(k0, k1, p, trk, rep, (uint32_t)(2 * c + 1), no, unused);
    } else {
        philox_normal_pair(k0, k1, p, trk, rep, (uint32_t)(2 * c), na, no);
    }
}

// The check statistics of one (track, replicate), accumulated in row order from the written observations y.  D bounds the columns at
// compile time, d <= D is the call's.  With D_c the increment of column c into the row: sum D, sum D^2 (fma), sum D D_prev (fma, rows
// with both increments); L = sqrt(D_0^2 + ...) as an fma chain from D_0 D_0: sum L, max L, and per threshold the rows with L <= thr.
template <int D>
struct SimrowsAcc {
    double yprev[D], dprev[D], s1[D], s2[D], s11[D], sl, ml, cnt[SIMROWS_NTHR];
    int bad;
};

template <int D>
SSDE_HD void simrows_stat_init(SimrowsAcc<D>& a) {
    SSDE_RLOOP for (int c = 0; c < D; c++) { a.yprev[c] = 0.0; a.dprev[c] = 0.0; a.s1[c] = 0.0; a.s2[c] = 0.0; a.s11[c] = 0.0; }
    a.sl = 0.0; a.ml = 0.0; a.bad = 0;
    SSDE_RLOOP for (int r = 0; r < SIMROWS_NTHR; r++) a.cnt[r] = 0.0;
}

// row position p of the track (0 the first row); thr(r): threshold r of n_thr
template <int D, class G>
SSDE_HD void simrows_stat_row(SimrowsAcc<D>& a, const double (&y)[D], int d, uint32_t p, G&& thr, int n_thr) {
    SSDE_NO_CONTRACT
    double q = 0.0;
    SSDE_RLOOP for (int c = 0; c < D; c++) {
        if (c < d) {
            if (!bands_finite(y[c])) a.bad = 1;
            if (p > 0) {
                const double dc = y[c] - a.yprev[c];
                a.s1[c] += dc;
                a.s2[c] = fma(dc, dc, a.s2[c]);
                if (p > 1) a.s11[c] = fma(dc, a.dprev[c], a.s11[c]);
                q = c == 0 ? dc * dc : fma(dc, dc, q);
                a.dprev[c] = dc;
            }
            a.yprev[c] = y[c];
        }
    }
    if (p > 0) {
        const double L = sqrt(q);
        a.sl += L;
        if (p == 1 || L > a.ml) a.ml = L;
        SSDE_RLOOP for (int r = 0; r < SIMROWS_NTHR; r++)
            if (r < n_thr && L <= thr(r)) a.cnt[r] += 1.0;
    }
}

// put(s, value) for s = 0 .. 3 d + 2 + n_thr - 1; rows: the track's length.  NaN everywhere for a track of fewer than two rows and
// where an observation or a parameter was not finite (bad).
template <int D, class P>
SSDE_HD void simrows_finish(const SimrowsAcc<D>& a, int d, int n_thr, int64_t rows, P&& put) {
    const bool nan = a.bad || rows < 2;
    const double qn = __builtin_nan("");
    SSDE_RLOOP for (int c = 0; c < D; c++) {
        if (c < d) {
            put(3 * c, nan ? qn : a.s1[c]);
            put(3 * c + 1, nan ? qn : a.s2[c]);
            put(3 * c + 2, nan ? qn : a.s11[c]);
        }
    }
    put(3 * d, nan ? qn : a.sl);
    put(3 * d + 1, nan ? qn : a.ml);
    SSDE_RLOOP for (int r = 0; r < SIMROWS_NTHR; r++)
        if (r < n_thr) put(3 * d + 2 + r, nan ? qn : a.cnt[r]);
}

// What k_sim_rows.hip is launched with: one batch of `nb` replicates over all the tracks.  Design blocks are column-major with the
// leading dimension ldx; row0, times, coeff and sigma_obs are device copies of the descriptor's.
struct SimrowsArgs {
    const double* xf[SIMROWS_MAX_PAR];
    const double* xr[SIMROWS_MAX_PAR];
    int kf[SIMROWS_MAX_PAR], kr[SIMROWS_MAX_PAR], off[SIMROWS_MAX_PAR];
    unsigned char link[SIMROWS_MAX_PAR];
    int kind, d, n_par, n_coef, n_thr, n_stat, n_coeff_rows, nb;
    int64_t n, ldx, n_tracks;
    const int64_t* row0;
    const double* times;
    const double* coeff;
    const double* sigma_obs;   // NULL: no error
    double z0[SIMROWS_MAX_DIM], thr[SIMROWS_NTHR];
    uint32_t k0, k1;
    int64_t rep_first;         // the replicate NUMBER of the batch's first replicate
    int64_t coef_first;        // its coefficient row (0 throughout with one row)
    double* obs;               // NULL, or the batch's [n x d x nb]
    double* stats;             // NULL, or the batch's [n_tracks x n_stat x nb]
};

}  // namespace ssde
#endif
