// ssde_bands.hpp -- confidence bands of the SDE parameters (ssde_par_bands): the per-lane math, DESIGN.md §3.18.
//
// A parameter's linear predictor at one row is a dot product of the row's design values with one row of the coefficient table; the
// table's row 0 is the point estimate and rows 1 .. n_post are posterior draws.  Pass 1 (lane = row) walks the draws in order and
// keeps, per row, the m smallest and the m largest linear predictors seen so far in two sorted tail buffers -- the largest as the m
// smallest of the negated values, so one insert serves both --; bands_finish reads the two order statistics each quantile needs from
// them.  Pass 2 (lane = draw) forms |dev / se| with dev the dot product with coeff[k] - coeff[0].  Everything is written with
// explicit fma so that a host build and the device build give the same bits: the ORDER of a dot product is fixed here -- column 0
// first, fixed-effect columns then random-effect columns, one fma chain starting from x_0 c_0.
// Host- and device-compilable, like ssde_speed.hpp.  The tail buffers live in memory (LDS on the device) behind an accessor; what
// the registers hold (the design values, a lane's coefficient differences) is walked by loops with constant trip counts.
#ifndef SSDE_BANDS_HPP
#define SSDE_BANDS_HPP

#include <math.h>
#include <stdint.h>

#include "ssde_math.hpp"

#ifndef SSDE_BANDS_MAX_TAIL
#define SSDE_BANDS_MAX_TAIL 64
#endif
#ifndef SSDE_BANDS_MAX_COLS
#define SSDE_BANDS_MAX_COLS 64
#endif
#ifndef SSDE_BANDS_MAX_PAR
#define SSDE_BANDS_MAX_PAR 16
#endif

#if defined(__clang__)
#define SSDE_BLOOP _Pragma("unroll")
#else
#define SSDE_BLOOP
#endif

namespace ssde {

constexpr int BANDS_MAX_TAIL = SSDE_BANDS_MAX_TAIL;
constexpr int BANDS_MAX_COLS = SSDE_BANDS_MAX_COLS;
constexpr int BANDS_MAX_PAR = SSDE_BANDS_MAX_PAR;

SSDE_HD bool bands_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }     // neither NaN nor +-inf

// R's type-7 quantile (the default of quantile()) of m sorted values at probability p: h = (m - 1) p, lo = floor(h),
// hi = min(lo + 1, m - 1), Q = x[lo] + (h - lo) (x[hi] - x[lo]).
struct BandsQ {
    int lo, hi;
    double frac;
};

SSDE_HD BandsQ bands_q(int m, double p) {
#if defined(__clang__)
#pragma clang fp contract(off)                           // h is rounded before lo is taken off it, whoever compiles this
#endif
    const double h = (double)(m - 1) * p;
    BandsQ q;
    q.lo = (int)floor(h);
    if (q.lo > m - 1) q.lo = m - 1;
    if (q.lo < 0) q.lo = 0;
    q.hi = q.lo + 1 < m - 1 ? q.lo + 1 : m - 1;
    q.frac = h - (double)q.lo;
    return q;
}

// x[lo] + frac (x[hi] - x[lo]); where the two are equal (or frac is 0) x[lo] as it is, as R's quantile() does -- the same bits
// for finite values, and no inf - inf for infinite ones
SSDE_HD double bands_lerp(double a, double b, double frac) { return (b == a || frac == 0.0) ? a : fma(frac, b - a, a); }

// What one call needs of the two tails: alpha = (1 - level) / 2; the lower quantile reads x[lo.lo], x[lo.hi] of the sorted draws,
// found at those indices of the buffer of the smallest; the upper one reads x[up.lo], x[up.hi], found at n_post - 1 - index of the
// buffer of the largest (kept negated, ascending).  m is the number of order statistics each buffer has to hold.
struct BandsPlan {
    BandsQ lo, up;
    int up_r_lo, up_r_hi;      // indices into the buffer of the largest: n_post - 1 - up.lo, n_post - 1 - up.hi
    int m_lo, m_up, m;
};

SSDE_HD BandsPlan bands_plan(int n_post, double level) {
    const double alpha = (1.0 - level) / 2.0;
    BandsPlan P;
    P.lo = bands_q(n_post, alpha);
    P.up = bands_q(n_post, 1.0 - alpha);
    P.up_r_lo = n_post - 1 - P.up.lo;
    P.up_r_hi = n_post - 1 - P.up.hi;
    P.m_lo = P.lo.hi + 1 > P.lo.lo + 2 ? P.lo.hi + 1 : P.lo.lo + 2;       // floor((n_post - 1) alpha) + 2
    P.m_up = P.up_r_lo + 1;                                               // the mirror count: n_post - floor((n_post - 1)(1 - alpha))
    P.m = P.m_lo > P.m_up ? P.m_lo : P.m_up;
    return P;
}

// the dot product: x(c) and cf(c) for c = 0 .. K - 1, KT >= K a compile-time bound
template <int KT, class X, class Cf>
SSDE_HD double bands_dot(X&& x, Cf&& cf, int K) {
    double acc = x(0) * cf(0);
    SSDE_BLOOP for (int c = 1; c < KT; c++)
        if (c < K) acc = fma(x(c), cf(c), acc);
    return acc;
}

// A tail buffer: buf(0) <= buf(1) <= ... <= buf(cnt - 1), the cnt <= m smallest values seen so far; cut is buf(m - 1) once the
// buffer is full and +inf before.  A value that does not beat the cut-off (v < cut) changes nothing: the caller tests that and
// calls tail_insert only then.  Equal values are kept with their multiplicity (a new one goes behind its equals).  NaN never
// passes v < cut.
template <class B>
SSDE_HD void tail_insert(B&& buf, int m, int& cnt, double& cut, double v) {
    int i = cnt < m ? cnt : m - 1;                       // the slot that opens: the end, or the largest's (it drops out)
    while (i > 0) {
        const double b = buf(i - 1);
        if (!(b > v)) break;
        buf(i) = b;
        i--;
    }
    buf(i) = v;
    if (cnt < m) cnt++;
    if (cnt == m) cut = buf(m - 1);
}

SSDE_HD double bands_ginv(double lp, int link, int resp) { return (resp && link == 1) ? exp(lp) : lp; }

// One (row, parameter) after the walk: lo(s) the s-th smallest linear predictor, up(s) the NEGATED s-th largest, lp0 the point
// estimate's, bad: a linear predictor was not finite.  out: est, pw_low, pw_upp (through the inverse link when resp, applied to the
// two order statistics before the interpolation), and lp0 / se on the link scale for the later passes (NaN where bad).
struct BandsRow {
    double est, pw_low, pw_upp, lp0, se;
};

template <class L, class U>
SSDE_HD BandsRow bands_finish(L&& lo, U&& up, const BandsPlan& P, double lp0, bool bad, int link, int resp, double z) {
    BandsRow r;
    const double qn = __builtin_nan("");
    if (bad) { r.est = qn; r.pw_low = qn; r.pw_upp = qn; r.lp0 = qn; r.se = qn; return r; }
    const double la = lo(P.lo.lo), lb = lo(P.lo.hi);
    const double ua = -up(P.up_r_lo), ub = -up(P.up_r_hi);
    const double qlo = bands_lerp(la, lb, P.lo.frac);
    r.est = bands_ginv(lp0, link, resp);
    if (resp && link == 1) {
        r.pw_low = bands_lerp(exp(la), exp(lb), P.lo.frac);
        r.pw_upp = bands_lerp(exp(ua), exp(ub), P.up.frac);
    } else {
        r.pw_low = qlo;
        r.pw_upp = bands_lerp(ua, ub, P.up.frac);
    }
    r.lp0 = lp0;
    r.se = (lp0 - qlo) / z;
    return r;
}

// |dev / se| with 0 / 0 counted as 0 and x / 0 = inf kept (R/sde.R:1155-1159)
SSDE_HD double bands_ratio(double dev, double se) {
    const double a = fabs(dev / se);
    return a == a ? a : 0.0;
}

// the simultaneous band's two ends on the link scale
SSDE_HD double bands_sim(double lp0, double se, double crit, int upper) { return fma(upper ? crit : -crit, se, lp0); }

// What the three passes of k_par_bands.hip are launched with: one chunk of `n` whole rows.  Blocks are column-major with the leading
// dimension ldx, the chunk's outputs with ldo; lp0 / se are the n x n_par scratch of the later passes (leading dimension lds).
struct BandsArgs {
    const double* xf[BANDS_MAX_PAR];
    const double* xr[BANDS_MAX_PAR];
    int kf[BANDS_MAX_PAR], kr[BANDS_MAX_PAR], off[BANDS_MAX_PAR];
    unsigned char link[BANDS_MAX_PAR];
    int n_par, n_coef, n_post, resp;
    int64_t n, ldx, ldo, lds;
    const double* coeff;       // (1 + n_post) x n_coef, row-major, HBM
    double z;
    BandsPlan plan;
    double *est, *pw_low, *pw_upp;     // pass 1 (each may be NULL)
    double *lp0, *se;                  // pass 1 writes (NULL: pointwise only), passes 2 and 3 read
    int64_t rows_per_block;            // pass 2: rows of one row block, a multiple of 64
    double* part;                      // pass 2: [row block][n_par][n_post] maxima of the blocks
    double* max_dev;                   // the reduction: [n_par][n_post], max-ed into
    double crit[BANDS_MAX_PAR];        // pass 3
    double *sim_low, *sim_upp;         // pass 3 (each may be NULL)
};

constexpr int64_t BANDS_MAX_ROW_BLOCKS = 512;

// rows of one row block of pass 2 for a chunk of n rows: the smallest multiple of 64 that needs no more than BANDS_MAX_ROW_BLOCKS
SSDE_HD int64_t bands_rows_per_block(int64_t n) {
    const int64_t per = (n + 64 * BANDS_MAX_ROW_BLOCKS - 1) / (64 * BANDS_MAX_ROW_BLOCKS);
    return 64 * (per < 1 ? 1 : per);
}

}  // namespace ssde
#endif
