// ssde_lagforms.hpp -- the bulk's forms at one theta, on the host (the statistics: ssde_lagstats.hpp).
//
// v = M lam (and the same for the check's shorter cut), then per tap row i its share of S, C_1..3 and su_a (the mu dt terms
// through s and n), summed over the rows by a fixed tree and turned into the accumulators tf_finish forms (ssde_tf.hpp, as
// TfCtcrw::finish).  The result goes BY VALUE into the reducing launch (ReduceArgs.lag_acc, ssde_device.hpp): nothing of it lives
// in device memory.  Taps beyond the cut are exact zeros, so the loops stop at K: ~(K + 1)^2 products per cut, both cuts from one
// pass over the rows of M.
#pragma once
#include "ssde_lagstats.hpp"
#include "ssde_tf.hpp"

#include <cmath>

namespace ssde {

constexpr int LAG_NRAW = 6;           // raw sums of a cut: S, C_1, C_2, C_3, su_1, su_2

struct LagFormArgs {
    const double* M;                  // [LAG_N][LAG_N] (host)
    const double* s;                  // [2][LAG_N] (host)
    double n;                         // bulk rows
    int K, Kc;                        // taps 0..K of the forms, 0..Kc of the check
    int d, mask;                      // response coordinates, DIR_* bits of the evaluation
    double lam[LAG_N];                // impulse response of u
    double rr[LAG_N];                 // impulse response of r (r_{t-k}: rr shifted by k)
    double sum_lam[2], sum_rho[2][3]; // sums of the taps 0..K (index 0) and 0..Kc (index 1)
    double cm[2];                     // mu_a dt
    double statc[48];                 // the stationary constants (IsoArgs.statc): tf_finish forms the accumulators from them
};

struct LagFormOut {
    double raw[2][LAG_NRAW];          // the raw sums of the cut K (index 0) and of the check's cut Kc (index 1)
    double acc[NACC_MAX];             // the 4 + d accumulators of the cut K
    double chk;                       // the largest relative difference between the two cuts
};

// sums of the taps of both cuts, as the forms use them (f.lam, f.rr, f.K, f.Kc set)
// (serial sums from tap 0 on: the shorter cut's sum is the longer one's running sum as it passes Kc -- one walk, four chains, the
//  bits of a walk per cut)
inline void lag_tap_sums(LagFormArgs& f) {
    const int k0 = f.K > f.Kc ? f.K : f.Kc;
    double sl = 0.0, sr[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < 2; c++) {
        f.sum_lam[c] = 0.0;
        for (int j = 0; j < 3; j++) f.sum_rho[c][j] = 0.0;
    }
    for (int i = 0; i <= k0; i++) {
        sl += f.lam[i];
        for (int j = 0; j < 3; j++)
            if (i >= j + 1) sr[j] += f.rr[i - j - 1];
        for (int c = 0; c < 2; c++)
            if (i == (c ? f.Kc : f.K)) {
                f.sum_lam[c] = sl;
                for (int j = 0; j < 3; j++) f.sum_rho[c][j] = sr[j];
            }
    }
}

// Four doubles as one value (the compilers' vector extension, as head_v4 of ssde_headforms.hpp): the partial sums of a row's products
// are the elements, so the order of every sum is the same whatever the instruction set.
typedef double lag_v4 __attribute__((vector_size(32)));
#define SSDE_LAG_INLINE inline __attribute__((always_inline))

// The raw sums of both cuts from ONE pass over rows 0..K of M.  Fixed order:
//   - the taps of each cut go to a zero-padded local first (nothing past a cut is read from the caller's arrays), so one loop over
//     whole blocks of eight serves both cuts -- past a cut it adds exact zeros;
//   - per row and cut eight partial sums, lane = tap index modulo 8 (two values of four), combined as the element-wise sum of the
//     two values and then (p0 + p1) + (p2 + p3);
//   - the per-row terms;
//   - a halving tree over the rows that starts at the smallest power of two >= K + 1: the levels above it would add zeros only, so
//     the result is the 256-wide tree's.
// No product is fused with an addition here, whoever compiles this: the baseline build and the AVX2 build give the same bits, and
// two calls at the same theta do.  raw[1] of a call (K, Kc) is raw[0] of a call whose K is that Kc.
SSDE_LAG_INLINE void lag_forms_sums(const LagFormArgs& A, double (*raw)[LAG_NRAW]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    static_assert(LAG_N <= 256 && LAG_N % 8 == 0, "the tree over the rows is at most 256 wide; the rows of M hold whole blocks of eight");
    const int cutv[2] = {A.K < LAG_N - 1 ? A.K : LAG_N - 1, A.Kc < LAG_N - 1 ? A.Kc : LAG_N - 1};
    const int Km = cutv[0] > cutv[1] ? cutv[0] : cutv[1];
    for (int c = 0; c < 2; c++)
        for (int j = 0; j < LAG_NRAW; j++) raw[c][j] = 0.0;
    if (Km < 0) return;
    const int K8 = (Km + 8) & ~7;                       // taps in whole blocks: <= LAG_N
    double tap[2][LAG_N];
    for (int c = 0; c < 2; c++)
        for (int k = 0; k < K8; k++) tap[c][k] = k <= cutv[c] ? A.lam[k] : 0.0;
    int P = 1;
    while (P < Km + 1) P <<= 1;
    double red[2 * LAG_NRAW][256];
    for (int j = 0; j < 2 * LAG_NRAW; j++)
        for (int i = Km + 1; i < P; i++) red[j][i] = 0.0;
    for (int i = 0; i <= Km; i++) {
        const double* m = A.M + (int64_t)i * LAG_N;     // (symmetric: row i for column i)
        lag_v4 p[2][2] = {{{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}}, {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}}};
        for (int k = 0; k < K8; k += 8) {
            lag_v4 m0, m1;
            __builtin_memcpy(&m0, m + k, 32);
            __builtin_memcpy(&m1, m + k + 4, 32);
            for (int c = 0; c < 2; c++) {
                lag_v4 l0, l1;
                __builtin_memcpy(&l0, tap[c] + k, 32);
                __builtin_memcpy(&l1, tap[c] + k + 4, 32);
                p[c][0] += m0 * l0;
                p[c][1] += m1 * l1;
            }
        }
        for (int c = 0; c < 2; c++) {
            double* r0 = &red[c * LAG_NRAW][i];          // (the row's entry of sum j: r0[j * 256])
            // (a row past the cut has li = rho = 0: every term of it is an exact zero)
            if (i > cutv[c]) { for (int j = 0; j < LAG_NRAW; j++) r0[j * 256] = 0.0; continue; }
            const lag_v4 ps = p[c][0] + p[c][1];
            const double V = (ps[0] + ps[1]) + (ps[2] + ps[3]);
            const double Lam = A.sum_lam[c];
            const double li = A.lam[i];
            double rho[3];
            for (int k = 0; k < 3; k++) rho[k] = i >= k + 1 ? A.rr[i - k - 1] : 0.0;
            double S = li * V, Ck[3] = {rho[0] * V, rho[1] * V, rho[2] * V};
            r0[4 * 256] = r0[5 * 256] = 0.0;
            for (int a = 0; a < A.d; a++) {
                const double sa = A.s[a * LAG_N + i], cm = A.cm[a];
                S -= 2.0 * Lam * cm * li * sa;
                for (int k = 0; k < 3; k++) Ck[k] -= cm * (Lam * rho[k] * sa + A.sum_rho[c][k] * li * sa);
                double su = li * sa;
                if (i == 0) {
                    S += A.n * cm * cm * Lam * Lam;
                    for (int k = 0; k < 3; k++) Ck[k] += A.n * cm * cm * Lam * A.sum_rho[c][k];
                    su -= A.n * cm * Lam;
                }
                r0[(4 + a) * 256] = su;
            }
            r0[0] = S;
            for (int k = 0; k < 3; k++) r0[(1 + k) * 256] = Ck[k];
        }
    }
    for (int w = P >> 1; w > 0; w >>= 1)
        for (int j = 0; j < 2 * LAG_NRAW; j++)
            for (int i = 0; i < w; i++) red[j][i] += red[j][i + w];
    for (int c = 0; c < 2; c++)
        for (int j = 0; j < LAG_NRAW; j++) raw[c][j] = red[c * LAG_NRAW + j][0];
}

// The same source compiled a second time for AVX2 where the host has it (four doubles per instruction instead of two); the choice is
// made once per process.  isa: 0 the baseline build, 1 the wide one (the baseline where there is none), < 0 the process's choice.
// (clang only: the pragma that keeps products and additions apart in lag_forms_sums is clang's, and without it the wide build would
//  fuse them and give other bits than the baseline.)
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__) && defined(__clang__)
inline void lag_forms_sums_base(const LagFormArgs& A, double (*raw)[LAG_NRAW]) { lag_forms_sums(A, raw); }
__attribute__((target("avx2,fma"))) inline void lag_forms_sums_avx2(const LagFormArgs& A, double (*raw)[LAG_NRAW]) { lag_forms_sums(A, raw); }
inline bool lag_forms_wide() {
    static const bool wide = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
    return wide;
}
inline void lag_forms_sums_isa(const LagFormArgs& A, double (*raw)[LAG_NRAW], int isa) {
    if (lag_forms_wide() && isa != 0) lag_forms_sums_avx2(A, raw);
    else lag_forms_sums_base(A, raw);
}
#else
inline bool lag_forms_wide() { return false; }
inline void lag_forms_sums_isa(const LagFormArgs& A, double (*raw)[LAG_NRAW], int) { lag_forms_sums(A, raw); }
#endif

#if defined(__clang__)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"     // (tf_finish asks for loops unrolled that have a run-time bound here)
#endif
// The raw sums (lag_forms_sums), the accumulators tf_finish forms from the cut K's, and the check.  One compilation of the finish
// serves every instruction set.
inline void lag_forms_host_isa(const LagFormArgs& A, LagFormOut& o, int isa) {
    lag_forms_sums_isa(A, o.raw, isa);
    for (int k = 0; k < NACC_MAX; k++) o.acc[k] = 0.0;
    const double su[2] = {o.raw[0][4], o.raw[0][5]};
    tf_finish(A.statc, A.d, A.mask, o.raw[0][0], o.raw[0][1], o.raw[0][2], o.raw[0][3], su, o.acc);     // (what the streaming lanes finish with)
    // the check: every raw sum of the two cuts, relative to itself or to sqrt(S n) (the size of a sum of n products of u with a
    // unit-scale signal), whichever is larger
    const double floor_ = std::sqrt(std::fabs(o.raw[0][0]) * A.n);
    double w = 0.0;
    for (int j = 0; j < 4 + A.d; j++) {
        const double a = o.raw[0][j], b = o.raw[1][j];
        const double sc = std::fmax(std::fmax(std::fabs(a), std::fabs(b)), floor_);
        const double r = std::fabs(a - b) / sc;
        w = (r == r) ? std::fmax(w, r) : INFINITY;
    }
    if (!(w == w)) w = INFINITY;
    o.chk = w;
}
inline void lag_forms_host(const LagFormArgs& A, LagFormOut& o) { lag_forms_host_isa(A, o, -1); }
#if defined(__clang__)
#pragma clang diagnostic pop
#endif

// ---- OU_SSM / BM_SSM (the scalar family: BasisScal of ssde_tf.hpp) ------------------------------------------------------------------
// Over the stationary rows those lanes keep S = sum u^2, S1 = sum u A1, S3 = sum u A3 and macc_a = sum u_a mx_a.  In the bulk every
// signal sig in {u, A1, A3} is sum_i tap_sig[i] z_{a,t-i} + kap_sig[a]: z the LEVEL y - ref (OU_SSM: the process is stationary around mu,
// its transfer function has no factor 1 - q^-1) or the INCREMENT y_t - y_{t-1} (BM_SSM: T = 1, u_t = (1 - k) u_{t-1} + Dy_t - mu dt);
// kap the fixed point of the same step under z == 0 (in closed form: lag_form_taps_scal).  mx has reached its fixed point mx*.  So
//     sum_t u sig = lam' M tap_sig + sum_a (kap_u[a] tap_sig' s_a + kap_sig[a] lam' s_a + n kap_u[a] kap_sig[a]),
//     su_a = sum_t u_a = lam' s_a + n kap_u[a],     macc_a = mx* su_a.
constexpr int LAG_NRAW_SCAL = 5;      // raw sums of a cut: S, S1, S3, su_1, su_2

struct LagScalArgs {
    const double* M;                  // [LAG_N][LAG_N] (host)
    const double* s;                  // [2][LAG_N] (host)
    double n;                         // bulk rows
    int K, Kc;                        // taps 0..K of the forms, 0..Kc of the check
    int d, mask;                      // response coordinates, DIR_* bits of the evaluation
    bool has_p2;                      // OU_SSM (a second scale parameter; A3 lives)
    double lam[LAG_N], t1[LAG_N], t3[LAG_N];   // responses of u, A1, A3 (as the row's products read them)
    double ku[2], k1[2], k3[2];       // the affine parts of u, A1, A3 per coordinate
    double mxs;                       // mx*: d x / d mu at its fixed point
    double statc[48];                 // the stationary constants (IsoArgs.statc): scal_tf_finish forms the accumulators from them
};

#if defined(__clang__)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"
#endif
// Fixed order: per row four partial sums over the blocks of LAG_N / 4 taps, (q0 + q1) + (q2 + q3); the per-row terms; a 256-wide
// halving tree over the rows; loops stopped at the cut.  o.raw[c][0..4] (raw[c][5] = 0).  (Forced-only and untimed: serial
// sums, a pass per cut -- not the one-pass order of lag_forms_sums.)
inline void lag_forms_scal_host(const LagScalArgs& A, LagFormOut& o) {
    static_assert(LAG_N <= 256, "the tree over the rows is 256 wide");
    constexpr int QB = LAG_N / 4, NR = LAG_NRAW_SCAL;
    double red[2 * NR][256];
    for (int j = 0; j < 2 * NR; j++)
        for (int i = 0; i < 256; i++) red[j][i] = 0.0;
    for (int c = 0; c < 2; c++) {
        const int K = c ? A.Kc : A.K;
        for (int i = 0; i <= K && i < LAG_N; i++) {
            double q[4] = {0.0, 0.0, 0.0, 0.0};
            const double* m = A.M + (int64_t)i * LAG_N;     // (symmetric: row i for column i)
            for (int b = 0; b < 4; b++) {
                const int k1 = K < (b + 1) * QB - 1 ? K : (b + 1) * QB - 1;
                double v = 0.0;
                for (int k = b * QB; k <= k1; k++) v += m[k] * A.lam[k];
                q[b] = v;
            }
            const double V = (q[0] + q[1]) + (q[2] + q[3]);
            const double li = A.lam[i], a1 = A.t1[i], a3 = A.t3[i];
            double S = li * V, S1 = a1 * V, S3 = a3 * V;
            for (int a = 0; a < A.d; a++) {
                const double sa = A.s[a * LAG_N + i], ku = A.ku[a], k1 = A.k1[a], k3 = A.k3[a];
                S += 2.0 * ku * li * sa;
                S1 += (ku * a1 + k1 * li) * sa;
                S3 += (ku * a3 + k3 * li) * sa;
                double su = li * sa;
                if (i == 0) {
                    S += A.n * ku * ku;
                    S1 += A.n * ku * k1;
                    S3 += A.n * ku * k3;
                    su += A.n * ku;
                }
                red[c * NR + 3 + a][i] = su;
            }
            red[c * NR + 0][i] = S; red[c * NR + 1][i] = S1; red[c * NR + 2][i] = S3;
        }
    }
    for (int w = 128; w > 0; w >>= 1)
        for (int j = 0; j < 2 * NR; j++)
            for (int i = 0; i < w; i++) red[j][i] += red[j][i + w];
    for (int c = 0; c < 2; c++) {
        for (int j = 0; j < NR; j++) o.raw[c][j] = red[c * NR + j][0];
        o.raw[c][NR] = 0.0;
    }
    for (int k = 0; k < NACC_MAX; k++) o.acc[k] = 0.0;
    const double macc[2] = {A.mxs * o.raw[0][3], A.mxs * o.raw[0][4]};
    scal_tf_finish(A.statc[0], A.statc + 10, A.statc + 13, A.d, A.mask, A.has_p2, o.raw[0][0], o.raw[0][1], o.raw[0][2], macc, o.acc);   // (what the streaming lanes finish with)
    // the check: as lag_forms_host
    const double floor_ = std::sqrt(std::fabs(o.raw[0][0]) * A.n);
    double w = 0.0;
    for (int j = 0; j < 3 + A.d; j++) {
        const double a = o.raw[0][j], b = o.raw[1][j];
        const double sc = std::fmax(std::fmax(std::fabs(a), std::fabs(b)), floor_);
        const double r = std::fabs(a - b) / sc;
        w = (r == r) ? std::fmax(w, r) : INFINITY;
    }
    if (!(w == w)) w = INFINITY;
    o.chk = w;
}
#if defined(__clang__)
#pragma clang diagnostic pop
#endif

}  // namespace ssde
