// ssde_lagstats.hpp -- the bulk of a stationary batch from lag statistics.
//
// Past the covariance transient the CTCRW filter on a regular grid is linear and time-invariant in the increments
// dy_t = y_t - y_{t-1} - mu dt (ssde_tf.hpp): the innovation and the r signal of the transfer-function lanes are
//     u_t = sum_i lam_i dy_{t-i},     r_{t-k} = sum_i rr_{i-k} dy_{t-i},
// with impulse responses that decay like rho^i.  Cut at K taps (the warm-up the window plan asks for), every sum the stationary
// lanes accumulate over rows t >= A (S = sum u^2, C_k = sum u r_{t-k}, su = sum u) is a quadratic or linear form in the data with
// coefficients that depend on theta only through the taps:
//     sum_t u_t v_t = lam' M v - ...  (the mu dt terms: s and n below),
// where, per batch (summed over tracks, and over the response coordinates for M),
//     M_ik = sum_{t = A}^{n - 1} Dy_{t-i} Dy_{t-k},   s_{a,i} = sum_{t = A}^{n - 1} Dy_{a, t-i},   n = rows past A,
// Dy = y_t - y_{t-1}.  M is built at create as Toeplitz lag sums plus the corrections at the bulk's two ends:
//     M_{i, i+l} = Q_l + sum_{m < i} (h_m h_{m+l} - g_m g_{m+l}),    Q_l = sum_{t = A}^{n - 1} Dy_t Dy_{t-l},
// h_j = Dy_{A-1-j} (head), g_j = Dy_{n-1-j} (tail); s telescopes: s_{a,i} = y_{n-1-i} - y_{A-1-i}.
#pragma once
#include <stdint.h>

namespace ssde {

constexpr int LAG_N = 192;            // taps held: K_max + 1
constexpr int LAG_KMAX = LAG_N - 1;   // the longest cut an evaluation may ask for
constexpr int LAG_A = 256;            // first bulk row (multiple of WIN_ALIGN); rows [0, LAG_A) of every track are streamed
constexpr int LAG_CHECK = 16;         // the bulk's check: the same forms with this many taps fewer
constexpr int LAG_LB = 32;            // lags per work item of the Toeplitz pass (k_lagstats.hip)
static_assert(LAG_A > LAG_N, "the head and the lag window of the first bulk row must lie inside the track");
static_assert(LAG_N % LAG_LB == 0 && LAG_N % 64 == 0, "lag blocks");

// M (LAG_N x LAG_N, symmetric) from the Toeplitz sums Q[l] and D[p * LAG_N + q] = sum (h_p h_q - g_p g_q); fixed order
inline void lag_assemble(const double* Q, const double* D, double* M) {
    for (int l = 0; l < LAG_N; l++) {
        double run = Q[l];
        for (int i = 0; i + l < LAG_N; i++) {
            M[(int64_t)i * LAG_N + i + l] = M[(int64_t)(i + l) * LAG_N + i] = run;
            run += D[(int64_t)i * LAG_N + i + l];
        }
    }
}

// The same statistics on the host, track by track (the CPU reference of ssde_lagstats_host): y[track][row][coordinate] with
// rows[track] rows each, stored one track after the other.  Q, D accumulate over tracks and coordinates, s[a][i] per coordinate.
inline void lag_track_stats(const double* y, int rows, int d, double* Q, double* D, double* s) {
    const int n = rows;
    if (n <= LAG_A) return;
    auto Y = [&](int t, int a) { return y[(int64_t)t * d + a]; };
    auto Dy = [&](int t, int a) { return Y(t, a) - Y(t - 1, a); };
    for (int a = 0; a < d; a++) {
        for (int l = 0; l < LAG_N; l++) {
            double q = 0.0;
            for (int t = LAG_A; t < n; t++) q += Dy(t, a) * Dy(t - l, a);
            Q[l] += q;
        }
        for (int p = 0; p < LAG_N; p++)
            for (int q = 0; q < LAG_N; q++)
                D[(int64_t)p * LAG_N + q] += Dy(LAG_A - 1 - p, a) * Dy(LAG_A - 1 - q, a) - Dy(n - 1 - p, a) * Dy(n - 1 - q, a);
        for (int i = 0; i < LAG_N; i++) s[a * LAG_N + i] += Y(n - 1 - i, a) - Y(LAG_A - 1 - i, a);
    }
}

// ---- early cuts (CTCRW) ----------------------------------------------------------------------------------------------------------
// The same statistics with the first bulk row A' < LAG_A: every multiple of LAG_CUT_STEP (= WIN_ALIGN) from LAG_CUT_MIN to LAG_CUT_MAX,
// for lags i, k < A' (no evaluation asks for more: K <= A' - s_stat).  A track with n <= A' contributes nothing, one with
// A' < n <= LAG_A its rows [A', n).  They are the late statistics plus the head rows' own contribution,
//     M(A') = M(LAG_A) + M~(A'),   M~(A')_ik = sum_{t = A'}^{min(n, LAG_A) - 1} Dy_{t-i} Dy_{t-k}
// (s and n alike), and M~(A') is the definition above applied to the tracks CUT OFF after LAG_A rows: Toeplitz sums over
// [A', min(n, LAG_A)) and the end terms h_j = Dy_{A'-1-j}, g_j = Dy_{min(n, LAG_A)-1-j}.  Entries with a lag >= A' are zero.
constexpr int LAG_CUT_MIN = 32, LAG_CUT_MAX = 128, LAG_CUT_STEP = 16;
constexpr int LAG_NCUT = (LAG_CUT_MAX - LAG_CUT_MIN) / LAG_CUT_STEP + 1;
static_assert(LAG_CUT_MAX < LAG_A && LAG_CUT_MAX <= LAG_N && LAG_CUT_MIN % LAG_CUT_STEP == 0, "early cuts");
// index of an early cut, -1 where A' is none
inline int lag_cut_index(int cut) {
    return (cut >= LAG_CUT_MIN && cut <= LAG_CUT_MAX && cut % LAG_CUT_STEP == 0) ? (cut - LAG_CUT_MIN) / LAG_CUT_STEP : -1;
}
// bit c set: cut LAG_CUT_MIN + c LAG_CUT_STEP (what the window policy reads: ssde_windows.hpp)
constexpr unsigned LAG_CUT_ALL = (1u << LAG_NCUT) - 1u;

// lag_track_stats with the first bulk row `cut` and the track cut off after `cap` rows (cap >= n: the whole track): Q[l], D[p][q], s[a][i]
// for l, i < cut and p, q <= cut - 2, the other entries untouched.  Returns the bulk rows of the track.
inline int lag_track_stats_cut(const double* y, int rows, int d, int cut, int cap, double* Q, double* D, double* s) {
    const int n = rows < cap ? rows : cap;
    if (n <= cut) return 0;
    auto Y = [&](int t, int a) { return y[(int64_t)t * d + a]; };
    auto Dy = [&](int t, int a) { return Y(t, a) - Y(t - 1, a); };
    const int nl = cut < LAG_N ? cut : LAG_N;
    for (int a = 0; a < d; a++) {
        for (int l = 0; l < nl; l++) {
            double q = 0.0;
            for (int t = cut; t < n; t++) q += Dy(t, a) * Dy(t - l, a);
            Q[l] += q;
        }
        for (int p = 0; p + 2 <= cut && p < LAG_N; p++)
            for (int q = 0; q + 2 <= cut && q < LAG_N; q++)
                D[(int64_t)p * LAG_N + q] += Dy(cut - 1 - p, a) * Dy(cut - 1 - q, a) - Dy(n - 1 - p, a) * Dy(n - 1 - q, a);
        for (int i = 0; i < nl; i++) s[a * LAG_N + i] += Y(n - 1 - i, a) - Y(cut - 1 - i, a);
    }
    return n - cut;
}

// M of an early cut from its Q and D (lag_assemble's order), entries with a lag >= cut zero
inline void lag_assemble_cut(const double* Q, const double* D, int cut, double* M) {
    for (int64_t e = 0; e < (int64_t)LAG_N * LAG_N; e++) M[e] = 0.0;
    const int nl = cut < LAG_N ? cut : LAG_N;
    for (int l = 0; l < nl; l++) {
        double run = Q[l];
        for (int i = 0; i + l < nl; i++) {
            M[(int64_t)i * LAG_N + i + l] = M[(int64_t)(i + l) * LAG_N + i] = run;
            run += D[(int64_t)i * LAG_N + i + l];
        }
    }
}

// OU_SSM (stationary around mu: no factor 1 - q^-1 to take on the data) needs the same statistics of the LEVELS z_{a,t} = y_{a,t} - ref_a
// instead of the increments; ref_a is one number per coordinate, fixed at create near the data (the handle's: the observation at
// row LAG_A - 1 of the first track in tiled order that has a bulk), so that z stays within a few process standard deviations.  The
// Toeplitz-plus-end-corrections identity holds for any sequence (h_j = z_{A-1-j}, g_j = z_{n-1-j}); s no longer telescopes:
//     s_{a,0} = sum_{t >= A} z_{a,t},     s_{a,i+1} = s_{a,i} + h_{a,i} - g_{a,i}.
// e[a][i] = sum over tracks of (h_{a,i} - g_{a,i}), s0[a] = sum over tracks of s_{a,0}  ->  s[a][i]; fixed order
inline void lag_levels_s(const double* s0, const double* e, double* s) {
    for (int a = 0; a < 2; a++) {
        double run = s0[a];
        for (int i = 0; i < LAG_N; i++) {
            s[a * LAG_N + i] = run;
            run += e[a * LAG_N + i];
        }
    }
}

// lag_track_stats for the levels y - ref: Q, D as there; e[a][i] and s0[a] as lag_levels_s takes them
inline void lag_track_stats_levels(const double* y, int rows, int d, const double* ref, double* Q, double* D, double* e, double* s0) {
    const int n = rows;
    if (n <= LAG_A) return;
    for (int a = 0; a < d; a++) {
        auto Z = [&](int t) { return y[(int64_t)t * d + a] - ref[a]; };
        for (int l = 0; l < LAG_N; l++) {
            double q = 0.0;
            for (int t = LAG_A; t < n; t++) q += Z(t) * Z(t - l);
            Q[l] += q;
        }
        for (int p = 0; p < LAG_N; p++)
            for (int q = 0; q < LAG_N; q++)
                D[(int64_t)p * LAG_N + q] += Z(LAG_A - 1 - p) * Z(LAG_A - 1 - q) - Z(n - 1 - p) * Z(n - 1 - q);
        for (int i = 0; i < LAG_N; i++) e[a * LAG_N + i] += Z(LAG_A - 1 - i) - Z(n - 1 - i);
        double z0 = 0.0;
        for (int t = LAG_A; t < n; t++) z0 += Z(t);
        s0[a] += z0;
    }
}

// (the per-evaluation forms built from M, s and n: ssde_lagforms.hpp, on the host)

}  // namespace ssde
