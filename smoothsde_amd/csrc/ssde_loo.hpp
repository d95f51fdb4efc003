// ssde_loo.hpp -- leave-one-out residuals and predictive densities (ssde_smooth_loo): the per-lane math, DESIGN.md §3.20.
//
// The smoother's backward recursion (ssde_smooth.hpp: smooth_back_row) carries r, N from a track's last state row to its first.
// With r, N the values BEFORE row j is folded in, the smoothing error w_j = F_j^-1 v_j - K_j'r and its precision
// M_j = F_j^-1 + K_j'N K_j are the diagonal blocks of Sigma_yy^-1 (y - m) and of Sigma_yy^-1 of the track's joint Gaussian, so
// y_j | y_-j ~ N(y_j - M_j^-1 w_j, M_j^-1) (de Jong 1989).  loo_back_row forms them from the row's record and the incoming (r, N),
// then advances (r, N) with the expressions of smooth_back_row, in its order; it never reads the predicted covariance RC::P, nor the
// state columns of RC::A the measurement does not see.  loo_fold / loo_finish reduce a track's rows to its statistics.
// Host- and device-compilable; every loop has a constant trip count.
#ifndef SSDE_LOO_HPP
#define SSDE_LOO_HPP

#include <math.h>
#include <stdint.h>

#include "../../include/ssde.h"      // SSDE_LOO_MAX_THR: the one definition
#include "ssde_smooth.hpp"

#if defined(__clang__)
#define SSDE_LLOOP _Pragma("unroll")
#else
#define SSDE_LLOOP
#endif

namespace ssde {

constexpr int LOO_NTHR = SSDE_LOO_MAX_THR;
constexpr int LOO_NSTAT_MAX = 4 + LOO_NTHR;

SSDE_HD bool loo_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }       // neither NaN nor +-inf

// One row's results.  served: the record took an update (no component of its whitened innovation is NaN) and M is positive
// definite (every pivot of its Cholesky factor > 0 and finite); mean, cov mean something only then.  white: D = M^-1 has a
// Cholesky factor as well (every pivot > 0 and finite); z, q, lpd mean something only then.
template <int D>
struct LooRow {
    double mean[D], cov[D][D], z[D], q, lpd;
    bool served, white;
};

// lower Cholesky factor of the symmetric S (its lower triangle is read); false where a pivot is <= 0 or not finite (C is then not
// to be used)
template <int D>
SSDE_HD bool loo_cholesky(const double (&S)[D][D], double (&C)[D][D]) {
    bool ok = true;
    SSDE_DLOOP for (int j = 0; j < D; j++) {
        double s = S[j][j];
        SSDE_DLOOP for (int k = 0; k < j; k++) s -= C[j][k] * C[j][k];
        ok = ok && s > 0.0 && loo_finite(s);
        C[j][j] = sqrt(s);
        SSDE_DLOOP for (int i = j + 1; i < D; i++) {
            double t = S[i][j];
            SSDE_DLOOP for (int k = 0; k < j; k++) t -= C[i][k] * C[j][k];
            C[i][j] = t / C[j][j];
        }
    }
    return ok;
}

// Row j's deletion quantities from the incoming (r, N), then (r, N) advanced over row j's record exactly as smooth_back_row does.
// tail: row j is the track's last (r = N = 0 before it: T_j and K_j there are not read).
template <int MODEL, int D, int SD, class G>
SSDE_HD void loo_back_row(double (&r)[SD], double (&N)[SD][SD], bool tail, G&& rec, LooRow<D>& o) {
    typedef DenseDims<MODEL, D> DM;
    typedef SmoothRec<MODEL, D> RC;
    static_assert(SD == DM::SD, "state dimension");
    double Fi[D][D], u[D], w[D], M[D][D];
    SSDE_DLOOP for (int i = 0; i < D; i++)
        SSDE_DLOOP for (int j = 0; j < D; j++) Fi[i][j] = rec(RC::FI + RC::up(i, j));
    SSDE_DLOOP for (int i = 0; i < D; i++) {
        double s = 0.0;
        SSDE_DLOOP for (int j = 0; j < D; j++) s += Fi[i][j] * rec(RC::V + j);
        u[i] = s;                                                   // F^-1 v
    }
    if (tail) {
        SSDE_DLOOP for (int i = 0; i < D; i++) {
            w[i] = u[i];
            SSDE_DLOOP for (int j = 0; j < D; j++) M[i][j] = Fi[i][j];
        }
        SSDE_DLOOP for (int a = 0; a < SD; a++) {
            r[a] = 0.0;
            SSDE_DLOOP for (int b = 0; b < SD; b++) N[a][b] = 0.0;
        }
        SSDE_DLOOP for (int i = 0; i < D; i++) {
            r[DM::z(i)] = u[i];
            SSDE_DLOOP for (int j = 0; j < D; j++) N[DM::z(i)][DM::z(j)] = Fi[i][j];
        }
    } else {
        const double t12 = rec(RC::T), e = rec(RC::T + 1);
        double K[SD][D];
        SSDE_DLOOP for (int a = 0; a < SD; a++)
            SSDE_DLOOP for (int j = 0; j < D; j++) K[a][j] = rec(RC::K + a + SD * j);
        // w = F^-1 v - K'r (the incoming r), then r <- T'r + Z'w
        SSDE_DLOOP for (int j = 0; j < D; j++) {
            double s = u[j];
            SSDE_DLOOP for (int a = 0; a < SD; a++) s -= K[a][j] * r[a];
            w[j] = s;
        }
        if (MODEL == M_CTCRW) {
            SSDE_DLOOP for (int a = 0; a < SD; a += 2) r[a + 1] = t12 * r[a] + e * r[a + 1];
        } else {
            SSDE_DLOOP for (int a = 0; a < SD; a++) r[a] = e * r[a];
        }
        SSDE_DLOOP for (int j = 0; j < D; j++) r[DM::z(j)] += w[j];
        // N K of the incoming N: M = F^-1 + K'(N K); then N <- T'(N L) - Z'(K'(N L)) + Z'F^-1 Z, L = T - K Z
        double NK[SD][D];
        SSDE_DLOOP for (int a = 0; a < SD; a++)
            SSDE_DLOOP for (int j = 0; j < D; j++) {
                double s = 0.0;
                SSDE_DLOOP for (int b = 0; b < SD; b++) s += N[a][b] * K[b][j];
                NK[a][j] = s;
            }
        SSDE_DLOOP for (int i = 0; i < D; i++)
            SSDE_DLOOP for (int j = 0; j < D; j++) {
                double s = Fi[i][j];
                SSDE_DLOOP for (int a = 0; a < SD; a++) s += K[a][i] * NK[a][j];
                M[i][j] = s;
            }
        SSDE_DLOOP for (int a = 0; a < SD; a++) {
            if (MODEL == M_CTCRW) {
                SSDE_DLOOP for (int b = 0; b < SD; b += 2) N[a][b + 1] = t12 * N[a][b] + e * N[a][b + 1];
            } else {
                SSDE_DLOOP for (int b = 0; b < SD; b++) N[a][b] = e * N[a][b];
            }
            SSDE_DLOOP for (int j = 0; j < D; j++) N[a][DM::z(j)] -= NK[a][j];
        }
        double KM[D][SD];
        SSDE_DLOOP for (int j = 0; j < D; j++)
            SSDE_DLOOP for (int b = 0; b < SD; b++) {
                double s = 0.0;
                SSDE_DLOOP for (int a = 0; a < SD; a++) s += K[a][j] * N[a][b];
                KM[j][b] = s;
            }
        SSDE_DLOOP for (int b = 0; b < SD; b++) {
            if (MODEL == M_CTCRW) {
                SSDE_DLOOP for (int a = 0; a < SD; a += 2) N[a + 1][b] = t12 * N[a][b] + e * N[a + 1][b];
            } else {
                SSDE_DLOOP for (int a = 0; a < SD; a++) N[a][b] = e * N[a][b];
            }
            SSDE_DLOOP for (int j = 0; j < D; j++) N[DM::z(j)][b] -= KM[j][b];
        }
        SSDE_DLOOP for (int i = 0; i < D; i++)
            SSDE_DLOOP for (int j = 0; j < D; j++) N[DM::z(i)][DM::z(j)] += Fi[i][j];
        SSDE_DLOOP for (int a = 0; a < SD; a++)
            SSDE_DLOOP for (int b = a + 1; b < SD; b++) {
                const double m = 0.5 * (N[a][b] + N[b][a]);
                N[a][b] = m; N[b][a] = m;
            }
    }
    // the deletion quantities of row j
    bool upd = true;
    SSDE_DLOOP for (int i = 0; i < D; i++) upd = upd && !(rec(RC::E + i) != rec(RC::E + i));
    SSDE_DLOOP for (int i = 0; i < D; i++)
        SSDE_DLOOP for (int j = i + 1; j < D; j++) {
            const double m = 0.5 * (M[i][j] + M[j][i]);
            M[i][j] = m; M[j][i] = m;
        }
    double C[D][D];
    o.served = loo_cholesky<D>(M, C) && upd;
    o.white = false;
    o.q = 0.0; o.lpd = 0.0;
    if (!o.served) return;
    // Dm = M^-1 as smooth_record_row inverts F: closed form for d <= 2, partial-pivot LU above; symmetrised
    double Dm[D][D];
    if constexpr (D == 1) {
        Dm[0][0] = 1.0 / M[0][0];
    } else if constexpr (D == 2) {
        const double id = 1.0 / (M[0][0] * M[1][1] - M[1][0] * M[0][1]);
        Dm[0][0] = M[1][1] * id; Dm[1][1] = M[0][0] * id;
        Dm[0][1] = -(M[0][1] * id); Dm[1][0] = Dm[0][1];
    } else {
        DualN<0> Md[D][D], Mi[D][D];
        SSDE_DLOOP for (int i = 0; i < D; i++)
            SSDE_DLOOP for (int j = 0; j < D; j++) Md[i][j] = DualN<0>(M[i][j]);
        dense_inverse_lu<D, DualN<0>>(Md, Mi);
        SSDE_DLOOP for (int i = 0; i < D; i++)
            SSDE_DLOOP for (int j = i; j < D; j++) {
                const double m = 0.5 * (Mi[i][j].v + Mi[j][i].v);
                Dm[i][j] = m; Dm[j][i] = m;
            }
    }
    double dl[D];
    SSDE_DLOOP for (int i = 0; i < D; i++) {
        double s = 0.0;
        SSDE_DLOOP for (int j = 0; j < D; j++) s += Dm[i][j] * w[j];
        dl[i] = s;                                                  // delta = D w
        o.mean[i] = (rec(RC::A + DM::z(i)) + rec(RC::V + i)) - s;
        SSDE_DLOOP for (int j = 0; j < D; j++) o.cov[i][j] = Dm[i][j];
    }
    o.white = loo_cholesky<D>(Dm, C);
    if (!o.white) return;
    double q = 0.0, ld = 0.0;
    SSDE_DLOOP for (int i = 0; i < D; i++) {
        double s = dl[i];
        SSDE_DLOOP for (int k = 0; k < i; k++) s -= C[i][k] * o.z[k];
        o.z[i] = s / C[i][i];
        q += o.z[i] * o.z[i];
        ld += log(C[i][i]);
    }
    o.q = q;
    o.lpd = -0.5 * ((double)D * 1.8378770664093454835606594728112 + 2.0 * ld + q);
}

// a track's statistics, folded row by row in the walk's order (the track's last row first)
struct LooAcc {
    double lsum, qmax, qrow;
    int rows, over[LOO_NTHR];
};

SSDE_HD void loo_init(LooAcc& a) {
    a.lsum = 0.0; a.qmax = 0.0; a.qrow = 0.0; a.rows = 0;
    SSDE_LLOOP for (int k = 0; k < LOO_NTHR; k++) a.over[k] = 0;
}

// a served row with a Cholesky factor, at the caller's row crow.  Replacing the maximum on >= in a walk that runs from the last
// row to the first leaves the SMALLEST row of a tie (ssde_path_speed's convention).
template <class G>
SSDE_HD void loo_fold(LooAcc& a, double q, double lpd, int64_t crow, G&& thr, int n_thr) {
    a.lsum += lpd;
    if (a.rows == 0 || q >= a.qmax) { a.qmax = q; a.qrow = (double)crow; }
    a.rows++;
    SSDE_LLOOP for (int k = 0; k < LOO_NTHR; k++)
        if (k < n_thr && q > thr(k)) a.over[k]++;
}

// out[0 .. 4 + n_thr): the served rows, the sum of lpd, the largest q and its row (NaN without a served row), the counts; elements
// past 4 + n_thr are set to 0 and mean nothing
SSDE_HD void loo_finish(const LooAcc& a, int n_thr, double (&out)[LOO_NSTAT_MAX]) {
    const double qn = __builtin_nan("");
    out[0] = (double)a.rows;
    out[1] = a.lsum;
    out[2] = a.rows ? a.qmax : qn;
    out[3] = a.rows ? a.qrow : qn;
    SSDE_LLOOP for (int k = 0; k < LOO_NTHR; k++) out[4 + k] = k < n_thr ? (double)a.over[k] : 0.0;
}

}  // namespace ssde
#endif
