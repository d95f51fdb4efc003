// ssde_smooth.hpp -- fixed-interval Kalman smoother (ssde_smooth): the per-lane math both routes share.
//
// Forward: smooth_record_row writes what the filter forms at one state row j BEFORE dense_step advances
// the lane: the prediction a_j, P_j, and -- on rows with an update -- the innovation v_j, F_j^-1, the gain K_j and the
// whitened innovation C_j^-1 v_j; on rows without one v, F^-1 and K are 0 (so L_j = T_j) and the residual is NaN.  The two
// coefficients of T_j (t12, e: makeT of the three families) close the record.  Backward: smooth_back_row is one step of
// the de Jong / Durbin-Koopman recursion over such a record.  `rec(k)` addresses double k of the row's record, whatever
// layout the kernel keeps it in (k_smooth.hip: time-major, lane-coalesced).
#ifndef SSDE_SMOOTH_HPP
#define SSDE_SMOOTH_HPP

#include "ssde_dense.hpp"

namespace ssde {

template <int MODEL, int D>
struct SmoothRec {
    static constexpr int SD = DenseDims<MODEL, D>::SD;
    static constexpr int NP = SD * (SD + 1) / 2, NF = D * (D + 1) / 2;
    static constexpr int A = 0, P = SD, V = P + NP, FI = V + D, K = FI + NF, T = K + SD * D, E = T + 2;
    static constexpr int R = E + D;                          // doubles per row (CTCRW, d = 2: 31)
    SSDE_HD static constexpr int up(int r, int c) { return r <= c ? c * (c + 1) / 2 + r : r * (r + 1) / 2 + c; }
};

// makeT's two coefficients over dt as smooth_record_row forms them below: CTCRW [[1, t12], [0, e]] per dimension, OU e I, BM I.  For
// the bridges of ssde_predict_draws (ssde_bridge.hpp).  smooth_record_row and predict_query_row keep their own lines: routing them
// through this function changes predict_query_kernel's register allocation, and their kernels stay as they are.
template <int MODEL, int D>
SSDE_HD void smooth_trans_coef(const DualN<0>* par, double dt, double& t12, double& e) {
    t12 = 0.0; e = 1.0;
    if (MODEL == M_CTCRW) {
        const double tau = exp(par[D].v), beta = 1.0 / tau;
        e = exp(-(beta * dt));
        t12 = (1.0 - e) / beta;
    } else if (MODEL == M_OU_SSM) {
        e = exp(-dt / exp(par[D].v));
    }
}

// The row's record, from the lane's state before dense_step.  par / H as dense_step takes them (values only).  Returns whether the
// row takes an update (false: a NA row, or det F <= 0 -- what ssde_predict's side row tells apart).
template <int MODEL, int D, class W>
SSDE_HD bool smooth_record_row(const DenseLane<MODEL, D, 0>& L, const DualN<0>* par, const DualN<0> (&H)[D][D], double dt,
                               const double* y, bool na, W&& rec) {
    typedef DenseDims<MODEL, D> DM;
    typedef SmoothRec<MODEL, D> RC;
    constexpr int SD = DM::SD;
    typedef DualN<0> T_;
    SSDE_DLOOP for (int r = 0; r < SD; r++) rec(RC::A + r) = L.a[r].v;
    SSDE_DLOOP for (int c = 0; c < SD; c++)
        SSDE_DLOOP for (int r = 0; r <= c; r++) rec(RC::P + RC::up(r, c)) = L.P[r][c].v;
    // makeT: CTCRW [[1, t12], [0, e]] per dimension, OU e I, BM I (the same formulas as dense_step_g)
    double t12 = 0.0, e = 1.0;
    if (MODEL == M_CTCRW) {
        const double tau = exp(par[D].v), beta = 1.0 / tau;
        e = exp(-(beta * dt));
        t12 = (1.0 - e) / beta;
    } else if (MODEL == M_OU_SSM) {
        e = exp(-dt / exp(par[D].v));
    }
    rec(RC::T) = t12;
    rec(RC::T + 1) = e;
    // the measurement: the update decision exactly as dense_step_g takes it
    bool upd = !na;
    T_ F[D][D], det(1.0);
    if (upd) {
        SSDE_DLOOP for (int i = 0; i < D; i++)
            SSDE_DLOOP for (int j = 0; j < D; j++) F[i][j] = L.P[DM::z(i)][DM::z(j)] + H[i][j];
        if constexpr (D == 1) det = F[0][0];
        else if constexpr (D == 2) det = F[0][0] * F[1][1] - F[1][0] * F[0][1];
        else det = dfabs(dense_det_lu<D, T_>(F));
        upd = (MODEL == M_CTCRW) ? !(det.v <= 0.0) : !(fabs(det.v) <= 0.0);
    }
    if (!upd) {
        SSDE_DLOOP for (int i = 0; i < D; i++) rec(RC::V + i) = 0.0;
        SSDE_DLOOP for (int k = 0; k < RC::NF; k++) rec(RC::FI + k) = 0.0;
        SSDE_DLOOP for (int k = 0; k < SD * D; k++) rec(RC::K + k) = 0.0;
        SSDE_DLOOP for (int i = 0; i < D; i++) rec(RC::E + i) = __builtin_nan("");
        return false;
    }
    T_ Fi[D][D];
    if constexpr (D == 1) {
        Fi[0][0] = 1.0 / F[0][0];
    } else if constexpr (D > 2) {
        dense_inverse_lu<D, T_>(F, Fi);
    } else {
        const T_ id = 1.0 / det;
        Fi[0][0] = F[1][1] * id; Fi[0][1] = -(F[0][1] * id);
        Fi[1][0] = -(F[1][0] * id); Fi[1][1] = F[0][0] * id;
    }
    double v[D];
    SSDE_DLOOP for (int i = 0; i < D; i++) { v[i] = y[i] - L.a[DM::z(i)].v; rec(RC::V + i) = v[i]; }
    SSDE_DLOOP for (int c = 0; c < D; c++)
        SSDE_DLOOP for (int r = 0; r <= c; r++) rec(RC::FI + RC::up(r, c)) = 0.5 * (Fi[r][c].v + Fi[c][r].v);
    // K = T P Z' F^-1 (dense_step_g's product, T applied to the rows of P)
    SSDE_DLOOP for (int r = 0; r < SD; r++)
        SSDE_DLOOP for (int j = 0; j < D; j++) {
            double s = 0.0;
            SSDE_DLOOP for (int i = 0; i < D; i++) {
                double tp;
                if (MODEL == M_CTCRW) tp = (r & 1) ? e * L.P[r][DM::z(i)].v : L.P[r][DM::z(i)].v + t12 * L.P[r + 1][DM::z(i)].v;
                else tp = e * L.P[r][DM::z(i)].v;
                s += tp * Fi[i][j].v;
            }
            rec(RC::K + r + SD * j) = s;
        }
    // whitened innovation C^-1 v, C the lower Cholesky factor of (the symmetric part of) F
    double C[D][D];
    SSDE_DLOOP for (int j = 0; j < D; j++) {
        double s = F[j][j].v;
        SSDE_DLOOP for (int k = 0; k < j; k++) s -= C[j][k] * C[j][k];
        C[j][j] = sqrt(s);
        SSDE_DLOOP for (int i = j + 1; i < D; i++) {
            double t = 0.5 * (F[i][j].v + F[j][i].v);
            SSDE_DLOOP for (int k = 0; k < j; k++) t -= C[i][k] * C[j][k];
            C[i][j] = t / C[j][j];
        }
    }
    SSDE_DLOOP for (int i = 0; i < D; i++) {
        double s = v[i];
        SSDE_DLOOP for (int k = 0; k < i; k++) s -= C[i][k] * v[k];
        v[i] = s / C[i][i];                       // (in place: v[k < i] already hold the whitened values)
        rec(RC::E + i) = v[i];
    }
    return true;
}

// Backward step over row j's record: r <- Z'F^-1 v + L'r, N <- Z'F^-1 Z + L'N L (L = T - K Z), then the smoothed mean / covariance
// a + P r, P - P N P.  tail: row j is the track's last (r = N = 0 before it: T_j and K_j there are not read).
template <int MODEL, int D, int SD, class G>
SSDE_HD void smooth_back_row(double (&r)[SD], double (&N)[SD][SD], bool tail, G&& rec, double (&am)[SD], double (&V)[SD][SD]) {
    typedef DenseDims<MODEL, D> DM;
    typedef SmoothRec<MODEL, D> RC;
    static_assert(SD == DM::SD, "state dimension");
    double Fi[D][D], u[D];
    SSDE_DLOOP for (int i = 0; i < D; i++)
        SSDE_DLOOP for (int j = 0; j < D; j++) Fi[i][j] = rec(RC::FI + RC::up(i, j));
    SSDE_DLOOP for (int i = 0; i < D; i++) {
        double s = 0.0;
        SSDE_DLOOP for (int j = 0; j < D; j++) s += Fi[i][j] * rec(RC::V + j);
        u[i] = s;                                                   // F^-1 v
    }
    if (tail) {
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
        // r <- T'r + Z'(F^-1 v - K'r)
        double w[D];
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
        // M = N L = N T - (N K) Z, then N <- T'M - Z'(K'M) + Z'F^-1 Z
        double NK[SD][D];
        SSDE_DLOOP for (int a = 0; a < SD; a++)
            SSDE_DLOOP for (int j = 0; j < D; j++) {
                double s = 0.0;
                SSDE_DLOOP for (int b = 0; b < SD; b++) s += N[a][b] * K[b][j];
                NK[a][j] = s;
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
    // a^ = a + P r, V = P - P N P
    double P[SD][SD];
    SSDE_DLOOP for (int a = 0; a < SD; a++)
        SSDE_DLOOP for (int b = 0; b < SD; b++) P[a][b] = rec(RC::P + RC::up(a, b));
    SSDE_DLOOP for (int a = 0; a < SD; a++) {
        double s = rec(RC::A + a);
        SSDE_DLOOP for (int b = 0; b < SD; b++) s += P[a][b] * r[b];
        am[a] = s;
    }
    double PN[SD][SD];
    SSDE_DLOOP for (int a = 0; a < SD; a++)
        SSDE_DLOOP for (int b = 0; b < SD; b++) {
            double s = 0.0;
            SSDE_DLOOP for (int c = 0; c < SD; c++) s += P[a][c] * N[c][b];
            PN[a][b] = s;
        }
    SSDE_DLOOP for (int a = 0; a < SD; a++)
        SSDE_DLOOP for (int b = a; b < SD; b++) {
            double s = 0.0, t = 0.0;
            SSDE_DLOOP for (int c = 0; c < SD; c++) { s += PN[a][c] * P[c][b]; t += PN[b][c] * P[c][a]; }
            const double m = P[a][b] - 0.5 * (s + t);
            V[a][b] = m; V[b][a] = m;
        }
}

}  // namespace ssde
#endif
