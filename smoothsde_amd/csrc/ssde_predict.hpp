// ssde_predict.hpp -- the state at any time from the smoother's records (ssde_predict): the per-lane math, DESIGN.md §3.11.
//
// A query (row j, offset delta) is the smoothed state of a NA row inserted at t_j + delta that carries row j's parameters.  The
// backward walk (k_predict.hip) stops at every wanted state row and predict_packet_row stores what the query needs of it in a
// packet: the filtered moments a_f, P_f of the row's record, the r and N the recursion holds BEFORE the row is processed (those of
// the interval's right end; zeros at a track's last row), the row's linear predictors and its interval.  predict_query_row is the
// rest: one prediction step over delta (dense_step, na = true) and the correction by T2 = T(Delta - delta), r+ and N+.
// `pk(k)` addresses double k of a packet, whatever layout the kernel keeps it in.
#ifndef SSDE_PREDICT_HPP
#define SSDE_PREDICT_HPP

#include "ssde_smooth.hpp"

namespace ssde {

// relative slack on delta <= Delta: offsets and intervals are differences of time stamps, a lattice residual one more subtraction
constexpr double PREDICT_DT_RTOL = 1e-9;
constexpr double PREDICT_DT_TAIL = -1.0;                     // the packet's interval at a track's last row (forecast: any delta)

template <int MODEL, int D>
struct PredictPk {
    static constexpr int SD = DenseDims<MODEL, D>::SD, Q = DenseDims<MODEL, D>::Q;
    static constexpr int NP = SD * (SD + 1) / 2;
    static constexpr int AF = 0, PF = SD, R = PF + NP, N = R + SD, PAR = N + NP, DT = PAR + Q;
    static constexpr int SZ = DT + 1;                        // doubles per packet (CTCRW, d = 2: 33)
    static constexpr int SW = Q + 1;                         // the record pass's side row: the linear predictors, then the interval
    SSDE_HD static constexpr int up(int r, int c) { return r <= c ? c * (c + 1) / 2 + r : r * (r + 1) / 2 + c; }
};

// The side row of a state row (written next to its record by the forward pass): par[0 .. Q), then dt -- NaN where the row attempted
// an update and rejected it (det F <= 0): such a row serves no query.
template <int MODEL, int D, class W>
SSDE_HD void predict_side_row(const DualN<0>* par, double dt, bool na, bool updated, W&& side) {
    typedef PredictPk<MODEL, D> PK;
    SSDE_DLOOP for (int j = 0; j < PK::Q; j++) side(j) = par[j].v;
    side(PK::Q) = (!na && !updated) ? __builtin_nan("") : dt;
}

// Row j's packet from its record `rec(k)`, its side row `side(k)` and the r, N of the walk before the row is processed.
template <int MODEL, int D, int SD, class G, class S_, class W>
SSDE_HD void predict_packet_row(G&& rec, S_&& side, const double (&r)[SD], const double (&N)[SD][SD], bool tail, W&& pk) {
    typedef DenseDims<MODEL, D> DM;
    typedef SmoothRec<MODEL, D> RC;
    typedef PredictPk<MODEL, D> PK;
    static_assert(SD == DM::SD, "state dimension");
    double P[SD][SD], Fi[D][D], u[D];
    SSDE_DLOOP for (int a = 0; a < SD; a++)
        SSDE_DLOOP for (int b = 0; b < SD; b++) P[a][b] = rec(RC::P + RC::up(a, b));
    SSDE_DLOOP for (int i = 0; i < D; i++)
        SSDE_DLOOP for (int j = 0; j < D; j++) Fi[i][j] = rec(RC::FI + RC::up(i, j));
    SSDE_DLOOP for (int i = 0; i < D; i++) {
        double s = 0.0;
        SSDE_DLOOP for (int j = 0; j < D; j++) s += Fi[i][j] * rec(RC::V + j);
        u[i] = s;                                                   // F^-1 v (0 on a row without an update)
    }
    // filtered moments: a_f = a + P Z' F^-1 v, P_f = sym(P - P Z' F^-1 Z P)
    double G_[SD][D];
    SSDE_DLOOP for (int a = 0; a < SD; a++) {
        double s = rec(RC::A + a);
        SSDE_DLOOP for (int i = 0; i < D; i++) s += P[a][DM::z(i)] * u[i];
        pk(PK::AF + a) = s;
        SSDE_DLOOP for (int j = 0; j < D; j++) {
            double t = 0.0;
            SSDE_DLOOP for (int i = 0; i < D; i++) t += P[a][DM::z(i)] * Fi[i][j];
            G_[a][j] = t;                                           // P Z' F^-1
        }
    }
    SSDE_DLOOP for (int a = 0; a < SD; a++)
        SSDE_DLOOP for (int b = a; b < SD; b++) {
            double s = 0.0, t = 0.0;
            SSDE_DLOOP for (int j = 0; j < D; j++) { s += G_[a][j] * P[b][DM::z(j)]; t += G_[b][j] * P[a][DM::z(j)]; }
            pk(PK::PF + PK::up(a, b)) = P[a][b] - 0.5 * (s + t);
        }
    SSDE_DLOOP for (int a = 0; a < SD; a++) {
        pk(PK::R + a) = tail ? 0.0 : r[a];
        SSDE_DLOOP for (int b = a; b < SD; b++) pk(PK::N + PK::up(a, b)) = tail ? 0.0 : N[a][b];
    }
    SSDE_DLOOP for (int j = 0; j < PK::Q; j++) pk(PK::PAR + j) = side(j);
    const double dt = side(PK::Q);
    pk(PK::DT) = (tail && dt == dt) ? PREDICT_DT_TAIL : dt;         // (a rejected update stays NaN at the tail too)
}

// The query at offset `off` past the packet's row: false (the outputs are not written) where the definitions give NaN.
template <int MODEL, int D, int SD, class G>
SSDE_HD bool predict_query_row(G&& pk, double off, double (&am)[SD], double (&V)[SD][SD]) {
    typedef DenseDims<MODEL, D> DM;
    typedef PredictPk<MODEL, D> PK;
    static_assert(SD == DM::SD, "state dimension");
    constexpr int Q = DM::Q;
    const double dtp = pk(PK::DT);
    if (!(dtp == dtp)) return false;                                // the row rejected its update
    const bool tail = dtp < 0.0;
    if (!tail && off > dtp * (1.0 + PREDICT_DT_RTOL)) return false; // no extrapolation across a fix
    DenseLane<MODEL, D, 0> L;
    SSDE_DLOOP for (int a = 0; a < SD; a++) {
        L.a[a] = DualN<0>(pk(PK::AF + a));
        SSDE_DLOOP for (int b = 0; b < SD; b++) L.P[a][b] = DualN<0>(pk(PK::PF + PK::up(a, b)));
    }
    L.nll = DualN<0>(0.0);
    DualN<0> par[Q], H[D][D];
    SSDE_DLOOP for (int j = 0; j < Q; j++) par[j] = DualN<0>(pk(PK::PAR + j));
    double y[D];
    SSDE_DLOOP for (int i = 0; i < D; i++) {
        y[i] = 0.0;
        SSDE_DLOOP for (int j = 0; j < D; j++) H[i][j] = DualN<0>(0.0);
    }
    dense_step<MODEL, D, 0>(L, par, H, off, y, true);               // a_t = T(off) a_f + c(off), P_t = T P_f T' + Q(off)
    // T2 = T(Delta - off) with row j's parameters (makeT as smooth_record_row forms it)
    const double dt2 = tail ? 0.0 : fmax(dtp - off, 0.0);
    double t12 = 0.0, e = 1.0;
    if (MODEL == M_CTCRW) {
        const double tau = exp(par[D].v), beta = 1.0 / tau;
        e = exp(-(beta * dt2));
        t12 = (1.0 - e) / beta;
    } else if (MODEL == M_OU_SSM) {
        e = exp(-dt2 / exp(par[D].v));
    }
    // w = T2' r+, M = T2' N+ T2
    double w[SD], M[SD][SD];
    SSDE_DLOOP for (int a = 0; a < SD; a++) {
        w[a] = pk(PK::R + a);
        SSDE_DLOOP for (int b = 0; b < SD; b++) M[a][b] = pk(PK::N + PK::up(a, b));
    }
    if (MODEL == M_CTCRW) {
        SSDE_DLOOP for (int a = 0; a < SD; a += 2) w[a + 1] = t12 * w[a] + e * w[a + 1];
        SSDE_DLOOP for (int a = 0; a < SD; a++)
            SSDE_DLOOP for (int b = 0; b < SD; b += 2) M[a][b + 1] = t12 * M[a][b] + e * M[a][b + 1];
        SSDE_DLOOP for (int b = 0; b < SD; b++)
            SSDE_DLOOP for (int a = 0; a < SD; a += 2) M[a + 1][b] = t12 * M[a][b] + e * M[a + 1][b];
    } else {
        SSDE_DLOOP for (int a = 0; a < SD; a++) {
            w[a] = e * w[a];
            SSDE_DLOOP for (int b = 0; b < SD; b++) M[a][b] = e * e * M[a][b];
        }
    }
    // a^ = a_t + P_t w, V = sym(P_t - P_t M P_t)
    SSDE_DLOOP for (int a = 0; a < SD; a++) {
        double s = L.a[a].v;
        SSDE_DLOOP for (int b = 0; b < SD; b++) s += L.P[a][b].v * w[b];
        am[a] = s;
    }
    double PM[SD][SD];
    SSDE_DLOOP for (int a = 0; a < SD; a++)
        SSDE_DLOOP for (int b = 0; b < SD; b++) {
            double s = 0.0;
            SSDE_DLOOP for (int c = 0; c < SD; c++) s += L.P[a][c].v * M[c][b];
            PM[a][b] = s;
        }
    SSDE_DLOOP for (int a = 0; a < SD; a++)
        SSDE_DLOOP for (int b = a; b < SD; b++) {
            double s = 0.0, t = 0.0;
            SSDE_DLOOP for (int c = 0; c < SD; c++) { s += PM[a][c] * L.P[c][b].v; t += PM[b][c] * L.P[c][a].v; }
            const double m = 0.5 * (L.P[a][b].v + L.P[b][a].v) - 0.5 * (s + t);
            V[a][b] = m; V[b][a] = m;
        }
    return true;
}

}  // namespace ssde
#endif
