// ssde_ahead.hpp -- multi-step-ahead forecast errors and scores (ssde_forecast_scores): the per-lane math, DESIGN.md §3.21.
//
// The record of state row r holds the one-step prediction a_r, P_r = E, Var[x_r | y_first .. y_{r-1}].  The forecast of row t from
// the data through row t - k is that prediction pushed through the k - 1 rows r = t - k + 1 .. t - 1 as the filter pushes it through a
// NA row: ahead_step, which is dense_step with na = true on the row's own linear predictors and interval.  What a step through row i
// and a score at row t need beyond the record -- the linear predictors (T_i, Q_i and the drift come from them), the interval, y_t,
// H_t and whether y_t is NA -- the forward pass writes next to the record as a side row (ahead_side_row; AheadSide lays it out).
// ahead_score standardises the error of one target; ahead_fold adds a scored target to the sums of its (track, horizon).
// Host- and device-compilable; every loop has a constant trip count.
#ifndef SSDE_AHEAD_HPP
#define SSDE_AHEAD_HPP

#include <math.h>
#include <stdint.h>

#include "../../include/ssde.h"      // SSDE_AHEAD_MAX_*: the one definition
#include "ssde_loo.hpp"              // loo_cholesky, loo_finite: the conventions of ssde_smooth_loo

namespace ssde {

constexpr int AHEAD_NH = SSDE_AHEAD_MAX_H;
constexpr int AHEAD_NTHR = SSDE_AHEAD_MAX_THR;
constexpr int AHEAD_NSTAT0 = 5;                               // the statistics before the counts
constexpr int AHEAD_NSTAT_MAX = AHEAD_NSTAT0 + AHEAD_NTHR;

// the side row of a state row: the linear predictors, the interval after the row, y, the symmetric part of H (upper triangle,
// SmoothRec::up's order) and 1.0 where the row's observation is NA (the handle's na_mode), else 0.0
template <int MODEL, int D>
struct AheadSide {
    static constexpr int Q = DenseDims<MODEL, D>::Q, NF = D * (D + 1) / 2;
    static constexpr int PAR = 0, DT = Q, Y = DT + 1, H = Y + D, NA = H + NF;
    static constexpr int SW = NA + 1;                        // doubles per side row (CTCRW, d = 2: 11)
    SSDE_HD static constexpr int up(int r, int c) { return r <= c ? c * (c + 1) / 2 + r : r * (r + 1) / 2 + c; }
};

template <int MODEL, int D, class W>
SSDE_HD void ahead_side_row(const DualN<0>* par, const DualN<0> (&H)[D][D], double dt, const double* y, bool na, W&& side) {
    typedef AheadSide<MODEL, D> AS;
    SSDE_DLOOP for (int j = 0; j < AS::Q; j++) side(AS::PAR + j) = par[j].v;
    side(AS::DT) = dt;
    SSDE_DLOOP for (int i = 0; i < D; i++) side(AS::Y + i) = y[i];
    SSDE_DLOOP for (int c = 0; c < D; c++)
        SSDE_DLOOP for (int r = 0; r <= c; r++) side(AS::H + AS::up(r, c)) = 0.5 * (H[r][c].v + H[c][r].v);
    side(AS::NA) = na ? 1.0 : 0.0;
}

// the chain's state from row r's record: a_r, P_r
template <int MODEL, int D, class G>
SSDE_HD void ahead_load(G&& rec, DenseLane<MODEL, D, 0>& L) {
    typedef SmoothRec<MODEL, D> RC;
    constexpr int SD = RC::SD;
    SSDE_DLOOP for (int a = 0; a < SD; a++) {
        L.a[a] = DualN<0>(rec(RC::A + a));
        SSDE_DLOOP for (int b = 0; b < SD; b++) L.P[a][b] = DualN<0>(rec(RC::P + RC::up(a, b)));
    }
    L.nll = DualN<0>(0.0);
}

// one prediction step through the row whose side row is `side`: a <- T a + drift, P <- T P T' + Q, as the filter steps through a NA
// row; returns the row's interval
template <int MODEL, int D, class S_>
SSDE_HD double ahead_step(DenseLane<MODEL, D, 0>& L, S_&& side) {
    typedef AheadSide<MODEL, D> AS;
    DualN<0> par[AS::Q], H[D][D];
    SSDE_DLOOP for (int j = 0; j < AS::Q; j++) par[j] = DualN<0>(side(AS::PAR + j));
    double y[D];
    SSDE_DLOOP for (int i = 0; i < D; i++) {
        y[i] = 0.0;
        SSDE_DLOOP for (int j = 0; j < D; j++) H[i][j] = DualN<0>(0.0);
    }
    const double dt = side(AS::DT);
    dense_step<MODEL, D, 0>(L, par, H, dt, y, true);
    return dt;
}

// One target: scored where y is not NA, m = Z a and S = Z P Z' + H are finite and the symmetrised S has a Cholesky factor with
// finite, positive pivots; then z = C^-1 (y - m), q = z'z, lpd = -(D log 2 pi + log det S + q) / 2, e2 = |y - m|^2.
template <int D>
struct AheadScore {
    double z[D], q, lpd, e2;
    bool scored;
};

template <int MODEL, int D, class S_>
SSDE_HD void ahead_score(const DenseLane<MODEL, D, 0>& L, S_&& side, AheadScore<D>& o) {
    typedef DenseDims<MODEL, D> DM;
    typedef AheadSide<MODEL, D> AS;
    double S[D][D], C[D][D], v[D];
    bool fin = true;
    SSDE_DLOOP for (int i = 0; i < D; i++) {
        const double m = L.a[DM::z(i)].v;
        v[i] = side(AS::Y + i) - m;
        fin = fin && loo_finite(m);
        SSDE_DLOOP for (int j = 0; j < D; j++) {
            S[i][j] = 0.5 * (L.P[DM::z(i)][DM::z(j)].v + L.P[DM::z(j)][DM::z(i)].v) + side(AS::H + AS::up(i, j));
            fin = fin && loo_finite(S[i][j]);
        }
    }
    o.q = 0.0; o.lpd = 0.0; o.e2 = 0.0;
    SSDE_DLOOP for (int i = 0; i < D; i++) o.z[i] = 0.0;
    o.scored = fin && side(AS::NA) == 0.0 && loo_cholesky<D>(S, C);
    if (!o.scored) return;
    double q = 0.0, ld = 0.0, e2 = 0.0;
    SSDE_DLOOP for (int i = 0; i < D; i++) {
        double s = v[i];
        SSDE_DLOOP for (int k = 0; k < i; k++) s -= C[i][k] * o.z[k];
        o.z[i] = s / C[i][i];
        q += o.z[i] * o.z[i];
        ld += log(C[i][i]);
        e2 += v[i] * v[i];
    }
    o.q = q; o.e2 = e2;
    o.lpd = -0.5 * ((double)D * 1.8378770664093454835606594728112 + 2.0 * ld + q);
}

// a scored target into the sums of its (track, horizon): acc(k) is statistic k (0 the scored targets, 1 the sum of lpd, 2 of q, 3 of
// |y - m|^2, 4 of the lead time, 5 + r the targets with q > thr[r]; whole numbers add exactly in doubles)
template <int D, class A_, class G>
SSDE_HD void ahead_fold(A_&& acc, const AheadScore<D>& o, double lead, G&& thr, int n_thr) {
    acc(0) += 1.0;
    acc(1) += o.lpd;
    acc(2) += o.q;
    acc(3) += o.e2;
    acc(4) += lead;
    SSDE_LLOOP for (int r = 0; r < AHEAD_NTHR; r++)
        if (r < n_thr && o.q > thr(r)) acc(AHEAD_NSTAT0 + r) += 1.0;
}

}  // namespace ssde
#endif
