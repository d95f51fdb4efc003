// ssde_bridge.hpp -- joint posterior draws of the state at any time (ssde_predict_draws): the per-lane math, DESIGN.md §3.14.
//
// A draw of ssde_smooth_draws fixes the state at every state row.  Given the draw's states at the two rows around a query, the state
// inside the interval depends on nothing else (Markov): it is a Gaussian bridge between them, built from two prediction steps with
// row j's parameters -- dense_step (na = true) over delta_1 from the last answer and over delta_2 = Delta_j - delta to the right end --
// in the shape §3.10 uses for a backward step (X = Q1 T2' Ls^-T, C = Q1 - X X').  Past a track's last row there is no right end and
// the step is a plain simulation step.  bridge_slot_walk chains the distinct offsets of one slot in ascending order; the host twin
// (tests/hostsim/hostsim_predict_draws.cpp) and predict_draws_query_kernel both call it.  The transition's coefficients come from
// dense_step and smooth_trans_coef: nothing here spells them.
//
// Two packets per slot (a wanted state row of a lane), both slot-minor in the kernels (double k of slot i at base + k * stride + i):
//   ends, per draw: BridgePk::L + c the draw's state at the slot's row, BridgePk::R + c at the next row (not written at a tail);
//   side, per slot: BridgePk::PAR + j the row's linear predictors, BridgePk::DT its interval -- PREDICT_DT_TAIL at a track's last
//   row, NaN where the row rejected its update (predict_packet_row's rule).
#ifndef SSDE_BRIDGE_HPP
#define SSDE_BRIDGE_HPP

#include "ssde_draws.hpp"
#include "ssde_predict.hpp"

namespace ssde {

template <int MODEL, int D>
struct BridgePk {
    static constexpr int SD = DenseDims<MODEL, D>::SD, Q = DenseDims<MODEL, D>::Q;
    static constexpr int L = 0, R = SD, EZ = 2 * SD;          // the ends of one (slot, draw)
    static constexpr int PAR = 0, DT = Q, SW = Q + 1;          // the slot's side row, as PredictPk::SW lays it out
};

// the slot's side packet from the record pass's side row `side(k)`
template <int MODEL, int D, class S_, class W>
SSDE_HD void bridge_side_row(S_&& side, bool tail, W&& pk) {
    typedef BridgePk<MODEL, D> BK;
    SSDE_DLOOP for (int j = 0; j < BK::Q; j++) pk(BK::PAR + j) = side(j);
    const double dt = side(BK::Q);
    pk(BK::DT) = (tail && dt == dt) ? PREDICT_DT_TAIL : dt;
}

// the bridge's deviates: the row deviates' generator with counter words (s, track's low word, rank, 2^31 | (draw * 8 + (c >> 1))) --
// bit 31 of the last word is clear in every row deviate, so no bridge deviate equals one
template <int SD>
SSDE_HD void bridge_deviates(uint64_t seed, uint64_t track, uint32_t s, uint32_t rank, uint32_t draw, int col0, double (&z)[SD]) {
    const uint64_t trk = (track & 0xffffffffull) | ((uint64_t)rank << 32);
    SSDE_DLOOP for (int p = 0; p < SD; p += 2) {
        double n1, n2;
        draw_normal_pair(seed, trk, s, 0x80000000u | (draw * 8u + (uint32_t)((col0 + p) >> 1)), n1, n2);
        z[p] = n1;
        if (p + 1 < SD) z[p + 1] = n2;
    }
}

// One answer: the state d1 past x_prev given the right end alpha_next d2 further on (tail: no right end, alpha_next and d2 unread).
// A pivot <= 0 of chol(C) / chol(Q1) gives a zero column, of chol(S) NaN.
template <int MODEL, int D>
SSDE_HD void bridge_step(const DualN<0>* par, const double (&x_prev)[DenseDims<MODEL, D>::SD],
                         const double (&alpha_next)[DenseDims<MODEL, D>::SD], double d1, double d2, bool tail,
                         const double (&z)[DenseDims<MODEL, D>::SD], double (&x_out)[DenseDims<MODEL, D>::SD]) {
    constexpr int SD = DenseDims<MODEL, D>::SD;
    DenseLane<MODEL, D, 0> L;
    SSDE_DLOOP for (int a = 0; a < SD; a++) {
        L.a[a] = DualN<0>(x_prev[a]);
        SSDE_DLOOP for (int b = 0; b < SD; b++) L.P[a][b] = DualN<0>(0.0);
    }
    L.nll = DualN<0>(0.0);
    DualN<0> H[D][D];
    double y[D];
    SSDE_DLOOP for (int i = 0; i < D; i++) {
        y[i] = 0.0;
        SSDE_DLOOP for (int j = 0; j < D; j++) H[i][j] = DualN<0>(0.0);
    }
    dense_step<MODEL, D, 0>(L, par, H, d1, y, true);                // m1 = T(d1) x_prev + c(d1), Q1 = Q(d1)
    double m1[SD], Cm[SD][SD], add[SD];
    SSDE_DLOOP for (int a = 0; a < SD; a++) {
        m1[a] = L.a[a].v; add[a] = 0.0;
        SSDE_DLOOP for (int b = 0; b < SD; b++) Cm[a][b] = L.P[a][b].v;
    }
    if (!tail) {
        dense_step<MODEL, D, 0>(L, par, H, d2, y, true);            // m2 = T(d2) m1 + c(d2), S = T(d2) Q1 T(d2)' + Q(d2)
        double t12, e;
        smooth_trans_coef<MODEL, D>(par, d2, t12, e);
        double S[SD][SD], Ls[SD][SD], X[SD][SD], w[SD];
        SSDE_DLOOP for (int a = 0; a < SD; a++)
            SSDE_DLOOP for (int b = 0; b < SD; b++) S[a][b] = L.P[a][b].v;
        draw_chol<SD, false>(S, Ls);
        // X = Q1 T2' Ls^-T (B = Q1 T2' as draw_factor_row forms P_f T'), w = Ls^-1 (alpha_next - m2)
        SSDE_DLOOP for (int r = 0; r < SD; r++) {
            SSDE_DLOOP for (int c = 0; c < SD; c++) {
                double s;
                if (MODEL == M_CTCRW) s = (c & 1) ? e * Cm[r][c] : Cm[r][c] + t12 * Cm[r][c + 1];
                else s = e * Cm[r][c];
                SSDE_DLOOP for (int k = 0; k < c; k++) s -= X[r][k] * Ls[c][k];
                X[r][c] = s / Ls[c][c];
            }
        }
        SSDE_DLOOP for (int c = 0; c < SD; c++) {
            double s = alpha_next[c] - L.a[c].v;
            SSDE_DLOOP for (int k = 0; k < c; k++) s -= Ls[c][k] * w[k];
            w[c] = s / Ls[c][c];
        }
        SSDE_DLOOP for (int r = 0; r < SD; r++) {
            double s = 0.0;
            SSDE_DLOOP for (int c = 0; c < SD; c++) s += X[r][c] * w[c];
            add[r] = s;
        }
        // C = Q1 - X X': symmetric as formed
        SSDE_DLOOP for (int r = 0; r < SD; r++)
            SSDE_DLOOP for (int c = r; c < SD; c++) {
                double s = Cm[r][c];
                SSDE_DLOOP for (int k = 0; k < SD; k++) s -= X[r][k] * X[c][k];
                Cm[r][c] = s; Cm[c][r] = s;
            }
    }
    double Lc[SD][SD];
    draw_chol<SD, true>(Cm, Lc);
    SSDE_DLOOP for (int r = 0; r < SD; r++) {
        double s = m1[r] + add[r];
        SSDE_DLOOP for (int c = 0; c <= r; c++) s += Lc[r][c] * z[c];
        x_out[r] = s;
    }
}

// One (slot, draw): the slot's n_off distinct offsets off(r), ascending, chained from the left end.  dev(r, z) fills the deviates of
// rank r, emit(r, x) takes rank r's answer; a rank without an answer (the definitions' NaN) is not emitted.  dt: the side packet's.
template <int MODEL, int D, class O, class Z, class E>
SSDE_HD void bridge_slot_walk(const DualN<0>* par, double dt, const double (&left)[DenseDims<MODEL, D>::SD],
                              const double (&right)[DenseDims<MODEL, D>::SD], int64_t n_off, O&& off, Z&& dev, E&& emit) {
    constexpr int SD = DenseDims<MODEL, D>::SD;
    if (!(dt == dt)) return;                                        // the row rejected its update
    const bool tail = dt < 0.0;
    double t_prev = 0.0, x_prev[SD];
    SSDE_DLOOP for (int c = 0; c < SD; c++) x_prev[c] = left[c];
    for (int64_t r = 0; r < n_off; r++) {
        const double delta = off(r);
        if (delta == 0.0) { emit(r, left); continue; }
        if (!tail && delta > dt * (1.0 + PREDICT_DT_RTOL)) return;  // no extrapolation across a fix: this and every larger offset
        if (!tail && delta >= dt) { emit(r, right); continue; }
        double z[SD], x[SD];
        dev(r, z);
        bridge_step<MODEL, D>(par, x_prev, right, delta - t_prev, tail ? 0.0 : dt - delta, tail, z, x);
        emit(r, x);
        t_prev = delta;
        SSDE_DLOOP for (int c = 0; c < SD; c++) x_prev[c] = x[c];
    }
}

}  // namespace ssde
#endif
