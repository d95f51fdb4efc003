// ssde_draws.hpp -- joint posterior draws of the state path (ssde_smooth_draws): the per-lane math, DESIGN.md §3.10.
//
// Backward sampling over the records the smoother's forward pass wrote (SmoothRec, ssde_smooth.hpp).  draw_factor_row turns the
// records of rows j and j + 1 into the row's factors -- the offset m = a_f - J a_{j+1}, the smoother gain J = P_f T' P_{j+1}^-1 and
// the lower Cholesky factor L of the conditional covariance C -- which do not depend on the draw; draw_step applies them to one
// draw: alpha_j = m + J alpha_{j+1} + L z.  What row j + 1 contributes (a_{j+1} and the Cholesky factor of P_{j+1}) is carried in a
// DrawNext from the step before, so a backward walk reads every record once.  draw_normal_pair is the deviate generator of
// k_sim.hip (Philox4x32-10 + Box-Muller) for host and device.
#ifndef SSDE_DRAWS_HPP
#define SSDE_DRAWS_HPP

#include <stdint.h>

#include "ssde_smooth.hpp"

namespace ssde {

template <int MODEL, int D>
struct DrawFac {
    static constexpr int SD = DenseDims<MODEL, D>::SD;
    static constexpr int NL = SD * (SD + 1) / 2;
    static constexpr int M = 0, J = SD, L = J + SD * SD;
    static constexpr int R = L + NL;                         // doubles per row (CTCRW, d = 2: 30)
    SSDE_HD static constexpr int lo(int r, int c) { return r * (r + 1) / 2 + c; }      // r >= c
};

// what row j + 1 hands to row j: its prediction a_{j+1}, the lower Cholesky factor of P_{j+1} and the reciprocals of its pivots
template <int SD>
struct DrawNext {
    double a[SD], Lp[SD][SD], id[SD];
};

// before the track's last row: nothing is handed over (draw_factor_row does not read it when tail)
template <int SD>
SSDE_HD void draw_next_init(DrawNext<SD>& nx) {
    SSDE_DLOOP for (int r = 0; r < SD; r++) {
        nx.a[r] = 0.0; nx.id[r] = 0.0;
        SSDE_DLOOP for (int c = 0; c < SD; c++) nx.Lp[r][c] = 0.0;
    }
}

// Lower Cholesky factor in state order.  ZERO: a pivot <= 0 gives a zero column (a semidefinite matrix that rounding left slightly
// negative); otherwise the square root of a negative pivot is NaN and spreads through the factor.
template <int SD, bool ZERO>
SSDE_HD void draw_chol(const double (&S)[SD][SD], double (&L)[SD][SD]) {
    SSDE_DLOOP for (int j = 0; j < SD; j++) {
        double s = S[j][j];
        SSDE_DLOOP for (int k = 0; k < j; k++) s -= L[j][k] * L[j][k];
        if (ZERO && s <= 0.0) {
            SSDE_DLOOP for (int i = j; i < SD; i++) L[i][j] = 0.0;
            continue;
        }
        L[j][j] = sqrt(s);
        SSDE_DLOOP for (int i = j + 1; i < SD; i++) {
            double t = S[i][j];
            SSDE_DLOOP for (int k = 0; k < j; k++) t -= L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
}

// Row j's factors from its record `rec(k)`; nx holds row j + 1's hand-over on entry (not read when tail: row j is the track's last)
// and row j's on return.  fac(k) addresses double k of the factor row (DrawFac).
template <int MODEL, int D, int SD, class G, class W>
SSDE_HD void draw_factor_row(G&& rec, bool tail, DrawNext<SD>& nx, W&& fac) {
    typedef DenseDims<MODEL, D> DM;
    typedef SmoothRec<MODEL, D> RC;
    typedef DrawFac<MODEL, D> FC;
    static_assert(SD == DM::SD, "state dimension");
    double a[SD], P[SD][SD], Fi[D][D], u[D];
    SSDE_DLOOP for (int r = 0; r < SD; r++) a[r] = rec(RC::A + r);
    SSDE_DLOOP for (int r = 0; r < SD; r++)
        SSDE_DLOOP for (int c = 0; c < SD; c++) P[r][c] = rec(RC::P + RC::up(r, c));
    SSDE_DLOOP for (int i = 0; i < D; i++)
        SSDE_DLOOP for (int j = 0; j < D; j++) Fi[i][j] = rec(RC::FI + RC::up(i, j));
    SSDE_DLOOP for (int i = 0; i < D; i++) {
        double s = 0.0;
        SSDE_DLOOP for (int j = 0; j < D; j++) s += Fi[i][j] * rec(RC::V + j);
        u[i] = s;                                                   // F^-1 v (0 on a row without an update)
    }
    // filtered moments: a_f = a + P Z' F^-1 v, P_f = sym(P - P Z' F^-1 Z P)
    double af[SD], G_[SD][D], Pf[SD][SD];
    SSDE_DLOOP for (int r = 0; r < SD; r++) {
        double s = a[r];
        SSDE_DLOOP for (int i = 0; i < D; i++) s += P[r][DM::z(i)] * u[i];
        af[r] = s;
        SSDE_DLOOP for (int j = 0; j < D; j++) {
            double t = 0.0;
            SSDE_DLOOP for (int i = 0; i < D; i++) t += P[r][DM::z(i)] * Fi[i][j];
            G_[r][j] = t;                                           // P Z' F^-1
        }
    }
    SSDE_DLOOP for (int r = 0; r < SD; r++)
        SSDE_DLOOP for (int c = r; c < SD; c++) {
            double s = 0.0, t = 0.0;
            SSDE_DLOOP for (int j = 0; j < D; j++) { s += G_[r][j] * P[c][DM::z(j)]; t += G_[c][j] * P[r][DM::z(j)]; }
            const double m = P[r][c] - 0.5 * (s + t);
            Pf[r][c] = m; Pf[c][r] = m;
        }
    double Cm[SD][SD], L[SD][SD], Jm[SD][SD], mv[SD];
    if (tail) {
        SSDE_DLOOP for (int r = 0; r < SD; r++) {
            mv[r] = af[r];
            SSDE_DLOOP for (int c = 0; c < SD; c++) { Jm[r][c] = 0.0; Cm[r][c] = Pf[r][c]; }
        }
    } else {
        // B = P_f T' (makeT: CTCRW [[1, t12], [0, e]] per dimension, OU e I, BM I with e = 1)
        const double t12 = rec(RC::T), e = rec(RC::T + 1);
        double B[SD][SD], X[SD][SD];
        SSDE_DLOOP for (int r = 0; r < SD; r++)
            SSDE_DLOOP for (int c = 0; c < SD; c++) {
                if (MODEL == M_CTCRW) B[r][c] = (c & 1) ? e * Pf[r][c] : Pf[r][c] + t12 * Pf[r][c + 1];
                else B[r][c] = e * Pf[r][c];
            }
        // J = B P_{j+1}^-1 through P_{j+1} = Lp Lp': X = B Lp^-T, J = X Lp^-1
        SSDE_DLOOP for (int r = 0; r < SD; r++) {
            SSDE_DLOOP for (int c = 0; c < SD; c++) {
                double s = B[r][c];
                SSDE_DLOOP for (int k = 0; k < c; k++) s -= X[r][k] * nx.Lp[c][k];
                X[r][c] = s * nx.id[c];
            }
            SSDE_DLOOP for (int c = SD - 1; c >= 0; c--) {
                double s = X[r][c];
                SSDE_DLOOP for (int k = c + 1; k < SD; k++) s -= Jm[r][k] * nx.Lp[k][c];
                Jm[r][c] = s * nx.id[c];
            }
        }
        // C = P_f - J P_{j+1} J' = P_f - X X' (J Lp = X): symmetric as formed
        SSDE_DLOOP for (int r = 0; r < SD; r++)
            SSDE_DLOOP for (int c = r; c < SD; c++) {
                double s = Pf[r][c];
                SSDE_DLOOP for (int k = 0; k < SD; k++) s -= X[r][k] * X[c][k];
                Cm[r][c] = s; Cm[c][r] = s;
            }
        SSDE_DLOOP for (int r = 0; r < SD; r++) {
            double s = af[r];
            SSDE_DLOOP for (int c = 0; c < SD; c++) s -= Jm[r][c] * nx.a[c];
            mv[r] = s;                                              // a_f - J a_{j+1}
        }
    }
    SSDE_DLOOP for (int r = 0; r < SD; r++) {
        fac(FC::M + r) = mv[r];
        SSDE_DLOOP for (int c = 0; c < SD; c++) fac(FC::J + r + SD * c) = Jm[r][c];
    }
    draw_chol<SD, true>(Cm, L);
    SSDE_DLOOP for (int r = 0; r < SD; r++)
        SSDE_DLOOP for (int c = 0; c <= r; c++) fac(FC::L + FC::lo(r, c)) = L[r][c];
    // the hand-over to row j - 1
    draw_chol<SD, false>(P, nx.Lp);
    SSDE_DLOOP for (int r = 0; r < SD; r++) { nx.a[r] = a[r]; nx.id[r] = 1.0 / nx.Lp[r][r]; }
}

// One draw's step: alpha <- m + J alpha + L z (tail: alpha <- m + L z, whatever alpha held).
template <int MODEL, int D, int SD, class G>
SSDE_HD void draw_step(G&& fac, bool tail, double (&alpha)[SD], const double (&z)[SD]) {
    typedef DrawFac<MODEL, D> FC;
    double nw[SD];
    SSDE_DLOOP for (int r = 0; r < SD; r++) {
        double s = fac(FC::M + r);
        if (!tail) {
            SSDE_DLOOP for (int c = 0; c < SD; c++) s += fac(FC::J + r + SD * c) * alpha[c];
        }
        SSDE_DLOOP for (int c = 0; c <= r; c++) s += fac(FC::L + FC::lo(r, c)) * z[c];
        nw[r] = s;
    }
    SSDE_DLOOP for (int r = 0; r < SD; r++) alpha[r] = nw[r];
}

// ---- deviates: Philox4x32-10 as a counter-based generator + Box-Muller, as k_sim.hip has it ---------------------------------
SSDE_HD void draw_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// two independent N(0, 1) deviates of (seed, track, row, stream)
SSDE_HD void draw_normal_pair(uint64_t seed, uint64_t track, uint32_t row, uint32_t stream, double& n1, double& n2) {
    uint32_t o[4];
    draw_philox4x32_10(row, (uint32_t)track, (uint32_t)(track >> 32), stream, (uint32_t)seed, (uint32_t)(seed >> 32), o);
    const double u1 = ((double)((((uint64_t)o[0] << 32) | o[1]) >> 11) + 0.5) * 0x1.0p-53;     // (0, 1)
    const double u2 = ((double)((((uint64_t)o[2] << 32) | o[3]) >> 11) + 0.5) * 0x1.0p-53;
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
#if defined(__HIP_DEVICE_COMPILE__)
    sincospi(2.0 * u2, &s, &c);
#else
    s = sin(2.0 * M_PI * u2); c = cos(2.0 * M_PI * u2);
#endif
    n1 = r * c; n2 = r * s;
}

// the deviates of one draw at one state row: column c of the handle's state takes element c & 1 of stream draw * 8 + (c >> 1)
template <int SD>
SSDE_HD void draw_deviates(uint64_t seed, uint64_t track, uint32_t row, uint32_t draw, int col0, double (&z)[SD]) {
    SSDE_DLOOP for (int p = 0; p < SD; p += 2) {
        double n1, n2;
        draw_normal_pair(seed, track, row, draw * 8u + (uint32_t)((col0 + p) >> 1), n1, n2);
        z[p] = n1;
        if (p + 1 < SD) z[p + 1] = n2;
    }
}

}  // namespace ssde
#endif
