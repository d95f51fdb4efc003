// ssde_headforms.hpp -- the head of the lag-statistics path from Gram statistics, on the host (the bulk's forms:
// ssde_lagforms.hpp).
//
// With the bulk cut at the transient's end the streamed head is rows [0, cut) of every track (k_iso_shared_cut.hip).  Every recursion
// its lanes run -- ctcrw_mean_step on the table rows, SharedCtcrw::step_stat past them, which is the same step with the table's last
// row -- is affine in the track's data with coefficients that depend on theta only through the shared gains, and invariant under a
// constant shift of y and x.  Per (track k, coordinate a) the inputs are
//     w = (x0 - y_0, v0, D_1, ..., D_{C-1}),   D_i = y_i - y_{i-1},      C = HEAD_C rows, HEAD_NW = C + 1 components,
// and the statistics built once at create (k_lagstats.hip: head_gram_kernel) are
//     G = sum_{k,a} w w',     s_a = sum_k w_{k,a},     n = tracks;
// their leading block serves every cut <= C.
//
// The step in the shifted state c = (xi, v), xi_t = x_t - y_{t-1} (xi_0 = x0 - y_0), and d_j = (tx_j, tv_j): with u_t = D_t - xi_t
// (D_0 = 0) and the row's gains, ctcrw_mean_step reads
//     c'   = F c + g D_t + mu_a h,                         F = [[1 - k1, t12], [-k2, e]],  g = (k1 - 1, k2),  h = bm (b1, b2)
//     d_j' = F d_j + E_j c + kp_j D_t + mu_a lm_j,         E_j = [[-dk1_j, dt12_j], [-dk2_j, de_j]],  kp_j = (dk1_j, dk2_j),  lm_j = -bm (dt12_j, de_j)
// (dt12_j = de_j = 0 but for log tau), and mx, mv hold no data.  What the lanes accumulate per row, summed over tracks and coordinates, is
//     sum u^2 = G_tt - 2 q_xi + P_xi,xi,     sum u tx_j = q_tx_j - P_xi,tx_j,     sum_k u_a = s_a[1 + t] - m_a,xi
// with the second moments P_cc = sum c c', P_cd_j = sum c d_j', the first moments m_a = sum_k (c, d_j) and the moments with the row's
// own increment q = sum (c, d_j) D_t.  P and m follow from the step by a recursion of a dozen 2 x 2 products per row.  q needs the
// state as a function of the data: z_t = Z_t w + zeta_t,a, so q = Z_t G[., 1 + t] + sum_a zeta_t,a s_a[1 + t] -- eight dot products
// with one row of G.  The rows of Z_t are the responses of the step to a unit input per component of w (mu = 0), zeta that of zero
// data under the evaluation's mu.  From the first row at which every later row has the table's last gains, the column of increment
// i + 1 is the column of increment i one row later: those columns are read off ONE stored column (tests/test_headforms_host.py holds
// the shortcut to the run with every column a probe).  ~8 cut^2 / 2 multiply-adds per call instead of the cut^3 / 3 of the quadratic
// forms R_t G R_t' taken row by row.  The cancellation in sum u^2 is that of any quadratic form in the increments (the bulk's
// lam' M lam alike): |D|^2 / |u|^2 rounding units.
//
// accq = sum_t iF_t S_t, gq_j = sum_t (diF_j,t S_t / 2 - iF_t X_j,t), gmu_a = -sum_t iF_t mx_t U_t,a, finished by ctcrw_finish_parts.
// Fixed order, explicit loops, no allocation: two calls at the same theta give the same bits.  Host code only, no HIP type.
#pragma once
#include "ssde_math.hpp"

namespace ssde {

constexpr int HEAD_C = 128;                 // rows the statistics cover: the largest early cut
constexpr int HEAD_NW = HEAD_C + 1;         // components of w
constexpr int HEAD_GROW = 16;               // doubles per row of the gain table (GAIN_ROW)
constexpr int HEAD_LDW = (HEAD_NW + 7) / 8 * 8;   // padded row of the statistics as the forms read them
constexpr int HEAD_NS = 8;                  // state components: xi, v, then (tx_j, tv_j) per covariance direction

// w of one (track, coordinate): y[row][coordinate] tiled rows (>= HEAD_C of them), a0 = (x_1, v_1, x_2, v_2)
inline void head_track_w(const double* y, const double* a0, int d, int a, double* w) {
    w[0] = a0[2 * a] - y[a];
    w[1] = a0[2 * a + 1];
    for (int i = 1; i < HEAD_C; i++) w[1 + i] = y[(int64_t)i * d + a] - y[(int64_t)(i - 1) * d + a];
}

// The statistics of one track, added to G [HEAD_NW][HEAD_NW] and s [2][HEAD_NW] (the CPU reference of ssde_headstats_host)
inline void head_track_stats(const double* y, const double* a0, int d, double* G, double* s) {
    double w[HEAD_NW];
    for (int a = 0; a < d; a++) {
        head_track_w(y, a0, d, a, w);
        for (int p = 0; p < HEAD_NW; p++) {
            for (int q = 0; q < HEAD_NW; q++) G[p * HEAD_NW + q] += w[p] * w[q];
            s[a * HEAD_NW + p] += w[p];
        }
    }
}

// the statistics as the forms read them: rows of HEAD_LDW doubles, zero-padded (every loop then runs in whole blocks of four)
inline void head_pad_stats(const double* G, const double* s, double* Gp, double* sp) {
    for (int i = 0; i < HEAD_LDW * HEAD_LDW; i++) Gp[i] = 0.0;
    for (int i = 0; i < 2 * HEAD_LDW; i++) sp[i] = 0.0;
    for (int p = 0; p < HEAD_NW; p++)
        for (int q = 0; q < HEAD_NW; q++) Gp[p * HEAD_LDW + q] = G[p * HEAD_NW + q];
    for (int a = 0; a < 2; a++)
        for (int p = 0; p < HEAD_NW; p++) sp[a * HEAD_LDW + p] = s[a * HEAD_NW + p];
}

struct HeadFormArgs {
    const double* G;                  // [HEAD_LDW][HEAD_LDW] (host): the statistics in the leading HEAD_NW x HEAD_NW block, zeros around it
    const double* s;                  // [2][HEAD_LDW] (host), zeros past HEAD_NW
    double n;                         // tracks
    int cut;                          // rows of the head: 1 .. HEAD_C
    int d, mask;                      // response coordinates, DIR_* bits of the evaluation
    const double* gain;               // [gain_last + 1][HEAD_GROW]: the evaluation's gain table; rows past the last repeat it
    int gain_last;
    CtcrwTrans tr;
    double mu[2];
    bool full_probes;                 // every column by its own run (testing the shortcut)
};

struct HeadFormOut {
    double accq, gq[NDIRP], gmu[2];   // what the lanes' CtcrwMean would hold, summed over the tracks
    double acc[8];                    // the 4 + d accumulators
    int n_full;                       // columns that ran as probes
};

// work arrays of one call (kept by the caller: no allocation per evaluation).  Zero when made: the forms rely on the entries they
// never write -- the padding of the probe columns and the stored column before its first row -- being zero.
struct HeadFormWork {
    double z[HEAD_NS][HEAD_LDW + 8];         // the probe columns, state component by state component
    double din[HEAD_LDW + 8];                // the row's unit increment
    double col[HEAD_NS][HEAD_C + 8];         // the last probe column, row t at HEAD_C - 1 - t (a row reads it forwards)
    HeadFormWork() { memset(this, 0, sizeof(*this)); }
};

// Four doubles as one value (the compilers' vector extension: two SSE2 halves where the target has nothing wider): the partial sums
// over i mod 4 of the dot products are the four elements, so the order of every sum is the same whatever the instruction set.
typedef double head_v4 __attribute__((vector_size(32)));
#define SSDE_HEAD_INLINE inline __attribute__((always_inline))
SSDE_HEAD_INLINE double head_hsum(const double* q) { return (q[0] + q[1]) + (q[2] + q[3]); }

// q[k] += z_k . g over [0, m4) for the HEAD_NS vectors at z + k * stride, m4 a multiple of four; per vector four partial sums over
// i mod 4, kept in acc[k][0..3]
SSDE_HEAD_INLINE void head_dots(const double* z, int stride, const double* g, int m4, double (*acc)[4]) {
    head_v4 a[HEAD_NS];
    for (int k = 0; k < HEAD_NS; k++) __builtin_memcpy(&a[k], acc[k], 32);
    for (int i = 0; i < m4; i += 4) {
        head_v4 gv;
        __builtin_memcpy(&gv, g + i, 32);
        for (int k = 0; k < HEAD_NS; k++) {
            head_v4 zv;
            __builtin_memcpy(&zv, z + (int64_t)k * stride + i, 32);
            a[k] += zv * gv;
        }
    }
    for (int k = 0; k < HEAD_NS; k++) __builtin_memcpy(acc[k], &a[k], 32);
}

// 2 x 2 blocks [[a, b], [c, d]] and pairs of the moment recursion
struct Head2 { double a, b, c, d; };
struct HeadP { double x, y; };
SSDE_HEAD_INLINE Head2 h2_mul(const Head2& p, const Head2& q) { return {p.a * q.a + p.b * q.c, p.a * q.b + p.b * q.d, p.c * q.a + p.d * q.c, p.c * q.b + p.d * q.d}; }
SSDE_HEAD_INLINE Head2 h2_t(const Head2& p) { return {p.a, p.c, p.b, p.d}; }
SSDE_HEAD_INLINE Head2 h2_add(const Head2& p, const Head2& q) { return {p.a + q.a, p.b + q.b, p.c + q.c, p.d + q.d}; }
SSDE_HEAD_INLINE Head2 h2_outer(const HeadP& u, const HeadP& v) { return {u.x * v.x, u.x * v.y, u.y * v.x, u.y * v.y}; }
SSDE_HEAD_INLINE HeadP h2_mv(const Head2& p, const HeadP& v) { return {p.a * v.x + p.b * v.y, p.c * v.x + p.d * v.y}; }
SSDE_HEAD_INLINE HeadP hp_add(const HeadP& u, const HeadP& v) { return {u.x + v.x, u.y + v.y}; }
SSDE_HEAD_INLINE HeadP hp_scale(double f, const HeadP& v) { return {f * v.x, f * v.y}; }

// false: a table row that is not scored (iF == 0) or predicts without B mu -- such an evaluation keeps the kernel
// (SSDE_HEAD_TIME_NO_DOTS / _NO_PROBES / _NO_MOMENTS: tools/headforms_time.cpp alone defines them, to time the call without the dot
//  products, the probe-column updates or the per-direction moment recursion; the result is then wrong)
SSDE_HEAD_INLINE bool head_forms_body(const HeadFormArgs& A, HeadFormWork& W, HeadFormOut& o) {
    const int cut = A.cut, D = A.d, mask = A.mask;
    o.accq = 0.0;
    for (int j = 0; j < NDIRP; j++) o.gq[j] = 0.0;
    for (int a = 0; a < 2; a++) o.gmu[a] = 0.0;
    for (int k = 0; k < 8; k++) o.acc[k] = 0.0;
    o.n_full = 0;
    if (cut < 1 || cut > HEAD_C || D < 1 || D > 2 || A.gain_last < 0) return false;
    for (int t = 0; t <= A.gain_last && t < cut; t++) {
        const double* r = A.gain + (int64_t)t * HEAD_GROW;
        if (r[0] == 0.0 || r[3] != 1.0) return false;
    }
    const int nw = cut + 1;                                      // components of w the head reads
    // the last increment that runs as a probe: from its row on every row has the table's last gains
    const int i0 = A.gain_last > 1 ? A.gain_last : 1;
    const int nf = (A.full_probes || 2 + i0 > nw) ? nw : 2 + i0; // probe columns of w
    const int nf4 = (nf + 3) & ~3;
    o.n_full = nf;
    bool dir[NDIRP];
    for (int j = 0; j < NDIRP; j++) dir[j] = (mask & dir_bit(j)) != 0;
    const bool want_mu = (mask & DIR_MU) != 0;
    for (int k = 0; k < HEAD_NS; k++)
        for (int c = 0; c < nf4; c++) W.z[k][c] = 0.0;
    for (int c = 0; c < nf4; c++) W.din[c] = 0.0;
    W.z[0][0] = 1.0;                                             // component 0: xi_0 = x0 - y_0
    W.z[1][1] = 1.0;                                             // component 1: v0
    // the affine parts (zero data under mu_a), the moments and the data-free mu direction
    HeadP zc[2] = {{0.0, 0.0}, {0.0, 0.0}}, zd[NDIRP][2] = {{{0.0, 0.0}, {0.0, 0.0}}, {{0.0, 0.0}, {0.0, 0.0}}, {{0.0, 0.0}, {0.0, 0.0}}};
    const double* s_[2] = {A.s, A.s + HEAD_LDW};
    Head2 Pcc = {A.G[0], A.G[1], A.G[HEAD_LDW], A.G[HEAD_LDW + 1]};
    Head2 Pcd[NDIRP] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    HeadP mc[2] = {{0.0, 0.0}, {0.0, 0.0}}, md[NDIRP][2] = {{{0.0, 0.0}, {0.0, 0.0}}, {{0.0, 0.0}, {0.0, 0.0}}, {{0.0, 0.0}, {0.0, 0.0}}};
    for (int a = 0; a < D; a++) mc[a] = {s_[a][0], s_[a][1]};
    double mx = 0.0, mv = 0.0;
    const CtcrwTrans& tr = A.tr;
    for (int t = 0; t < cut; t++) {
        const double* r = A.gain + (int64_t)(t < A.gain_last ? t : A.gain_last) * HEAD_GROW;
        const double iF = r[0], k1 = r[1], k2 = r[2], bm = r[3];
        const Head2 F = {1.0 - k1, tr.t12, -k2, tr.e};
        const HeadP g = {k1 - 1.0, k2}, h = {bm * tr.b1, bm * tr.b2};
        // ---- the moments with the row's own increment: q = Z_t G[., 1 + t] + sum_a zeta_a s_a[1 + t]  (row 0 has none: u_0 = -xi_0)
        double q[HEAD_NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double Gtt = 0.0, sg[2] = {0.0, 0.0};
        const int at = HEAD_C - 1 - t;
        if (nf < nw)
            for (int k = 0; k < HEAD_NS; k++) W.col[k][at] = W.z[k][nf - 1];
        if (t >= 1) {
            const double* grow = A.G + (int64_t)(1 + t) * HEAD_LDW;      // (symmetric: row 1 + t for column 1 + t)
            Gtt = grow[1 + t];
            for (int a = 0; a < D; a++) sg[a] = s_[a][1 + t];
            double acc[HEAD_NS][4];
            for (int k = 0; k < HEAD_NS; k++) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0;
            // the probe columns (a column whose increment lies ahead holds zeros), then the columns past them: component c is the
            // last probe's state at row t - (c - (nf - 1)), c <= t
#ifndef SSDE_HEAD_TIME_NO_DOTS
            head_dots(&W.z[0][0], HEAD_LDW + 8, grow, nf4, acc);
            if (t + 1 > nf) head_dots(&W.col[0][at + 1], HEAD_C + 8, grow + nf, (t + 1 - nf + 3) & ~3, acc);
#endif
            for (int k = 0; k < HEAD_NS; k++) q[k] = head_hsum(acc[k]);
            for (int a = 0; a < D; a++) {
                q[0] += zc[a].x * sg[a]; q[1] += zc[a].y * sg[a];
                for (int j = 0; j < NDIRP; j++) { q[2 + 2 * j] += zd[j][a].x * sg[a]; q[3 + 2 * j] += zd[j][a].y * sg[a]; }
            }
        }
        const HeadP qc = {q[0], q[1]};
        // ---- the row's sums and what ctcrw_mean_step accumulates from them
        const double S = Gtt - 2.0 * qc.x + Pcc.a;
        o.accq += iF * S;
        for (int j = 0; j < NDIRP; j++) {
            if (!dir[j]) continue;
            const double X = q[2 + 2 * j] - Pcd[j].a;
            o.gq[j] += 0.5 * r[4 + j] * S - iF * X;
        }
        if (want_mu)
            for (int a = 0; a < D; a++) o.gmu[a] -= iF * mx * (sg[a] - mc[a].x);
        // ---- the moments after the step
        const HeadP Fqc = h2_mv(F, qc);
        HeadP Fmc[2], wa[2];
        HeadP hsum = {0.0, 0.0};                                 // sum_a mu_a (F m_a + g s_a)
        double mu2 = 0.0, musg = 0.0;
        for (int a = 0; a < D; a++) {
            Fmc[a] = h2_mv(F, mc[a]);
            wa[a] = hp_add(Fmc[a], hp_scale(sg[a], g));
            hsum = hp_add(hsum, hp_scale(A.mu[a], wa[a]));
            mu2 += A.mu[a] * A.mu[a];
            musg += A.mu[a] * sg[a];
        }
#ifndef SSDE_HEAD_TIME_NO_MOMENTS
        for (int j = 0; j < NDIRP; j++) {
            if (!dir[j]) continue;
            const double de = (j == 1) ? tr.de : 0.0, dt12 = (j == 1) ? tr.dt12 : 0.0;
            const Head2 E = {-r[7 + j], dt12, -r[10 + j], de};
            const HeadP kp = {r[7 + j], r[10 + j]}, lm = {-bm * dt12, -bm * de};
            const HeadP qd = {q[2 + 2 * j], q[3 + 2 * j]};
            // P_cd' = F P_cd F' + F P_cc E' + (F q_c) kp' + sum_a mu_a (F m_a) lm' + g (F q_d + E q_c + G_tt kp + sum_a mu_a s_a lm)'
            //         + h (sum_a mu_a (F md_a + E m_a + s_a kp) + n sum_a mu_a^2 lm)'
            HeadP first = {0.0, 0.0}, hpart = hp_scale(A.n * mu2, lm);
            HeadP mdn[2];
            for (int a = 0; a < D; a++) {
                first = hp_add(first, hp_scale(A.mu[a], Fmc[a]));
                const HeadP step = hp_add(hp_add(h2_mv(F, md[j][a]), h2_mv(E, mc[a])), hp_scale(sg[a], kp));
                hpart = hp_add(hpart, hp_scale(A.mu[a], step));
                mdn[a] = hp_add(step, hp_scale(A.n * A.mu[a], lm));
            }
            const HeadP gpart = hp_add(hp_add(h2_mv(F, qd), h2_mv(E, qc)), hp_add(hp_scale(Gtt, kp), hp_scale(musg, lm)));
            Head2 P = h2_add(h2_mul(h2_mul(F, Pcd[j]), h2_t(F)), h2_mul(h2_mul(F, Pcc), h2_t(E)));
            P = h2_add(P, h2_add(h2_outer(Fqc, kp), h2_outer(first, lm)));
            P = h2_add(P, h2_add(h2_outer(g, gpart), h2_outer(h, hpart)));
            Pcd[j] = P;
            for (int a = 0; a < D; a++) md[j][a] = mdn[a];
        }
#endif
        {
            // P_cc' = F P_cc F' + (F q_c) g' + g (F q_c)' + G_tt g g' + sum_a mu_a (w_a h' + h w_a') + n sum_a mu_a^2 h h'
            Head2 P = h2_mul(h2_mul(F, Pcc), h2_t(F));
            P = h2_add(P, h2_add(h2_outer(Fqc, g), h2_outer(g, Fqc)));
            P = h2_add(P, h2_outer(hp_scale(Gtt, g), g));
            P = h2_add(P, h2_add(h2_outer(hsum, h), h2_outer(h, hsum)));
            P = h2_add(P, h2_outer(hp_scale(A.n * mu2, h), h));
            Pcc = P;
            for (int a = 0; a < D; a++) mc[a] = hp_add(wa[a], hp_scale(A.n * A.mu[a], h));
        }
        // ---- the step of the affine parts, of mu's direction and of the probe columns (the row's unit increment: column 1 + t)
        for (int a = 0; a < D; a++) {
            for (int j = 0; j < NDIRP; j++) {
                if (!dir[j]) continue;
                const double de = (j == 1) ? tr.de : 0.0, dt12 = (j == 1) ? tr.dt12 : 0.0;
                const Head2 E = {-r[7 + j], dt12, -r[10 + j], de};
                const HeadP lm = {-bm * dt12, -bm * de};
                zd[j][a] = hp_add(hp_add(h2_mv(F, zd[j][a]), h2_mv(E, zc[a])), hp_scale(A.mu[a], lm));
            }
            zc[a] = hp_add(h2_mv(F, zc[a]), hp_scale(A.mu[a], h));
        }
        if (want_mu) {
            const double nx = F.a * mx + F.b * mv + h.x, nv = F.c * mx + F.d * mv + h.y;
            mx = nx; mv = nv;
        }
        if (t >= 1 && 1 + t < nf) W.din[1 + t] = 1.0;
#ifndef SSDE_HEAD_TIME_NO_PROBES
        for (int j = 0; j < NDIRP; j++) {
            if (!dir[j]) continue;
            const double de = (j == 1) ? tr.de : 0.0, dt12 = (j == 1) ? tr.dt12 : 0.0;
            const double e11 = -r[7 + j], e21 = -r[10 + j], kp1 = r[7 + j], kp2 = r[10 + j];
            double* tx = W.z[2 + 2 * j];
            double* tv = W.z[3 + 2 * j];
            for (int c = 0; c < nf4; c++) {
                const double nx = (F.a * tx[c] + F.b * tv[c]) + (e11 * W.z[0][c] + dt12 * W.z[1][c]) + kp1 * W.din[c];
                const double nv = (F.c * tx[c] + F.d * tv[c]) + (e21 * W.z[0][c] + de * W.z[1][c]) + kp2 * W.din[c];
                tx[c] = nx; tv[c] = nv;
            }
        }
        for (int c = 0; c < nf4; c++) {
            const double nx = (F.a * W.z[0][c] + F.b * W.z[1][c]) + g.x * W.din[c];
            const double nv = (F.c * W.z[0][c] + F.d * W.z[1][c]) + g.y * W.din[c];
            W.z[0][c] = nx; W.z[1][c] = nv;
        }
#endif
        if (t >= 1 && 1 + t < nf) W.din[1 + t] = 0.0;
    }
    // what the lanes finish with: ctcrw_finish_parts on the summed accumulators (no log-determinant terms: those are data-free)
    CtcrwMean<2, 15> M;
    const double a0[4] = {0.0, 0.0, 0.0, 0.0};
    M.init(a0);
    M.accq = o.accq;
    for (int j = 0; j < NDIRP; j++) M.gq[j] = o.gq[j];
    for (int a = 0; a < 2; a++) M.gmu[a] = o.gmu[a];
    const double z[NDIRP] = {0.0, 0.0, 0.0};
    double out[6];
    ctcrw_finish_parts<2, 15>(0.0, z, M, out);
    o.acc[0] = out[0];
    o.acc[1] = dir[0] ? out[1] : 0.0;
    for (int a = 0; a < D; a++) o.acc[2 + a] = want_mu ? out[2 + a] : 0.0;
    o.acc[2 + D] = dir[1] ? out[4] : 0.0;
    o.acc[3 + D] = dir[2] ? out[5] : 0.0;
    return true;
}

// The same source compiled a second time for AVX2 + FMA where the host has them; the choice is made once per process.
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__) && (defined(__clang__) || defined(__GNUC__))
__attribute__((target("avx2,fma"))) inline bool head_forms_avx2(const HeadFormArgs& A, HeadFormWork& W, HeadFormOut& o) { return head_forms_body(A, W, o); }
inline bool head_forms_host(const HeadFormArgs& A, HeadFormWork& W, HeadFormOut& o) {
    static const bool wide = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
    return wide ? head_forms_avx2(A, W, o) : head_forms_body(A, W, o);
}
#else
inline bool head_forms_host(const HeadFormArgs& A, HeadFormWork& W, HeadFormOut& o) { return head_forms_body(A, W, o); }
#endif

}  // namespace ssde
