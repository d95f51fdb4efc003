// tests/hostsim/hostsim.cpp -- TEST-ONLY host build of the kernel arithmetic.
//
// Compiles smoothsde_amd/csrc/ssde_math.hpp (the per-lane step functions the HIP kernels
// inline; with ssde_dense.hpp and ssde_smooth.hpp the smoother's lane math) with g++ and
// walks tracks sequentially the way one wavefront lane does, so the
// CPU suite (-m "not gpu") can check the hand-derived forward sensitivities against the
// oracle without a GPU.  This is NOT a product path: it is built only by the tests, lives
// outside the package, and libssde_hip.so contains no CPU evaluation code.
#include <cstdint>
#include <cstdio>
#include <cmath>

#include "../../smoothsde_amd/csrc/ssde_math.hpp"
#include "../../smoothsde_amd/csrc/ssde_tv.hpp"
#include "../../smoothsde_amd/csrc/ssde_adj.hpp"
#include "../../smoothsde_amd/csrc/ssde_dense.hpp"
#include "../../smoothsde_amd/csrc/ssde_smooth.hpp"
#include "../../smoothsde_amd/csrc/ssde_knobs.hpp"
#include "../../smoothsde_amd/csrc/ssde_windows.hpp"
#include "hostsim_records.hpp"
#include <sstream>
#include <vector>

using namespace ssde;

namespace {

struct IsoArgs {
    int model, d, mask, any_nan;
    int64_t n, n_tracks;
    const int64_t* row0;   // first row of each track
    const int64_t* nrows;  // rows of each track
    const double* times;
    const double* obs;     // n x d column-major
    double log_sigma_obs, mu[2], p1, p2;  // working-scale parameters
    double p0[3];          // CTCRW: p11,p12,p22 ; OU/BM: p
};

template <int D, int MASK>
void run_ctcrw(const IsoArgs& A, double* out) {
    const double h = exp(A.log_sigma_obs) * exp(A.log_sigma_obs);
    const double tau = exp(A.p1), nu = exp(A.p2), beta = 1.0 / tau;
    const double sigma = 2.0 * nu / sqrt(M_PI * tau);
    for (int k = 0; k < 4 + D; k++) out[k] = 0.0;
    for (int64_t m = 0; m < A.n_tracks; m++) {
        CtcrwLane<D, MASK> L;
        double a0[2 * D];
        for (int a = 0; a < D; a++) { a0[2 * a] = A.obs[A.row0[m] + a * A.n]; a0[2 * a + 1] = 0.0; }
        L.init(a0, A.p0[0], A.p0[1], A.p0[2]);
        for (int64_t s = 1; s < A.nrows[m]; s++) {
            int64_t i = A.row0[m] + s;
            double dt = (s < A.nrows[m] - 1) ? A.times[i + 1] - A.times[i] : 1.0;
            CtcrwTrans tr;
            ctcrw_trans(dt, tau, beta, sigma, tr);
            double y[D];
            for (int a = 0; a < D; a++) y[a] = A.obs[i + a * A.n];
            ctcrw_step<D, MASK>(L, tr, h, A.mu, y, is_na(y[0], A.any_nan));
        }
        double o[4 + D];
        ctcrw_finish<D, MASK>(L, o);
        for (int k = 0; k < 4 + D; k++) out[k] += o[k];
    }
}

template <int D, int MASK, int MODEL>
void run_scal(const IsoArgs& A, double* out) {
    const double h = exp(A.log_sigma_obs) * exp(A.log_sigma_obs);
    for (int k = 0; k < 4 + D; k++) out[k] = 0.0;
    for (int64_t m = 0; m < A.n_tracks; m++) {
        ScalLane<D, MASK> L;
        double a0x[D];
        for (int a = 0; a < D; a++) a0x[a] = A.obs[A.row0[m] + a * A.n];
        L.init(a0x, A.p0[0]);
        for (int64_t s = 1; s < A.nrows[m]; s++) {
            int64_t i = A.row0[m] + s;
            double dt = (s < A.nrows[m] - 1) ? A.times[i + 1] - A.times[i] : 1.0;
            ScalTrans tr;
            if (MODEL == M_OU_SSM) ou_trans(dt, exp(A.p1), exp(A.p2), tr);
            else bm_trans(dt, exp(A.p1), tr);
            double y[D];
            for (int a = 0; a < D; a++) y[a] = A.obs[i + a * A.n];
            scal_step<D, MASK, MODEL == M_OU_SSM>(L, tr, h, A.mu, y, is_na(y[0], A.any_nan));
        }
        double o[4 + D];
        scal_finish<D, MASK>(L, o);
        for (int k = 0; k < 4 + D; k++) out[k] += o[k];
    }
}

template <int D, int MASK>
void run_model(const IsoArgs& A, double* out) {
    if (A.model == M_CTCRW) run_ctcrw<D, MASK>(A, out);
    else if (A.model == M_OU_SSM) run_scal<D, MASK, M_OU_SSM>(A, out);
    else run_scal<D, MASK, M_BM_SSM>(A, out);
}

template <int D>
void run_mask(const IsoArgs& A, double* out) {
    switch (A.mask) {
#define C(M) case M: run_model<D, M>(A, out); break;
        C(0) C(1) C(2) C(3) C(4) C(5) C(6) C(7) C(8) C(9) C(10) C(11) C(12) C(13) C(14) C(15)
#undef C
    }
}

// row-varying coefficients (ssde_tv.hpp): records by the pre-pass arithmetic, then one lane per direction
template <int MODEL, int D>
void run_tv(int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows, const double* times,
            const double* obs, const double* parmat, int q, int nd, const int* kinds, const int* dims, const double* wmat,
            double log_sigma_obs, const double* p0, const double* a0, double* out) {
    typedef TvOps<MODEL, D> Ops;
    constexpr int SD = Ops::Lane::SD;
    const double h = exp(log_sigma_obs) * exp(log_sigma_obs);
    for (int k = 0; k < 1 + nd; k++) out[k] = 0.0;
    for (int kk = -1; kk < nd; kk++) {              // kk = -1: value-only lane
        for (int64_t m = 0; m < n_tracks; m++) {
            typename Ops::Lane L;
            double a[SD];
            for (int c = 0; c < SD; c++) a[c] = 0.0;
            if (a0) for (int c = 0; c < SD; c++) a[c] = a0[m * SD + c];
            else for (int c = 0; c < D; c++) a[MODEL == M_CTCRW ? 2 * c : c] = obs[row0[m] + c * n];
            L.init(a, p0);
            for (int64_t s = 1; s < nrows[m]; s++) {
                const int64_t i = row0[m] + s;
                const double dt = (s < nrows[m] - 1) ? times[i + 1] - times[i] : 1.0;
                double par[4], y[D], rec[TV_RS];
                for (int j = 0; j < q; j++) par[j] = parmat[i + (int64_t)j * n];
                for (int c = 0; c < D; c++) y[c] = obs[i + c * n];
                tv_make_record<MODEL, D>(dt, par, y, rec);
                if (kk < 0) Ops::template step<false>(L, rec, h, 0, 0, 0.0, any_nan);
                else Ops::template step<true>(L, rec, h, kinds[kk], dims[kk], wmat[i * nd + kk], any_nan);
            }
            if (kk < 0) out[0] += L.value();
            else out[1 + kk] += L.grad();
        }
    }
}

// reverse sweep (ssde_adj.hpp): forward pass with a record per row, backward pass; G[i + j n] = d nllk / d parmat(i, j)
template <int MODEL, int D>
void run_adj(int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows, const double* times,
             const double* obs, const double* parmat, int q, double log_sigma_obs, const double* p0, const double* a0,
             double* out, double* G) {
    typedef typename AdjModel<MODEL, D>::Lane Lane;
    constexpr int SD = Lane::SD, NF = Lane::NF;
    const double h = exp(log_sigma_obs) * exp(log_sigma_obs);
    out[0] = out[1] = 0.0;
    for (int64_t k = 0; k < n * q; k++) G[k] = 0.0;
    for (int64_t m = 0; m < n_tracks; m++) {
        Lane L;
        double a[SD];
        for (int c = 0; c < SD; c++) a[c] = 0.0;
        if (a0) for (int c = 0; c < SD; c++) a[c] = a0[m * SD + c];
        else for (int c = 0; c < D; c++) a[MODEL == M_CTCRW ? 2 * c : c] = obs[row0[m] + c * n];
        L.init(a, p0);
        LogAcc ld; ld.init();
        double accq = 0.0;
        std::vector<double> recs((size_t)nrows[m] * NF);
        auto dt_of = [&](int64_t s) { const int64_t i = row0[m] + s; return (s < nrows[m] - 1) ? times[i + 1] - times[i] : 1.0; };
        for (int64_t s = 1; s < nrows[m]; s++) {
            const int64_t i = row0[m] + s;
            double mu[D], y[D];
            for (int c = 0; c < D; c++) { mu[c] = parmat[i + (int64_t)c * n]; y[c] = obs[i + c * n]; }
            typename Lane::Trans tr;
            Lane::trans(dt_of(s), parmat[i + (int64_t)D * n], q > D + 1 ? parmat[i + (int64_t)(D + 1) * n] : 0.0, tr);
            Lane::template put_trans<1>(&recs[(size_t)s * NF], tr);
            typename Lane::Trans tb;                                // (the forward step reads its transition back from the record, as the kernel does)
            Lane::template get_trans<1>(&recs[(size_t)s * NF], dt_of(s), tb);
            L.template fwd<true, 1>(tb, h, mu, y, is_na(y[0], any_nan), ld, accq, &recs[(size_t)s * NF]);
        }
        out[0] += 0.5 * ((double)D * ld.value() + accq);
        typename Lane::Adj A;
        A.zero();
        for (int64_t s = nrows[m] - 1; s >= 1; s--) {
            const int64_t i = row0[m] + s;
            double mu[D];
            for (int c = 0; c < D; c++) mu[c] = parmat[i + (int64_t)c * n];
            AdjRowGrad<D> g;
            Lane::template bwd<1>(A, &recs[(size_t)s * NF], h, mu, dt_of(s), g);
            for (int c = 0; c < D; c++) G[i + (int64_t)c * n] = g.gmu[c];
            G[i + (int64_t)D * n] = g.g1;
            if (q > D + 1) G[i + (int64_t)(D + 1) * n] = g.g2;
            out[1] += 2.0 * h * g.gh;
        }
    }
}

// ... on the full-covariance lanes (AdjFull: two response columns, per-row H_array or sigma_obs^2 I, any P0)
template <int MODEL>
void run_adj_full(int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows, const double* times,
                  const double* obs, const double* parmat, int q, double log_sigma_obs, const double* p0f, const double* a0,
                  const double* harr /* d x d x n or NULL */, double* out, double* G) {
    typedef AdjFull<MODEL> Lane;
    constexpr int SD = Lane::SD, NF = Lane::NF, D = 2;
    const double h = exp(log_sigma_obs) * exp(log_sigma_obs);
    out[0] = out[1] = 0.0;
    for (int64_t k = 0; k < n * q; k++) G[k] = 0.0;
    for (int64_t m = 0; m < n_tracks; m++) {
        Lane L;
        double a[SD];
        for (int c = 0; c < SD; c++) a[c] = 0.0;
        if (a0) for (int c = 0; c < SD; c++) a[c] = a0[m * SD + c];
        else for (int c = 0; c < D; c++) a[Lane::z(c)] = obs[row0[m] + c * n];
        L.init(a, p0f);
        LogAcc ld; ld.init();
        double accq = 0.0;
        std::vector<double> recs((size_t)nrows[m] * NF);
        auto dt_of = [&](int64_t s) { const int64_t i = row0[m] + s; return (s < nrows[m] - 1) ? times[i + 1] - times[i] : 1.0; };
        auto H_of = [&](int64_t i, double* H) { if (harr) { H[0] = harr[i * 4]; H[1] = harr[i * 4 + 2]; H[2] = harr[i * 4 + 3]; } else { H[0] = h; H[1] = 0.0; H[2] = h; } };
        for (int64_t s = 1; s < nrows[m]; s++) {
            const int64_t i = row0[m] + s;
            double mu[D], y[D], H[3];
            for (int c = 0; c < D; c++) { mu[c] = parmat[i + (int64_t)c * n]; y[c] = obs[i + c * n]; }
            H_of(i, H);
            typename Lane::Trans tr, tb;
            Lane::trans(dt_of(s), parmat[i + (int64_t)D * n], q > D + 1 ? parmat[i + (int64_t)(D + 1) * n] : 0.0, tr);
            Lane::template put_trans<1>(&recs[(size_t)s * NF], tr);
            Lane::template get_trans<1>(&recs[(size_t)s * NF], dt_of(s), tb);
            L.template fwd<true, 1>(tb, H, mu, y, is_na(y[0], any_nan), ld, accq, &recs[(size_t)s * NF]);
        }
        out[0] += 0.5 * (ld.value() + accq);
        typename Lane::Adj A;
        A.zero();
        for (int64_t s = nrows[m] - 1; s >= 1; s--) {
            const int64_t i = row0[m] + s;
            double mu[D], y[D], H[3];
            for (int c = 0; c < D; c++) { mu[c] = parmat[i + (int64_t)c * n]; y[c] = obs[i + c * n]; }
            H_of(i, H);
            AdjRowGrad<2> g;
            Lane::template bwd<1>(A, &recs[(size_t)s * NF], H, mu, y, dt_of(s), g);
            for (int c = 0; c < D; c++) G[i + (int64_t)c * n] = g.gmu[c];
            G[i + (int64_t)D * n] = g.g1;
            if (q > D + 1) G[i + (int64_t)(D + 1) * n] = g.g2;
            if (!harr) out[1] += 2.0 * h * g.gh;
        }
    }
}

// fixed-interval smoother (ssde_smooth.hpp over ssde_dense.hpp): each track the way one lane of dense_kernel's record mode /
// smooth_tv_record_kernel and then smooth_back_kernel walk it -- a plain record per state row, then the backward recursion.
// The problem as hostsim_records.hpp has it.  mean (n x SD), cov (n x SD x SD), resid (n x d), row-major, written on state rows only.
template <int MODEL, int D>
void run_smooth(const TwinProblem& pb, double* mean, double* cov, double* resid) {
    typedef SmoothRec<MODEL, D> RC;
    constexpr int SD = RC::SD, R = RC::R;
    const int64_t* row0 = pb.row0;
    std::vector<double> recs;
    for (int64_t m = 0; m < pb.n_tracks; m++) {
        const int64_t ns = twin_record_track<MODEL, D>(pb, m, recs);
        if (ns <= 0) continue;
        double r[SD], N[SD][SD];
        for (int a = 0; a < SD; a++) { r[a] = 0.0; for (int b = 0; b < SD; b++) N[a][b] = 0.0; }
        for (int64_t s = ns - 1; s >= 0; s--) {
            const double* rp = &recs[(size_t)s * R];
            double am[SD], V[SD][SD];
            smooth_back_row<MODEL, D, SD>(r, N, s == ns - 1, [&](int k) -> double { return rp[k]; }, am, V);
            const int64_t i = row0[m] + 1 + s;
            for (int a = 0; a < SD; a++) {
                mean[i * SD + a] = am[a];
                for (int b = 0; b < SD; b++) cov[(i * SD + a) * SD + b] = V[a][b];
            }
            for (int c = 0; c < D; c++) resid[i * D + c] = rp[RC::E + c];
        }
    }
}

}  // namespace

extern "C" {

int hostsim_smooth(int model, int d, TWIN_PARAMS, double* mean, double* cov, double* resid) {
#define SM(MODEL, D) if (model == MODEL && d == D) { run_smooth<MODEL, D>(TWIN_ARGS, mean, cov, resid); return 0; }
    TWIN_D12(SM) TWIN_D38(SM)
#undef SM
    return 1;
}

// out = [nllk (data term), d/d direction_0 .. d/d direction_{nd-1}]
int hostsim_kalman_tv(int model, int d, int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows,
                      const double* times, const double* obs, const double* parmat, int q, int nd, const int* kinds,
                      const int* dims, const double* wmat, double log_sigma_obs, const double* p0, const double* a0,
                      double* out) {
#define TV(MODEL, D) if (model == MODEL && d == D) { run_tv<MODEL, D>(any_nan, n, n_tracks, row0, nrows, times, obs, parmat, q, nd, kinds, dims, wmat, log_sigma_obs, p0, a0, out); return 0; }
    TV(M_CTCRW, 1) TV(M_CTCRW, 2) TV(M_OU_SSM, 1) TV(M_OU_SSM, 2) TV(M_BM_SSM, 1) TV(M_BM_SSM, 2)
#undef TV
    return 1;
}

// out = [nllk (data term), d / d log_sigma_obs]; G (n x q, column-major) = d nllk / d parmat
int hostsim_kalman_adj(int model, int d, int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows,
                       const double* times, const double* obs, const double* parmat, int q, double log_sigma_obs, const double* p0,
                       const double* a0, double* out, double* G) {
#define ADJ(MODEL, D) if (model == MODEL && d == D) { run_adj<MODEL, D>(any_nan, n, n_tracks, row0, nrows, times, obs, parmat, q, log_sigma_obs, p0, a0, out, G); return 0; }
    ADJ(M_CTCRW, 1) ADJ(M_CTCRW, 2) ADJ(M_OU_SSM, 1) ADJ(M_OU_SSM, 2) ADJ(M_BM_SSM, 1) ADJ(M_BM_SSM, 2)
#undef ADJ
    return 1;
}

int hostsim_kalman_adj_full(int model, int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows,
                            const double* times, const double* obs, const double* parmat, int q, double log_sigma_obs, const double* p0f,
                            const double* a0, const double* harr, double* out, double* G) {
#define ADJF(MODEL) if (model == MODEL) { run_adj_full<MODEL>(any_nan, n, n_tracks, row0, nrows, times, obs, parmat, q, log_sigma_obs, p0f, a0, harr, out, G); return 0; }
    ADJF(M_CTCRW) ADJF(M_OU_SSM) ADJF(M_BM_SSM)
#undef ADJF
    return 1;
}

// out = [nllk, g_sig, g_mu_0.., g_p1, g_p2]  (1 + 3 + d doubles)
int hostsim_kalman_iso(int model, int d, int mask, int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0,
                       const int64_t* nrows, const double* times, const double* obs, const double* theta /* ls, mu[d], p1, p2 */,
                       const double* p0, double* out) {
    IsoArgs A;
    A.model = model; A.d = d; A.mask = mask; A.any_nan = any_nan; A.n = n; A.n_tracks = n_tracks;
    A.row0 = row0; A.nrows = nrows; A.times = times; A.obs = obs;
    A.log_sigma_obs = theta[0];
    A.mu[0] = theta[1]; A.mu[1] = d > 1 ? theta[2] : 0.0;
    A.p1 = theta[1 + d]; A.p2 = theta[2 + d];
    A.p0[0] = p0[0]; A.p0[1] = p0[1]; A.p0[2] = p0[2];
    if (d == 1) run_mask<1>(A, out);
    else if (d == 2) run_mask<2>(A, out);
    else return 1;
    return 0;
}

// log I_q(x) and its derivatives w.r.t. x and q (CIR); out = [value, d/dx, d/dq]
void hostsim_log_bessel_i(double x, double q, double* out) { out[0] = log_bessel_i(x, q, out[1], out[2]); }
// ... with the second derivatives (the CIR Hessian, k_direct_hess.hip); out = [value, l_x, l_q, l_xx, l_xq, l_qq]
void hostsim_log_bessel_i2(double x, double q, double* out) {
    double d5[5];
    out[0] = log_bessel_i2(x, q, d5);
    for (int i = 0; i < 5; i++) out[1 + i] = d5[i];
}
// CIR transition: returns nll and adds gradient wrt (log mu, log beta, log sigma)
double hostsim_cir(double z0, double z1, double dt, double lmu, double lb, double ls, double* g) {
    return cir_direct(z0, z1, dt, lmu, lb, ls, g[0], g[1], g[2]);
}

// direct families, one transition: returns nll and adds gradient wrt (mu, p1, p2)
double hostsim_direct(int model, double z0, double z1, double dt, double mu, double p1, double p2, double* g) {
    if (model == M_BM) return bm_direct(z0, z1, dt, mu, p1, g[0], g[1]);
    return ou_direct(z0, z1, dt, mu, p1, p2, g[0], g[1], g[2]);
}

// The engine's knobs as the current environment sets them (csrc/ssde_knobs.hpp), one NAME=value line each ("unset" where an
// absent variable is a state of its own).  Returns the text's length; nothing is written when it does not fit into cap bytes.
int hostsim_knobs(int win_align, char* buf, int cap) {
    const ssde_engine::Knobs k = ssde_engine::knobs_from_env(win_align);
    std::ostringstream o;
    o.precision(17);
    auto put = [&](const char* name, const auto& v) { o << "SSDE_" << name << '=' << v << '\n'; };
    auto opt = [&](const char* name, const auto& v) { if (v) put(name, *v); else put(name, "unset"); };
    put("NO_QUIET", k.no_quiet); put("QUIET_ALWAYS", k.quiet_always); put("NO_NA_SORT", k.no_na_sort);
    put("NO_SHARED", k.no_shared); put("NO_TV", k.no_tv); put("NO_DIRECT_FAST", k.no_direct_fast); put("NO_GRAPH", k.no_graph);
    put("NO_DERIVE", k.no_derive); put("NO_LATTICE", k.no_lattice); put("NO_REGROUP", k.no_regroup);
    put("NO_DRIFT", k.no_drift); put("NO_DRIFT_GENERAL", k.no_drift_general); put("NO_DRIFT_PP", k.no_drift_pp);
    put("DRIFT_PP_ALL", k.drift_pp_all); put("NO_COLVAR", k.no_colvar); put("NO_COLVAR_FULL", k.no_colvar_full);
    put("CV_NO_SHARE", k.cv_no_share); put("CV_NO_MU_COLS", k.cv_no_mu_cols); put("CV_NO_FEW", k.cv_no_few);
    put("TV_NO_LEAN", k.tv_no_lean); put("NO_EXACT_HESS", k.no_exact_hess); put("PUBLISH", k.publish); put("TRACE", k.trace);
    opt("CHUNKS", k.chunks); opt("WINDOW", k.window); opt("ADJ_TAIL", k.adj_tail); opt("TV_WAVES", k.tv_waves);
    opt("TV_MINLEN", k.tv_minlen); opt("HESS_WINDOW", k.hess_window); put("QUIET_WINDOW", k.quiet_window); opt("ISO_SPLIT", k.iso_split);
    opt("DRIFT_MIN_TRACKS", k.drift_min_tracks); opt("CV_ADJ", k.cv_adj); opt("LAGSTATS", k.lagstats);
    opt("FUSED_FINALIZE", k.fused_finalize); put("GRID_RTOL", k.grid_rtol); put("ADJ_DIAG", k.adj_diag);
    opt("WAVE_CLOCK", k.wave_clock);
    const std::string t = o.str();
    if ((int)t.size() < cap) memcpy(buf, t.c_str(), t.size() + 1);
    return (int)t.size();
}

}  // extern "C"

// ---- the window policy (csrc/ssde_windows.hpp): thin entry points for tests/test_windows_host.py ---------------------------------
namespace {
using namespace ssde_engine;

// the order of hostsim_lib.WINDOW_FACTS; window < 0: SSDE_WINDOW unset
WindowFacts facts_from(const double* v) {
    WindowFacts f;
    f.model = (int)v[0]; f.uniform_dt = v[1] != 0.0; f.dt_uniform = v[2]; f.dt_min = v[3]; f.dt_max = v[4];
    f.max_chunks = (int)v[5]; f.want_chunks = (int)v[6]; f.want_chunks_d = (int)v[7]; f.glen_max = (int)v[8]; f.n_groups = (int)v[9];
    f.use_shared = v[10] != 0.0; f.drift = (int)v[11]; f.cv_adj = v[12] != 0.0; f.cv_one_wave = v[13] != 0.0; f.chunks_forced = v[14] != 0.0;
    if (v[15] >= 0.0) f.window = (int)v[15];
    f.cv_eta_lo[0] = v[16]; f.cv_eta_lo[1] = v[17]; f.cv_eta_hi[0] = v[18]; f.cv_eta_hi[1] = v[19];
    f.any_dirty = v[20] != 0.0; f.quiet_ok = v[21] != 0.0; f.lag_ready = v[22] != 0.0; f.quiet_window = (int)v[23]; f.block_rows = (int)v[24];
    return f;
}
WindowConsts consts_from(const int* c) { return WindowConsts{c[0], c[1], c[2], c[3]}; }
WindowParams params_from(const double* v) { return WindowParams{v[0], v[1], v[2], v[3], {v[4], v[5], v[6]}}; }
void put_plan(const WindowPlan& p, double* out) { out[0] = p.n_chunks; out[1] = p.window; out[2] = p.warmup; out[3] = p.rho; }

// a policy with one stand-in engine's chunk limits under it
struct PolicySim {
    WindowPolicy p;
    WindowPolicy::Call c;
    int max_chunks = 1, want_chunks = 1, saved_max_chunks = 0, saved_want_chunks = 0;
};
}  // namespace

extern "C" {

double hostsim_closed_loop_rho(int model, double dt, double p1, double p2, double hobs, const double* p0) {
    return closed_loop_rho(model, dt, p1, p2, hobs, p0);
}
// the transformed parameters of an evaluation at working-scale p1 = par[d], p2 = par[d + 1], decoded as eval_iso decodes them
void hostsim_window_params(int model, double p1, double p2, double hobs, const double* p0, double* out) {
    double tau = 0.0, beta = 0.0, sigma = 0.0;
    if (model == M_CTCRW) { tau = exp(p1); const double nu = exp(p2); beta = 1.0 / tau; sigma = 2.0 * nu / sqrt(M_PI * tau); }
    else if (model == M_OU_SSM) { tau = exp(p1); sigma = exp(p2); }
    else sigma = exp(p1);
    out[0] = tau; out[1] = beta; out[2] = sigma; out[3] = hobs; out[4] = p0[0]; out[5] = p0[1]; out[6] = p0[2];
}
// out = [n_chunks, window, warmup, rho]
void hostsim_window_plan(const double* facts, const int* consts, const double* params, int boost, double* out) {
    put_plan(plan_windows(facts_from(facts), consts_from(consts), params_from(params), boost), out);
}
// ev = [n_parts, can_derive, hess_req, gain_last, gain_usable]; out = the first plan (4), the plan in force (4), then
// [n_chunks, window, t0, t0_delta, dual, n_chunks_d, t0_d, lag_K, s_stat, quiet_window, quiet_w, quiet_b0]
void hostsim_window_geometry(const double* facts, const int* consts, const double* params, int boost, int gave_up, const double* ev,
                             double* out) {
    const WindowFacts f = facts_from(facts);
    const WindowConsts c = consts_from(consts);
    const WindowParams a = params_from(params);
    const WindowPlan first = plan_windows(f, c, a, boost);
    WindowEval e;
    e.n_parts = (int)ev[0]; e.can_derive = ev[1] != 0.0; e.hess_req = ev[2] != 0.0; e.gain_last = (int)ev[3]; e.gain_usable = ev[4] != 0.0;
    const WindowGeometry g = window_geometry(f, c, a, first, boost, gave_up != 0, e);
    put_plan(first, out); put_plan(g.plan, out + 4);
    const double v[12] = {(double)g.n_chunks, (double)g.window, (double)g.t0, (double)g.t0_delta, g.dual ? 1.0 : 0.0, (double)g.n_chunks_d,
                          (double)g.t0_d, (double)g.lag_K, (double)g.s_stat, (double)g.quiet_window, (double)g.quiet_w, (double)g.quiet_b0};
    for (int i = 0; i < 12; i++) out[8 + i] = v[i];
}
// the aligned warm-up of a planner (knob < 0: SSDE_WINDOW unset)
int64_t hostsim_warmup(double rho, int slack, int knob, int boost, int align) {
    return align_rows(warmup_rows(rho, slack, knob >= 0 ? std::optional<int>(knob) : std::nullopt, boost), align);
}
int hostsim_balanced_window0(int glen, int nc, int window, int can_derive, int win_align) {
    return balanced_window0(glen, nc, window, can_derive != 0, win_align);
}

// ---- the Hessian pass's plan (csrc/ssde_windows.hpp) -------------------------------------------------------------------------------
int hostsim_hess_first_warmup(int tv_window, int knob, int win_align) {
    return hess_first_warmup(tv_window, knob >= 0 ? std::optional<int>(knob) : std::nullopt, win_align);
}
int hostsim_hess_next_warmup(int W, int attempt, int glen_max) { return hess_next_warmup(W, attempt, glen_max); }
// items = [track, c, nc, block] per work item; returns their number (nothing is written past cap items)
int64_t hostsim_hess_item_plan(const int32_t* track_steps, int64_t M, int n_pb, int W, int waves, int win_align, int32_t* items, int64_t cap) {
    struct Item { int32_t track, c, nc, b; };
    std::vector<Item> v;
    hess_item_plan(track_steps, M, n_pb, W, waves, win_align, v);
    for (size_t k = 0; k < v.size() && (int64_t)k < cap; k++) { items[4 * k] = v[k].track; items[4 * k + 1] = v[k].c; items[4 * k + 2] = v[k].nc; items[4 * k + 3] = v[k].b; }
    return (int64_t)v.size();
}

// where the reverse sweep's rows lie in the tile (ssde_adj.hpp: what k_iso_adj.hip forms a row's address from)
int64_t hostsim_adj_row_bytes(int C) { return adj_row_bytes(C); }
int64_t hostsim_adj_row_offset(int row, int C) { return adj_row_offset(row, C); }
int64_t hostsim_adj_window_span(int rows, int C) { return adj_window_span(rows, C); }

void* hostsim_policy_new(int max_chunks, int want_chunks) {
    PolicySim* s = new PolicySim();
    s->max_chunks = max_chunks; s->want_chunks = want_chunks;
    return s;
}
void hostsim_policy_free(void* h) { delete (PolicySim*)h; }
void hostsim_policy_begin(void* h) { ((PolicySim*)h)->c = WindowPolicy::Call(); }
// one attempt's outcome; applies what the verdict asks of the engines; returns retry | action << 1
int hostsim_policy_attempt(void* h, double check, int finite, int one_window, int dist, int replans) {
    PolicySim* s = (PolicySim*)h;
    const WindowPolicy::Verdict v = s->p.after_attempt(s->c, {check, finite != 0, one_window != 0, dist != 0, replans != 0});
    apply_chunks(*s, v.engines);
    return (v.retry ? 1 : 0) | ((int)v.engines << 1);
}
int hostsim_policy_end(void* h, int finite, int forced) {
    PolicySim* s = (PolicySim*)h;
    const ChunkAction a = s->p.end_call(s->c, finite != 0, forced != 0);
    apply_chunks(*s, a);
    return (int)a;
}
void hostsim_policy_widen(void* h, int factor) { ((PolicySim*)h)->p.widen(factor); }
void hostsim_policy_relax(void* h) { ((PolicySim*)h)->p.relax(); }
// the order of hostsim_lib.POLICY_STATE
void hostsim_policy_state(void* h, double* out) {
    const PolicySim* s = (const PolicySim*)h;
    const double v[15] = {(double)s->p.window_boost, s->p.gave_up ? 1.0 : 0.0, (double)s->p.calm, (double)s->p.cooldown, (double)s->p.probe_from,
                          s->p.probing ? 1.0 : 0.0, s->p.check_floor, s->p.check_max, s->p.last_check, (double)s->p.n_retries,
                          (double)s->c.attempt, (double)s->max_chunks, (double)s->want_chunks, (double)s->saved_max_chunks, (double)s->saved_want_chunks};
    for (int i = 0; i < 15; i++) out[i] = v[i];
}

}  // extern "C"
