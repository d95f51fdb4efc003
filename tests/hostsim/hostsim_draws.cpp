// hostsim_draws.cpp -- TEST INFRASTRUCTURE, not an engine.
//
// Compiles smoothsde_amd/csrc/ssde_draws.hpp (the lane math of k_smooth_draws.hip) over ssde_smooth.hpp / ssde_dense.hpp with g++
// and walks each track the way one lane of the kernels does: smooth_record_row -> dense_step per state row, then draw_factor_row
// and draw_step per draw from the last record to the first.  tests/test_draws_hostsim.py compares it with tests/draws_ref.py.
#include <cstdint>
#include <vector>

#include "../../smoothsde_amd/csrc/ssde_draws.hpp"

using namespace ssde;

namespace {

// parmat: n x q row-major linear predictors; harr: n x d x d (row-major per row) or NULL (h I); p0f: SD x SD column-major;
// a0: n_tracks x SD; normals: n_draws x n x SD (indexed by the row) or NULL (Philox, track = the segment's ordinal).
// out (n_draws x n x SD, row-major) is written on state rows only.
template <int MODEL, int D>
void run_draws(int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows, const double* times,
               const double* obs, const double* parmat, const double* harr, double h, const double* p0f, const double* a0,
               uint64_t seed, int64_t draw0, int n_draws, const double* normals, double* out) {
    typedef DenseDims<MODEL, D> DM;
    typedef SmoothRec<MODEL, D> RC;
    typedef DrawFac<MODEL, D> FC;
    constexpr int SD = DM::SD, Q = DM::Q, R = RC::R;
    for (int64_t m = 0; m < n_tracks; m++) {
        const int64_t ns = nrows[m] - 1;
        if (ns <= 0) continue;
        DenseLane<MODEL, D, 0> L;
        L.init(a0 + m * SD, p0f);
        std::vector<double> recs((size_t)ns * R);
        for (int64_t s = 0; s < ns; s++) {
            const int64_t i = row0[m] + 1 + s;
            const double dt = (i + 1 < n) ? times[i + 1] - times[i] : 1.0;
            double y[D];
            for (int c = 0; c < D; c++) y[c] = obs[i + c * n];
            DualN<0> H[D][D], par[Q];
            for (int p = 0; p < D; p++)
                for (int q = 0; q < D; q++) H[p][q] = DualN<0>(harr ? harr[(i * D + p) * D + q] : (p == q ? h : 0.0));
            for (int j = 0; j < Q; j++) par[j] = DualN<0>(parmat[i * Q + j]);
            const bool na = is_na(y[0], any_nan);
            double* rp = &recs[(size_t)s * R];
            smooth_record_row<MODEL, D>(L, par, H, dt, y, na, [&](int k) -> double& { return rp[k]; });
            dense_step<MODEL, D, 0>(L, par, H, dt, y, na);
        }
        std::vector<double> al((size_t)n_draws * SD, 0.0);
        DrawNext<SD> nx = {};
        for (int64_t s = ns - 1; s >= 0; s--) {
            const double* rp = &recs[(size_t)s * R];
            const bool tail = s == ns - 1;
            double fac[FC::R];
            draw_factor_row<MODEL, D, SD>([&](int k) -> double { return rp[k]; }, tail, nx, [&](int k) -> double& { return fac[k]; });
            const int64_t i = row0[m] + 1 + s;
            for (int q = 0; q < n_draws; q++) {
                double z[SD], a[SD];
                if (normals) for (int c = 0; c < SD; c++) z[c] = normals[((int64_t)q * n + i) * SD + c];
                else draw_deviates<SD>(seed, (uint64_t)m, (uint32_t)s, (uint32_t)(draw0 + q), 0, z);
                for (int c = 0; c < SD; c++) a[c] = al[(size_t)q * SD + c];
                draw_step<MODEL, D, SD>([&](int k) -> double { return fac[k]; }, tail, a, z);
                for (int c = 0; c < SD; c++) { al[(size_t)q * SD + c] = a[c]; out[((int64_t)q * n + i) * SD + c] = a[c]; }
            }
        }
    }
}

}  // namespace

extern "C" {

int hostsim_draws(int model, int d, int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows,
                  const double* times, const double* obs, const double* parmat, const double* harr, double h, const double* p0f,
                  const double* a0, uint64_t seed, int64_t draw0, int n_draws, const double* normals, double* out) {
#define DR(MODEL, D) if (model == MODEL && d == D) { run_draws<MODEL, D>(any_nan, n, n_tracks, row0, nrows, times, obs, parmat, harr, h, p0f, a0, seed, draw0, n_draws, normals, out); return 0; }
    DR(M_CTCRW, 1) DR(M_CTCRW, 2) DR(M_OU_SSM, 1) DR(M_OU_SSM, 2) DR(M_BM_SSM, 1) DR(M_BM_SSM, 2)
#undef DR
    return 1;
}

int hostsim_draws_fac_doubles(int model, int d) {
#define DF(MODEL, D) if (model == MODEL && d == D) return DrawFac<MODEL, D>::R;
    DF(M_CTCRW, 1) DF(M_CTCRW, 2) DF(M_OU_SSM, 1) DF(M_OU_SSM, 2) DF(M_BM_SSM, 1) DF(M_BM_SSM, 2)
#undef DF
    return 0;
}

}  // extern "C"
