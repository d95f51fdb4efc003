// hostsim_path.cpp -- TEST INFRASTRUCTURE, not an engine.
//
// Compiles smoothsde_amd/csrc/ssde_path.hpp (the lane math of k_path_stats.hip) over ssde_draws.hpp / ssde_smooth.hpp with g++ and
// walks each track the way one lane of the kernels does: smooth_record_row -> dense_step per state row, then draw_factor_row,
// draw_step and path_step per draw from the last record to the first, path_finish at the end.  tests/test_path_hostsim.py compares
// it with tests/path_ref.py on the draws of tests/draws_ref.py.
#include <cstdint>
#include <vector>

#include "../../smoothsde_amd/csrc/ssde_path.hpp"

using namespace ssde;

namespace {

// parmat: n x q row-major linear predictors; harr: n x d x d (row-major per row) or NULL (h I); p0f: SD x SD column-major;
// a0: n_tracks x SD; is_row: n flags (the row is a row of the caller's data) or NULL (every row is); weight: n or NULL (1);
// regions: n_regions x 4.  out (n_draws x n_tracks x n_stat, row-major) is written for tracks with a state row only.
template <int MODEL, int D>
void run_path(int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows, const double* times,
               const double* obs, const double* parmat, const double* harr, double h, const double* p0f, const double* a0,
               uint64_t seed, int64_t draw0, int n_draws, const uint8_t* is_row, const double* weight, const double* regions, int n_regions,
               double* out) {
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
        std::vector<PathAcc<D>> acc((size_t)n_draws);
        for (auto& a : acc) path_init<D>(a);
        const int n_stat = 2 + n_regions;
        DrawNext<SD> nx = {};
        for (int64_t s = ns - 1; s >= 0; s--) {
            const double* rp = &recs[(size_t)s * R];
            const bool tail = s == ns - 1;
            double fac[FC::R];
            draw_factor_row<MODEL, D, SD>([&](int k) -> double { return rp[k]; }, tail, nx, [&](int k) -> double& { return fac[k]; });
            const int64_t i = row0[m] + 1 + s;
            for (int q = 0; q < n_draws; q++) {
                double z[SD], a[SD];
                draw_deviates<SD>(seed, (uint64_t)m, (uint32_t)s, (uint32_t)(draw0 + q), 0, z);
                for (int c = 0; c < SD; c++) a[c] = al[(size_t)q * SD + c];
                draw_step<MODEL, D, SD>([&](int k) -> double { return fac[k]; }, tail, a, z);
                for (int c = 0; c < SD; c++) al[(size_t)q * SD + c] = a[c];
                path_step<MODEL, D, SD>(acc[q], a, is_row ? is_row[i] != 0 : true, weight ? weight[i] : 1.0,
                                        [&](int k) -> double { return regions[k]; }, n_regions);
            }
        }
        for (int q = 0; q < n_draws; q++) {
            double st[PATH_NSTAT_MAX];
            path_finish<D>(acc[q], n_regions, st);
            for (int k = 0; k < n_stat; k++) out[((int64_t)q * n_tracks + m) * n_stat + k] = st[k];
        }
    }
}

}  // namespace

extern "C" {

int hostsim_path(int model, int d, int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows,
                 const double* times, const double* obs, const double* parmat, const double* harr, double h, const double* p0f,
                 const double* a0, uint64_t seed, int64_t draw0, int n_draws, const uint8_t* is_row, const double* weight,
                 const double* regions, int n_regions, double* out) {
    if (n_regions < 0 || n_regions > PATH_NREG) return 2;
#define PR(MODEL, D) if (model == MODEL && d == D) { run_path<MODEL, D>(any_nan, n, n_tracks, row0, nrows, times, obs, parmat, harr, h, p0f, a0, seed, draw0, n_draws, is_row, weight, regions, n_regions, out); return 0; }
    PR(M_CTCRW, 1) PR(M_CTCRW, 2) PR(M_OU_SSM, 1) PR(M_OU_SSM, 2) PR(M_BM_SSM, 1) PR(M_BM_SSM, 2)
#undef PR
    return 1;
}

}  // extern "C"
