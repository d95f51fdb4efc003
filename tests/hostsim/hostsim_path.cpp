// hostsim_path.cpp -- TEST INFRASTRUCTURE, not an engine.
//
// Compiles smoothsde_amd/csrc/ssde_path.hpp (the lane math of k_path_stats.hip) over ssde_draws.hpp / ssde_smooth.hpp with g++ and
// walks each track the way one lane of the kernels does: smooth_record_row -> dense_step per state row, then draw_factor_row,
// draw_step and path_step per draw from the last record to the first, path_finish at the end.  tests/test_path_hostsim.py compares
// it with tests/path_ref.py on the draws of tests/draws_ref.py.
#include "../../smoothsde_amd/csrc/ssde_path.hpp"
#include "hostsim_records.hpp"

using namespace ssde;

namespace {

// the problem as hostsim_records.hpp has it; is_row: n flags (the row is a row of the caller's data) or NULL (every row is);
// weight: n or NULL (1); regions: n_regions x 4.  out (n_draws x n_tracks x n_stat, row-major) is written for tracks with a state
// row only.
template <int MODEL, int D>
void run_path(const TwinProblem& pb, uint64_t seed, int64_t draw0, int n_draws, const uint8_t* is_row, const double* weight,
              const double* regions, int n_regions, double* out) {
    typedef SmoothRec<MODEL, D> RC;
    typedef DrawFac<MODEL, D> FC;
    constexpr int SD = RC::SD, R = RC::R;
    std::vector<double> recs;
    for (int64_t m = 0; m < pb.n_tracks; m++) {
        const int64_t ns = twin_record_track<MODEL, D>(pb, m, recs);
        if (ns <= 0) continue;
        std::vector<double> al((size_t)n_draws * SD, 0.0);
        std::vector<PathAcc<D>> acc((size_t)n_draws);
        for (auto& a : acc) path_init<D>(a);
        const int n_stat = 2 + n_regions;
        DrawNext<SD> nx;
        draw_next_init<SD>(nx);
        for (int64_t s = ns - 1; s >= 0; s--) {
            const double* rp = &recs[(size_t)s * R];
            const bool tail = s == ns - 1;
            double fac[FC::R];
            draw_factor_row<MODEL, D, SD>([&](int k) -> double { return rp[k]; }, tail, nx, [&](int k) -> double& { return fac[k]; });
            const int64_t i = pb.row0[m] + 1 + s;
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
            for (int k = 0; k < n_stat; k++) out[((int64_t)q * pb.n_tracks + m) * n_stat + k] = st[k];
        }
    }
}

}  // namespace

extern "C" {

int hostsim_path(int model, int d, TWIN_PARAMS, uint64_t seed, int64_t draw0, int n_draws, const uint8_t* is_row, const double* weight,
                 const double* regions, int n_regions, double* out) {
    if (n_regions < 0 || n_regions > PATH_NREG) return 2;
#define PR(MODEL, D) if (model == MODEL && d == D) { run_path<MODEL, D>(TWIN_ARGS, seed, draw0, n_draws, is_row, weight, regions, n_regions, out); return 0; }
    TWIN_D12(PR)
#undef PR
    return 1;
}

}  // extern "C"
