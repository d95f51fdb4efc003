// hostsim_draws.cpp -- TEST INFRASTRUCTURE, not an engine.
//
// Compiles smoothsde_amd/csrc/ssde_draws.hpp (the lane math of k_smooth_draws.hip) over ssde_smooth.hpp / ssde_dense.hpp with g++
// and walks each track the way one lane of the kernels does: smooth_record_row -> dense_step per state row, then draw_factor_row
// and draw_step per draw from the last record to the first.  tests/test_draws_hostsim.py compares it with tests/draws_ref.py.
#include "../../smoothsde_amd/csrc/ssde_draws.hpp"
#include "hostsim_records.hpp"

using namespace ssde;

namespace {

// the problem as hostsim_records.hpp has it; normals: n_draws x n x SD (indexed by the row) or NULL (Philox, track = the segment's
// ordinal).  out (n_draws x n x SD, row-major) is written on state rows only.
template <int MODEL, int D>
void run_draws(const TwinProblem& pb, uint64_t seed, int64_t draw0, int n_draws, const double* normals, double* out) {
    typedef SmoothRec<MODEL, D> RC;
    typedef DrawFac<MODEL, D> FC;
    constexpr int SD = RC::SD, R = RC::R;
    const int64_t n = pb.n;
    std::vector<double> recs;
    for (int64_t m = 0; m < pb.n_tracks; m++) {
        const int64_t ns = twin_record_track<MODEL, D>(pb, m, recs);
        if (ns <= 0) continue;
        std::vector<double> al((size_t)n_draws * SD, 0.0);
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

int hostsim_draws(int model, int d, TWIN_PARAMS, uint64_t seed, int64_t draw0, int n_draws, const double* normals, double* out) {
#define DR(MODEL, D) if (model == MODEL && d == D) { run_draws<MODEL, D>(TWIN_ARGS, seed, draw0, n_draws, normals, out); return 0; }
    TWIN_D12(DR)
#undef DR
    return 1;
}

int hostsim_draws_fac_doubles(int model, int d) {
#define DF(MODEL, D) if (model == MODEL && d == D) return DrawFac<MODEL, D>::R;
    TWIN_D12(DF)
#undef DF
    return 0;
}

}  // extern "C"
