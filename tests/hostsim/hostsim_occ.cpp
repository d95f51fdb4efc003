// hostsim_occ.cpp -- TEST INFRASTRUCTURE, not an engine.
//
// Compiles smoothsde_amd/csrc/ssde_occ.hpp (the lane math of k_path_occ.hip) over ssde_draws.hpp / ssde_smooth.hpp with g++ and
// walks each track the way one lane of the kernels does: smooth_record_row -> dense_step per state row, then draw_factor_row and
// draw_step per draw from the last record to the first, occ_cell on the drawn position and an integer add of the row's quantised
// weight.  tests/test_occ_hostsim.py compares it bitwise with tests/occ_ref.py on the draws of tests/draws_ref.py;
// tests/test_occ_abi_host.py reaches the quantum rule and the plans of ssde_smooth_plan.hpp through the small entry points below.
#include "../../smoothsde_amd/csrc/ssde_occ.hpp"
#include "../../smoothsde_amd/csrc/ssde_smooth_plan.hpp"
#include "hostsim_records.hpp"

using namespace ssde;

namespace {

// the problem as hostsim_records.hpp has it; is_row: n flags (the row is a row of the caller's data) or NULL (every row is);
// wq: n quantised weights; group: n_tracks labels or NULL (0).  counts: nx * ny * n_groups cells, then n_groups for the outside.
template <int MODEL, int D>
void run_occ(const TwinProblem& pb, uint64_t seed, int64_t draw0, int n_draws, const uint8_t* is_row, const uint64_t* wq,
             const int32_t* group, int n_groups, const OccGrid& grid, uint64_t* counts) {
    typedef SmoothRec<MODEL, D> RC;
    typedef DrawFac<MODEL, D> FC;
    typedef DenseDims<MODEL, D> DM;
    constexpr int SD = RC::SD, R = RC::R;
    const int64_t ncell = (int64_t)grid.nx * grid.ny;
    std::vector<double> recs;
    for (int64_t m = 0; m < pb.n_tracks; m++) {
        const int64_t ns = twin_record_track<MODEL, D>(pb, m, recs);
        const int og = group ? group[m] : 0;
        if (ns <= 0 || og < 0) continue;
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
                draw_deviates<SD>(seed, (uint64_t)m, (uint32_t)s, (uint32_t)(draw0 + q), 0, z);
                for (int c = 0; c < SD; c++) a[c] = al[(size_t)q * SD + c];
                draw_step<MODEL, D, SD>([&](int k) -> double { return fac[k]; }, tail, a, z);
                for (int c = 0; c < SD; c++) al[(size_t)q * SD + c] = a[c];
                if (is_row && !is_row[i]) continue;
                double p[D];
                for (int c = 0; c < D; c++) p[c] = a[DM::z(c)];
                const int cell = occ_cell<D>(p, grid);
                if (cell < 0) counts[ncell * n_groups + og] += wq[i];
                else counts[cell + ncell * og] += wq[i];
            }
        }
    }
}

}  // namespace

extern "C" {

int hostsim_occ(int model, int d, TWIN_PARAMS, uint64_t seed, int64_t draw0, int n_draws, const uint8_t* is_row, const uint64_t* wq,
                const int32_t* group, int n_groups, const double* grid4, int nx, int ny, uint64_t* counts) {
    if (nx < 1 || ny < 1 || n_groups < 1 || (d == 1 && ny != 1)) return 2;
    const OccGrid g{grid4[0], grid4[1], grid4[2], grid4[3], nx, ny};
#define OC(MODEL, D) if (model == MODEL && d == D) { run_occ<MODEL, D>(TWIN_ARGS, seed, draw0, n_draws, is_row, wq, group, n_groups, g, counts); return 0; }
    TWIN_D12(OC)
#undef OC
    return 1;
}

int hostsim_occ_quantum_exp(double wmax, int64_t n, int64_t n_draws) { return occ_quantum_exp(wmax, n, n_draws); }

// fast != 0: the engine's loop over all weights; else the definition, one weight at a time
void hostsim_occ_quantise(const double* w, int64_t n, int e, int fast, uint64_t* out) {
    if (fast) { occ_quantise_all(w, n, e, out); return; }
    for (int64_t i = 0; i < n; i++) out[i] = occ_quantise(w[i], e);
}

int hostsim_occ_batch_cap(int nw, int ch, int n_draws) { return ssde_plan::occ_batch_cap(nw, ch, n_draws); }

// grp_of [ceil(n_lanes / wave)] from lane_grp [n_lanes]
void hostsim_occ_groups(const int32_t* lane_grp, int64_t n_lanes, int wave, int64_t n_cells, int64_t tile_cells, int force_global,
                        int32_t mixed, int32_t* grp_of) {
    const std::vector<int32_t> r = ssde_plan::plan_occ_groups(std::vector<int32_t>(lane_grp, lane_grp + n_lanes), wave, n_cells,
                                                              tile_cells, force_global != 0, mixed);
    for (size_t g = 0; g < r.size(); g++) grp_of[g] = r[g];
}

}  // extern "C"
