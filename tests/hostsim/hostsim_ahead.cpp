// hostsim_ahead.cpp -- TEST INFRASTRUCTURE, not an engine.
//
// Compiles smoothsde_amd/csrc/ssde_ahead.hpp (the lane math of k_smooth_ahead.hip) with g++ through hostsim_ahead.hpp's walk, for the
// three Kalman families at the widths the engine instantiates, and exports the call's host plan (ssde_smooth_plan.hpp: the block
// plan, the partial records counted against the budget, the horizon validation).  tests/test_ahead_host.py compares the twin with
// tests/ahead_ref.py and tests the plan.
#include "hostsim_ahead.hpp"

extern "C" {

// 0: done; 1: no such model and width; 2: a bad threshold count or horizon list
int hostsim_ahead(int model, int d, TWIN_PARAMS, const int64_t* crow, const int32_t* hz, int n_h, const double* thr, int n_thr,
                  double* z, double* lpd, double* stats) {
    using namespace ssde;
    if (n_thr < 0 || n_thr > AHEAD_NTHR || ssde_plan::check_horizons(hz, n_h, SSDE_AHEAD_MAX_H, SSDE_AHEAD_MAX_STEP)) return 2;
#define AH(MODEL, D) if (model == MODEL && d == D) { hostsim_ahead_run<MODEL, D>(TWIN_ARGS, crow, hz, n_h, thr, n_thr, z, lpd, stats); return 0; }
    TWIN_D12(AH)
#undef AH
    return 1;
}

int hostsim_ahead_block() { return ssde_plan::AHEAD_BLOCK; }
int64_t hostsim_ahead_blocks(int64_t steps) { return ssde_plan::ahead_blocks(steps); }
int64_t hostsim_ahead_partial_doubles(int64_t steps, int n_h, int n_stat) { return ssde_plan::ahead_partial_doubles(steps, n_h, n_stat, 64); }
int hostsim_ahead_check_horizons(const int32_t* hz, int n_h) {
    return ssde_plan::check_horizons(hz, n_h, SSDE_AHEAD_MAX_H, SSDE_AHEAD_MAX_STEP);
}
// blk_off (G + 1) from the groups' state rows
void hostsim_ahead_block_offsets(const int64_t* steps, int G, int64_t* blk_off) {
    const std::vector<int64_t> off = ssde_plan::ahead_block_offsets(std::vector<int64_t>(steps, steps + G));
    std::copy(off.begin(), off.end(), blk_off);
}
// The chunks of G groups under `budget` doubles as the engine cuts them for this call: every group costs its records and side rows
// (steps * (R + SW) * 64) and its partial records.  cut (room for G + 1) receives the chunks' first groups and G; returns the chunks.
int hostsim_ahead_chunks(const int64_t* steps, int G, int R, int SW, int n_h, int n_stat, int64_t budget, int* cut) {
    std::vector<int64_t> cost((size_t)G + 1, 0);
    for (int g = 0; g < G; g++)
        cost[(size_t)g + 1] = cost[(size_t)g] + steps[g] * (R + SW) * 64 + ssde_plan::ahead_partial_doubles(steps[g], n_h, n_stat, 64);
    const std::vector<int> c = ssde_plan::chunk_groups(cost, budget);
    std::copy(c.begin(), c.end(), cut);
    return (int)c.size() - 1;
}

}  // extern "C"
