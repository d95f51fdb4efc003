// hostsim_speed.cpp -- TEST INFRASTRUCTURE, not an engine.
//
// Compiles smoothsde_amd/csrc/ssde_speed.hpp (the lane math of k_path_speed.hip) with g++ through hostsim_speed.hpp's walk.
// tests/test_speed_hostsim.py compares it with tests/speed_ref.py on the draws of tests/draws_ref.py.
#include "hostsim_speed.hpp"

extern "C" {

// 0: done; 1: not a CTCRW of one or two response columns; 2: a bad threshold count
int hostsim_speed(int model, int d, TWIN_PARAMS, uint64_t seed, int64_t draw0, int n_draws, const int64_t* crow, int64_t n_out,
                  const double* weight, const double* thr, int n_thr, double* stats, uint32_t* below) {
    if (n_thr < 0 || n_thr > ssde::SPEED_NTHR) return 2;
    if (model != ssde::M_CTCRW) return 1;
    if (d == 1) { hostsim_speed_run<ssde::M_CTCRW, 1>(TWIN_ARGS, seed, draw0, n_draws, crow, n_out, weight, thr, n_thr, stats, below); return 0; }
    if (d == 2) { hostsim_speed_run<ssde::M_CTCRW, 2>(TWIN_ARGS, seed, draw0, n_draws, crow, n_out, weight, thr, n_thr, stats, below); return 0; }
    return 1;
}

}  // extern "C"
