// hostsim_loo.cpp -- TEST INFRASTRUCTURE, not an engine.
//
// Compiles smoothsde_amd/csrc/ssde_loo.hpp (the lane math of k_smooth_loo.hip) with g++ through hostsim_loo.hpp's walk, for the three
// Kalman families at every width the engine instantiates.  tests/test_loo_hostsim.py compares it with tests/loo_ref.py.
#include "hostsim_loo.hpp"

extern "C" {

// 0: done; 1: no such model and width; 2: a bad threshold count
int hostsim_loo(int model, int d, TWIN_PARAMS, const int64_t* crow, const double* thr, int n_thr, double* mean, double* cov,
                double* resid, double* lpd, double* stats) {
    using namespace ssde;
    if (n_thr < 0 || n_thr > LOO_NTHR) return 2;
#define LO(MODEL, D) if (model == MODEL && d == D) { hostsim_loo_run<MODEL, D>(TWIN_ARGS, crow, thr, n_thr, mean, cov, resid, lpd, stats); return 0; }
    TWIN_D12(LO) TWIN_D38(LO)
#undef LO
    return 1;
}

}  // extern "C"
