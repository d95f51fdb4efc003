// hostsim_simrows.cpp -- TEST INFRASTRUCTURE: the lane math of ssde_simulate_rows (csrc/ssde_simrows.hpp) built for the host
// (simrows.mk -> libhostsim_simrows.so, loaded by tests/simrowsim_lib.py).  The walk itself is hostsim_simrows.hpp.
#include "hostsim_simrows.hpp"

extern "C" int hostsim_simrows(int kind, int d, int n_par, int64_t n, int64_t n_tracks, const int64_t* row0, const double* times,
                               const int32_t* ncol_fe, const double* const* x_fe, const int32_t* ncol_re, const double* const* x_re,
                               const uint8_t* link, const double* coeff, int n_coeff_rows, int n_coef, const double* sigma_obs,
                               const double* z0, uint64_t seed, int64_t rep0, int64_t n_rep, const double* thr, int n_thr,
                               double* obs, double* stats) {
    const ssde::TwinSimrows T{kind, d, n_par, n, n_tracks, row0, times, ncol_fe, x_fe, ncol_re, x_re, link, coeff, n_coeff_rows, n_coef,
                              sigma_obs, z0, seed, rep0, n_rep, thr, n_thr};
    return ssde::hostsim_simrows_run(T, obs, stats);
}

// the factors of one transition: out = (e, 1 - e, a, l11, l21, l22, sd) -- what the tests hold against the literal formulas
extern "C" void hostsim_simrows_factors(int kind, double dt, double p1, double p2, double* out) {
    const ssde::SimrowsFac F = kind == ssde::SIMROWS_CTCRW ? ssde::simrows_factors<ssde::SIMROWS_CTCRW>(dt, p1, p2)
                             : kind == ssde::SIMROWS_OU   ? ssde::simrows_factors<ssde::SIMROWS_OU>(dt, p1, p2)
                                                          : ssde::simrows_factors<ssde::SIMROWS_BM>(dt, p1, p2);
    out[0] = F.e; out[1] = F.ome; out[2] = F.a; out[3] = F.l11; out[4] = F.l21; out[5] = F.l22; out[6] = F.sd;
}
