// hostsim_bands.cpp -- TEST INFRASTRUCTURE: the lane math of ssde_par_bands (csrc/ssde_bands.hpp) built for the host (bands.mk ->
// libhostsim_bands.so, loaded by tests/bandsim_lib.py).  The walk itself is hostsim_bands.hpp.
#include "hostsim_bands.hpp"

extern "C" int hostsim_bands(int64_t n, int q, const int32_t* ncol_fe, const double* const* x_fe, const int32_t* ncol_re,
                             const double* const* x_re, const uint8_t* link, const double* coeff, int n_post, int resp, double level,
                             double z, double* est, double* pw_low, double* pw_upp, double* se, double* sim_low, double* sim_upp,
                             double* crit, double* max_dev) {
    const ssde::TwinBands T{n, q, ncol_fe, x_fe, ncol_re, x_re, link, coeff, n_post, resp, level, z};
    return ssde::hostsim_bands_run(T, est, pw_low, pw_upp, se, sim_low, sim_upp, crit, max_dev, [](auto&&, int) {});
}

// the plan of a call: the order statistics each tail needs (m_lo, m_up) -- what ssde_par_bands holds against SSDE_BANDS_MAX_TAIL
extern "C" void hostsim_bands_plan(int n_post, double level, int32_t* m_lo, int32_t* m_up) {
    const ssde::BandsPlan P = ssde::bands_plan(n_post, level);
    *m_lo = P.m_lo; *m_up = P.m_up;
}
