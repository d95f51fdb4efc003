// ssde_occ.hpp -- occupancy grids of posterior state paths (ssde_path_occupancy): the cell of a position, the quantum of a call and
// the quantised weight, DESIGN.md §3.13.  The kernel (k_path_occ.hip), the engine and the host twin (tests/hostsim/hostsim_occ.cpp)
// all take them from here.  Host- and device-compilable, like ssde_path.hpp; the quantum rule and the quantisation run on the host
// only.
#ifndef SSDE_OCC_HPP
#define SSDE_OCC_HPP

#include <math.h>
#include <stdint.h>

#include "ssde_draws.hpp"

namespace ssde {

// the grid as the C ABI has it (ssde_occ_grid), by value in the kernel's arguments
struct OccGrid {
    double x0, dx, y0, dy;
    int nx, ny;
};

// floor((p - lo) / step) where it is one of 0 .. n - 1, else -1.  The quotient is an IEEE division (no reciprocal): numpy's
// np.floor((p - lo) / step) is the same number.  NaN and +-inf fail the comparison and are outside.
SSDE_HD int occ_axis(double p, double lo, double step, int n) {
    const double f = floor((p - lo) / step);
    return (f >= 0.0 && f < (double)n) ? (int)f : -1;
}

// the cell ix + nx * iy of a position (p[1], y0 and dy are not read for D = 1), -1 outside the grid
template <int D>
SSDE_HD int occ_cell(const double (&p)[D], const OccGrid& g) {
    const int ix = occ_axis(p[0], g.x0, g.dx, g.nx);
    if (D == 1 || ix < 0) return ix;
    const int iy = occ_axis(p[D - 1], g.y0, g.dy, g.ny);
    return iy < 0 ? -1 : ix + g.nx * iy;
}

// The exponent e of the call's quantum 2^e: wmax the largest weight (1 where there are none), n the rows of the caller's data of the
// WHOLE handle.  With frexp(wmax) = (m, k) and b the bit length of n * n_draws, every weight is below 2^k and enters as at most
// 2^(k - e) = 2^(52 - b), at most n * n_draws < 2^b times: every sum stays below 2^52 and ldexp((double)sum, e) is exact.
inline int occ_quantum_exp(double wmax, int64_t n, int64_t n_draws) {
    int k = 0;
    frexp(wmax, &k);
    int b = 0;
    for (unsigned __int128 v = (unsigned __int128)(uint64_t)n * (uint64_t)n_draws; v; v >>= 1) b++;    // (the product may pass 64 bits)
    const int e = k + b - 52;
    return e > -1074 ? e : -1074;
}

// w as a whole number of quanta, ties to even (the default rounding mode); w finite and >= 0
inline uint64_t occ_quantise(double w, int e) { return (uint64_t)nearbyint(ldexp(w, -e)); }

// the same for n weights at the speed of a copy: where 2^-e is a normal double the product w * 2^-e is ldexp's (a power of two
// scales exactly; a product that underflows rounds to 0 quanta either way), and below 2^52 adding and taking off 2^52 rounds to the
// nearest whole number, ties to even, as nearbyint does
inline void occ_quantise_all(const double* w, int64_t n, int e, uint64_t* out) {
    if (-e > 1023 || -e < -1022) { for (int64_t i = 0; i < n; i++) out[i] = occ_quantise(w[i], e); return; }
    const double scale = ldexp(1.0, -e);
    for (int64_t i = 0; i < n; i++) {
        const double x = w[i] * scale;
        volatile double r = x + 4503599627370496.0;
        out[i] = x < 4503599627370496.0 ? (uint64_t)(r - 4503599627370496.0) : (uint64_t)x;
    }
}

}  // namespace ssde
#endif
