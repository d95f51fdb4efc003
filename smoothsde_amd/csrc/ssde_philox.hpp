// ssde_philox.hpp -- the normal deviates of the simulators (ssde_simulate, k_sim.hip; ssde_simulate_rows, k_sim_rows.hip): Philox4x32-10
// as a counter-based generator, two 53-bit uniforms of one block, Box-Muller.  A deviate is a pure function of the four counter words
// and the two key words; what the counter words mean is the caller's (k_sim.hip: row, track low, track high, stream; k_sim_rows.hip: row
// position in the track, track ordinal, replicate number, stream).  Host- and device-compilable: the device takes sincospi, a host
// build sin / cos of 2 pi u, which is what the numpy restatement (tests/sim_ref.py) does.
#ifndef SSDE_PHILOX_HPP
#define SSDE_PHILOX_HPP

#include <math.h>
#include <stdint.h>

#include "ssde_math.hpp"

namespace ssde {

SSDE_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// two independent N(0, 1) deviates of the counter (c0, c1, c2, c3) under the key (k0, k1)
SSDE_HD void philox_normal_pair(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, double& n1, double& n2) {
    uint32_t o[4];
    philox4x32_10(c0, c1, c2, c3, k0, k1, o);
    const double u1 = ((double)((((uint64_t)o[0] << 32) | o[1]) >> 11) + 0.5) * 0x1.0p-53;     // (0, 1)
    const double u2 = ((double)((((uint64_t)o[2] << 32) | o[3]) >> 11) + 0.5) * 0x1.0p-53;
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
#if defined(__HIP_DEVICE_COMPILE__)
    sincospi(2.0 * u2, &s, &c);
#else
    const double a = 2.0 * 3.141592653589793 * u2;
    s = sin(a); c = cos(a);
#endif
    n1 = r * c; n2 = r * s;
}

}  // namespace ssde
#endif
