// hostsim_occ_fine.hpp -- TEST INFRASTRUCTURE, not an engine.
//
// One (slot, draw) of ssde_path_occupancy_fine the way one thread of path_occ_fine_kernel (k_path_occ_fine.hip) runs it: `own` at the
// cell of the left end, then, where share != 0 and m > 1, bridge_slot_walk over the offsets ((r + 1) * dt) / m with `share` at every
// emitted point's cell and the share of every rank that is not emitted outside.  Shared by the host twin (hostsim_occ_fine.cpp) and
// the sanitizer program (tools/occ_fine_san.cpp).
#ifndef HOSTSIM_OCC_FINE_HPP
#define HOSTSIM_OCC_FINE_HPP

#include "../../smoothsde_amd/csrc/ssde_bridge.hpp"
#include "../../smoothsde_amd/csrc/ssde_occ.hpp"

// par: the slot's side packet (BridgePk::SW doubles); left / right: the draw's ends; cells: the output grid's nx * ny counters;
// *outside: its counter of the quanta in no cell
template <int MODEL, int D>
void occ_fine_slot(const double* pk, const double* left_, const double* right_, int m, uint64_t own, uint64_t share, uint64_t seed,
                   uint64_t track, uint32_t s, uint32_t draw, const ssde::OccGrid& grid, uint64_t* cells, uint64_t* outside) {
    using namespace ssde;
    typedef BridgePk<MODEL, D> BK;
    typedef DenseDims<MODEL, D> DM;
    constexpr int SD = BK::SD, Q = BK::Q;
    auto add = [&](const double (&x)[SD], uint64_t w) {
        double p[D];
        for (int c = 0; c < D; c++) p[c] = x[DM::z(c)];
        const int cell = occ_cell<D>(p, grid);
        if (cell < 0) *outside += w;
        else cells[cell] += w;
    };
    const double dt = pk[BK::DT];
    double left[SD], right[SD];
    for (int c = 0; c < SD; c++) { left[c] = left_[c]; right[c] = dt < 0.0 ? 0.0 : right_[c]; }
    if (own) add(left, own);
    if (share == 0 || m <= 1) return;
    DualN<0> par[Q];
    for (int j = 0; j < Q; j++) par[j] = DualN<0>(pk[BK::PAR + j]);
    const double dm = (double)m;
    int emitted = 0;
    bridge_slot_walk<MODEL, D>(
        par, dt, left, right, (int64_t)(m - 1), [&](int64_t r) -> double { return ((double)(r + 1) * dt) / dm; },
        [&](int64_t r, double (&z)[SD]) { bridge_deviates<SD>(seed, track, s, (uint32_t)r, draw, 0, z); },
        [&](int64_t, const double (&x)[SD]) { emitted++; add(x, share); });
    *outside += share * (uint64_t)(m - 1 - emitted);
}

#endif
