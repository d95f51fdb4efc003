// hostsim_prox.hpp -- the walk of k_path_prox.hip's two kernels on the host, over csrc/ssde_prox.hpp (see hostsim_prox.cpp).
#ifndef HOSTSIM_PROX_HPP
#define HOSTSIM_PROX_HPP

#include <cstdint>
#include <vector>

#include "../../smoothsde_amd/csrc/ssde_occ.hpp"
#include "../../smoothsde_amd/csrc/ssde_prox.hpp"

template <int MODEL, int D>
void hostsim_prox_run(const double* pos, int64_t n_point, int n_draws, const int64_t* pair_ptr, int64_t n_pairs, const double* weight,
                      const double* radii, int n_radii, double* stats) {
    using namespace ssde;
    typedef DenseDims<MODEL, D> DM;
    constexpr int SD = DM::SD, WV = 64, NW = PROX_TILE / WV;
    const int64_t nq = 2 * n_point;
    const int n_stat = 2 + n_radii;
    // the call's quantum and the weights in quanta, as the engine forms them
    double wmax = weight ? 0.0 : 1.0;
    for (int64_t i = 0; weight && i < n_point; i++) wmax = weight[i] > wmax ? weight[i] : wmax;
    const int e = occ_quantum_exp(wmax, n_point, 1);
    const uint64_t unit = occ_quantise(1.0, e);
    std::vector<uint64_t> wq;
    if (weight) { wq.resize((size_t)n_point); occ_quantise_all(weight, n_point, e, wq.data()); }
    const ProxPlan P = plan_prox_tiles(pair_ptr, n_pairs);
    const int64_t n_rec = P.n_tiles * (int64_t)n_draws;
    std::vector<uint64_t> part((size_t)n_rec * PROX_REC + 1);
    // prox_tile_kernel: block = tile + n_tiles * draw
    for (int64_t blk = 0; blk < n_rec; blk++) {
        const int64_t tile = blk % P.n_tiles, q = blk / P.n_tiles;
        const int cnt = P.tile_count[(size_t)tile];
        ProxAcc lane[PROX_TILE];
        for (int t = 0; t < PROX_TILE; t++) {
            prox_init(lane[t]);
            if (t >= cnt) continue;
            const int64_t i = P.tile_first[(size_t)tile] + t;
            const double* base = pos + nq * SD * q + i;
            double pa[D], pb[D];
            for (int c = 0; c < D; c++) {
                pa[c] = base[(int64_t)DM::z(c) * nq];
                pb[c] = base[(int64_t)DM::z(c) * nq + n_point];
            }
            prox_step<D>(lane[t], pa, pb, P.tile_idx0[(size_t)tile] + t, weight ? wq[(size_t)i] : unit,
                         [&](int r) { return radii[r]; }, n_radii);
        }
        // the wave's xor butterfly: every lane combines with the lane `o` away, all at once
        for (int w = 0; w < NW; w++)
            for (int o = 32; o > 0; o >>= 1) {
                ProxAcc was[WV];
                for (int l = 0; l < WV; l++) was[l] = lane[w * WV + l];
                for (int l = 0; l < WV; l++) prox_combine(lane[w * WV + l], was[l ^ o]);
            }
        uint64_t lds[NW * PROX_REC];
        for (int w = 0; w < NW; w++) prox_store(lane[w * WV], lds + w, NW);
        ProxAcc a = lane[0];
        for (int k = 1; k < NW; k++) {
            ProxAcc b;
            prox_load(b, lds + k, NW);
            prox_combine(a, b);
        }
        prox_store(a, part.data() + tile + P.n_tiles * q, n_rec);
    }
    // prox_fold_kernel: lane = (pair, draw)
    for (int64_t t = 0; t < n_pairs * (int64_t)n_draws; t++) {
        const int64_t p = t % n_pairs, q = t / n_pairs;
        ProxAcc a;
        prox_init(a);
        for (int64_t k = P.pair_tile[(size_t)p]; k < P.pair_tile[(size_t)p + 1]; k++) {
            ProxAcc b;
            prox_load(b, part.data() + k + P.n_tiles * q, n_rec);
            prox_combine(a, b);
        }
        double out[PROX_NSTAT_MAX];
        prox_finish(a, n_radii, e, out);
        for (int k = 0; k < n_stat; k++) stats[p + n_pairs * (k + (int64_t)n_stat * q)] = out[k];
    }
}

#endif
