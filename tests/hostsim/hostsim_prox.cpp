// hostsim_prox.cpp -- test-only host build of ssde_path_proximity's lane math and tile plan (csrc/ssde_prox.hpp), a library of its
// own (prox.mk).  It walks the states ssde_predict_draws returns exactly as k_path_prox.hip does: per (tile, draw) 256 lanes form
// their accumulators, each wave of 64 combines by the xor butterfly the kernel's __shfl_xor runs, the four waves combine in order,
// the record goes through prox_store / prox_load, and per (pair, draw) the tiles fold in ascending order into prox_finish.
// hostsim_prox.hpp holds the walk so that the stand-alone sanitizer program (prox_san.cpp) runs the same code.
#include "hostsim_prox.hpp"

extern "C" {

// counts: n_tiles, tiles_max; the tables are caller-allocated for at most `cap` tiles (0: only count)
int hostsim_prox_plan(const int64_t* pair_ptr, int64_t n_pairs, int tile, int64_t cap, int64_t* counts, int64_t* tile_pair,
                      int64_t* tile_first, int64_t* tile_idx0, int32_t* tile_count, int64_t* pair_tile) {
    const ssde::ProxPlan P = ssde::plan_prox_tiles(pair_ptr, n_pairs, tile);
    counts[0] = P.n_tiles; counts[1] = P.tiles_max;
    if (cap == 0) return 0;
    if (cap < P.n_tiles) return 2;
    for (int64_t i = 0; i < P.n_tiles; i++) {
        tile_pair[i] = P.tile_pair[(size_t)i]; tile_first[i] = P.tile_first[(size_t)i];
        tile_idx0[i] = P.tile_idx0[(size_t)i]; tile_count[i] = P.tile_count[(size_t)i];
    }
    for (int64_t p = 0; p <= n_pairs; p++) pair_tile[p] = P.pair_tile[(size_t)p];
    return 0;
}

// pos: [2 n_point x sdim x n_draws] as ssde_predict_draws leaves it; stats: [n_pairs x n_stat x n_draws] as ssde_path_proximity's
int hostsim_prox(int model, int d, const double* pos, int64_t n_point, int n_draws, const int64_t* pair_ptr, int64_t n_pairs,
                 const double* weight, const double* radii, int n_radii, double* stats) {
    if (n_radii < 0 || n_radii > ssde::PROX_NRAD) return 2;
#define PX(MODEL, D) if (model == ssde::MODEL && d == D) { hostsim_prox_run<ssde::MODEL, D>(pos, n_point, n_draws, pair_ptr, n_pairs, weight, radii, n_radii, stats); return 0; }
    PX(M_CTCRW, 1) PX(M_CTCRW, 2) PX(M_OU_SSM, 1) PX(M_OU_SSM, 2) PX(M_BM_SSM, 1) PX(M_BM_SSM, 2)
#undef PX
    return 1;
}

int hostsim_prox_quantum_exp(double wmax, int64_t n_point) { return ssde::occ_quantum_exp(wmax, n_point, 1); }

}  // extern "C"
