// occ_fine_san.cpp -- TEST INFRASTRUCTURE: plan_all_slots, plan_fine_weights, occ_fine_batch_cap (ssde_smooth_plan.hpp) and the slot
// loop of the host twin of ssde_path_occupancy_fine (tests/hostsim/hostsim_occ_fine.hpp: what one thread of path_occ_fine_kernel
// does) under the sanitizers, as a program of its own
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o build/occ_fine_san tools/occ_fine_san.cpp && build/occ_fine_san
// on the inputs of tests/test_occ_fine_plan_host.py in small: lanes of 9, 1, 2, 3 and 7 rows, one without a state row, one left out
// (group -1); intervals from a quarter of max_step to a hundred times it (the cap), a NaN and a zero interval; with and without a
// lattice row map (padded rows, one before a lane's first caller row) and weights; then every (slot, draw) for the three models and
// one and two columns from made-up ends and the Philox deviates, a rejected row (NaN interval) and a NaN end among them, with the
// sum of the quanta checked against the weights placed.
#include <cmath>
#include <cstdio>

#include "../smoothsde_amd/csrc/ssde_smooth_plan.hpp"
#include "../tests/hostsim/hostsim_occ_fine.hpp"

using namespace ssde;
using namespace ssde_plan;

template <int MODEL, int D>
static uint64_t slots_all(const QueryPlan& P, const FineWeights& F, const std::vector<double>& sdt, const std::vector<int32_t>& ns,
                          const OccGrid& grid, int n_draws) {
    typedef BridgePk<MODEL, D> BK;
    constexpr int SD = BK::SD, Q = BK::Q, SW = BK::SW;
    std::vector<uint64_t> cells((size_t)grid.nx * grid.ny, 0);
    uint64_t outside = 0, placed = 0;
    for (int64_t l = 0; l + 1 < (int64_t)P.want_off.size(); l++)
        for (int64_t slot = P.want_off[l]; slot < P.want_off[l + 1]; slot++) {
            const int s = P.want_step[(size_t)slot];
            double pk[SW], left[SD], right[SD];
            for (int j = 0; j < Q; j++) pk[BK::PAR + j] = j < D ? 0.1 * (j + 1) : 0.3 - 0.2 * (j - D);
            pk[BK::DT] = s == ns[(size_t)l] - 1 ? PREDICT_DT_TAIL : sdt[(size_t)slot];
            if (slot % 7 == 3) pk[BK::DT] = NAN;                         // a row that rejected its update
            for (int c = 0; c < SD; c++) { left[c] = 0.3 * c - 0.1 * s; right[c] = left[c] + 0.2; }
            if (slot % 11 == 5) right[0] = NAN;                          // a NaN end
            for (int q = 0; q < n_draws; q++) {
                occ_fine_slot<MODEL, D>(pk, left, right, F.m[(size_t)slot], F.own[(size_t)slot], F.share[(size_t)slot], 7, (uint64_t)l,
                                        (uint32_t)s, (uint32_t)(3 + q), grid, cells.data(), &outside);
                placed += F.own[(size_t)slot] + F.share[(size_t)slot] * (uint64_t)(F.m[(size_t)slot] - 1);
            }
        }
    uint64_t sum = outside;
    for (uint64_t v : cells) sum += v;
    if (sum != placed) { printf("quanta lost: %llu placed, %llu counted\n", (unsigned long long)placed, (unsigned long long)sum); return 0; }
    return sum + 1;
}

int main() {
    const std::vector<int32_t> ns = {8, 0, 1, 2, 6, 4}, grp = {0, 0, 1, 0, -1, 1};
    std::vector<int64_t> row0;
    int64_t n = 0;
    for (int32_t v : ns) { row0.push_back(n); n += v + 1; }
    const QueryPlan P = plan_all_slots(ns, grp);
    const int64_t n_slots = (int64_t)P.want_step.size();
    const QueryPlan none = plan_all_slots({}, {});
    const double dts[9] = {0.25, 0.5, 1.5, 2.5, 100.0, NAN, 0.0, 4.5, 64.0};
    std::vector<double> sdt((size_t)n_slots);
    for (int64_t i = 0; i < n_slots; i++) sdt[(size_t)i] = dts[i % 9];
    std::vector<uint64_t> wq((size_t)n);
    for (int64_t i = 0; i < n; i++) wq[(size_t)i] = (uint64_t)(i * 7919 % 1000);
    std::vector<int64_t> row_map((size_t)n, -1);
    int64_t k = 0;
    for (int64_t i = 0; i < n; i++) if (i % 3 != 1 || i == 0) row_map[(size_t)i] = k++;      // (row 1, lane 0's first state row: padded)
    const OccGrid g1{-1.0, 0.25, 0.0, 1.0, 9, 1}, g2{-1.0, 0.25, -0.5, 0.3, 9, 7};
    double total = (double)none.want_off.size();
    for (double max_step : {1.0, 0.3, (double)INFINITY})
        for (int variant = 0; variant < 3; variant++) {
            const FineWeights F = plan_fine_weights(P, row0, sdt, max_step, 64, variant == 1 ? row_map.data() : nullptr,
                                                    variant == 2 ? nullptr : wq.data(), (uint64_t)1 << 40);
            printf("max_step %g variant %d: %lld slots, %lld points, %lld capped\n", max_step, variant, (long long)n_slots,
                   (long long)F.n_points, (long long)F.n_capped);
            const uint64_t sums[6] = {slots_all<M_CTCRW, 1>(P, F, sdt, ns, g1, 3), slots_all<M_CTCRW, 2>(P, F, sdt, ns, g2, 3),
                                      slots_all<M_OU_SSM, 1>(P, F, sdt, ns, g1, 3), slots_all<M_OU_SSM, 2>(P, F, sdt, ns, g2, 3),
                                      slots_all<M_BM_SSM, 1>(P, F, sdt, ns, g1, 3), slots_all<M_BM_SSM, 2>(P, F, sdt, ns, g2, 3)};
            for (uint64_t v : sums) { if (v == 0) return 1; total += (double)v; }
        }
    for (int nd : {1, 5, 1 << 27})
        for (int64_t budget : {(int64_t)0, (int64_t)1 << 20, (int64_t)1 << 50}) total += occ_fine_batch_cap(budget, n_slots, 8, 4, nd);
    if (!std::isfinite(total)) { printf("a non-finite total\n"); return 1; }
    printf("occ_fine ok (%.0f)\n", total);
    return 0;
}
