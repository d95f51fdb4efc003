// bridge_san.cpp -- TEST INFRASTRUCTURE: smoothsde_amd/csrc/ssde_bridge.hpp and plan_slot_offsets (ssde_smooth_plan.hpp) under the
// sanitizers, as a program of its own
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o build/bridge_san tools/bridge_san.cpp && build/bridge_san
// on the inputs of tests/test_predict_draws_plan_host.py and test_predict_draws_hostsim.py in small: the tracks 9, 1, 2, 3, 7 with, per
// row, 1, 2 or 5 distinct offsets, 0, the interval, duplicates and a forecast chain; then every slot's offsets chained by
// bridge_slot_walk for the three models and one and two columns, from made-up ends and the Philox deviates; a rejected row (NaN
// interval) and a slot whose offsets pass the next fix among them.
#include <cmath>
#include <cstdio>

#include "../smoothsde_amd/csrc/ssde_bridge.hpp"
#include "../smoothsde_amd/csrc/ssde_smooth_plan.hpp"

using namespace ssde;
using namespace ssde_plan;

template <int MODEL, int D>
static double walk_all(const QueryPlan& P, const SlotOffsets& S, const std::vector<int32_t>& ns, int64_t nq, std::vector<double>& out) {
    constexpr int SD = DenseDims<MODEL, D>::SD, Q = DenseDims<MODEL, D>::Q;
    out.assign((size_t)nq * SD, NAN);
    double sum = 0.0;
    for (int64_t l = 0; l + 1 < (int64_t)P.want_off.size(); l++)
        for (int64_t slot = P.want_off[l]; slot < P.want_off[l + 1]; slot++) {
            const int s = P.want_step[(size_t)slot];
            DualN<0> par[Q];
            for (int j = 0; j < Q; j++) par[j] = DualN<0>(j < D ? 0.1 * (j + 1) : 0.3 - 0.2 * (j - D));
            double left[SD], right[SD];
            for (int c = 0; c < SD; c++) { left[c] = 0.3 * c - 0.1 * s; right[c] = left[c] + 0.2; }
            double dt = s == ns[(size_t)l] - 1 ? PREDICT_DT_TAIL : 0.5;
            if (slot % 7 == 3) dt = NAN;                                 // a row that rejected its update
            const int64_t g0 = S.off_ptr[(size_t)slot], n_off = S.off_ptr[(size_t)slot + 1] - g0;
            bridge_slot_walk<MODEL, D>(
                par, dt, left, right, n_off, [&](int64_t r) -> double { return S.off_val[(size_t)(g0 + r)]; },
                [&](int64_t r, double (&z)[SD]) { bridge_deviates<SD>(7, (uint64_t)l, (uint32_t)s, (uint32_t)r, 3, 0, z); },
                [&](int64_t r, const double (&x)[SD]) {
                    for (int64_t k = S.q_ptr[(size_t)(g0 + r)]; k < S.q_ptr[(size_t)(g0 + r) + 1]; k++)
                        for (int c = 0; c < SD; c++) { out[(size_t)S.q_dest[(size_t)k] * SD + c] = x[c]; sum += x[c]; }
                });
        }
    return sum;
}

int main() {
    const int lengths[5] = {9, 1, 2, 3, 7};
    std::vector<int64_t> row0, q_row;
    std::vector<int32_t> ns;
    std::vector<double> q_off;
    int64_t n = 0;
    for (int T : lengths) {
        row0.push_back(n);
        ns.push_back(T - 1);
        for (int j = 0; j < T; j++) {
            if (j == T - 1) { for (double f : {6.0, 0.0, 0.25, 1.7, 0.25}) { q_row.push_back(n + j); q_off.push_back(f); } continue; }
            switch (j % 4) {
                case 0: for (double f : {0.5}) { q_row.push_back(n + j); q_off.push_back(f * 0.5); } break;
                case 1: for (double f : {0.8, 0.3}) { q_row.push_back(n + j); q_off.push_back(f * 0.5); } break;
                case 2: for (double f : {0.9, 0.1, 0.5, 0.25, 0.75, 1.5}) { q_row.push_back(n + j); q_off.push_back(f * 0.5); } break;
                default: for (double f : {0.4, -0.0, 1.0, 0.4, 0.0}) { q_row.push_back(n + j); q_off.push_back(f * 0.5); } break;
            }
        }
        n += T;
    }
    const int64_t nq = (int64_t)q_row.size();
    const QueryPlan P = plan_queries(row0, ns, nullptr, 0.0, q_row.data(), q_off.data(), nq);
    const SlotOffsets S = plan_slot_offsets(P);
    printf("%zu of %lld queries planned on %zu slots, %zu distinct offsets, the longest list %lld\n", P.order.size(), (long long)nq,
           P.want_step.size(), S.off_val.size(), (long long)S.most);
    const SlotOffsets none = plan_slot_offsets(plan_queries({}, {}, nullptr, 0.0, nullptr, nullptr, 0));
    double sum = (double)none.q_ptr.size();
    std::vector<double> out;
    sum += walk_all<M_CTCRW, 1>(P, S, ns, nq, out) + walk_all<M_CTCRW, 2>(P, S, ns, nq, out);
    sum += walk_all<M_OU_SSM, 1>(P, S, ns, nq, out) + walk_all<M_OU_SSM, 2>(P, S, ns, nq, out);
    sum += walk_all<M_BM_SSM, 1>(P, S, ns, nq, out) + walk_all<M_BM_SSM, 2>(P, S, ns, nq, out);
    for (int nd : {1, 5, 1 << 27})
        for (int64_t budget : {(int64_t)0, (int64_t)1 << 20, (int64_t)1 << 50}) sum += predict_draws_batch_cap(budget, (int64_t)P.want_step.size(), 4, nq, 4, nd);
    if (!std::isfinite(sum)) { printf("a non-finite answer\n"); return 1; }
    printf("bridge ok (%.6f)\n", sum);
    return 0;
}
