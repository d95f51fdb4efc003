// plan_san.cpp -- TEST INFRASTRUCTURE: smoothsde_amd/csrc/ssde_smooth_plan.hpp under the sanitizers, as a program of its own
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o build/plan_san tools/plan_san.cpp && build/plan_san
// on the inputs of tests/test_smooth_plan_host.py in small: the tracks 9, 1, 2, 3, 7
// on their own rows and on a lattice of 0.5, the lanes in both orders, queries on every row; then the chunk plan and the batch caps.
#include <cstdio>

#include "../smoothsde_amd/csrc/ssde_smooth_plan.hpp"

using namespace ssde_plan;

int main() {
    const int lengths[5] = {9, 1, 2, 3, 7}, inc[8] = {1, 3, 2, 4, 1, 2, 4, 3};
    int64_t sum = 0;
    for (int lattice = 0; lattice < 2; lattice++)
        for (int reverse = 0; reverse < 2; reverse++) {
            std::vector<int64_t> row0, pad_row, q_row;
            std::vector<int32_t> ns;
            std::vector<double> q_off;
            int64_t n = 0, p = 0;
            for (int T : lengths) {
                int64_t k = 0;
                row0.push_back(lattice ? p : n);
                for (int j = 0; j < T; j++) {
                    if (j > 0) k += lattice ? inc[(j - 1) % 8] : 1;
                    pad_row.push_back(p + k);
                    const double dt = j + 1 < T ? 0.5 * (lattice ? inc[j % 8] : 1) : 1.0;
                    for (double f : {6.0, 1.5, 1.0, 0.98, 0.37, 0.37, 0.0}) { q_row.push_back(n + j); q_off.push_back(f * dt); }
                }
                ns.push_back((int32_t)k);
                n += T; p += k + 1;
            }
            if (reverse) { std::reverse(row0.begin(), row0.end()); std::reverse(ns.begin(), ns.end()); }
            const QueryPlan P = plan_queries(row0, ns, lattice ? pad_row.data() : nullptr, 0.5, q_row.data(), q_off.data(), (int64_t)q_row.size());
            for (int wave : {2, 64})
                for (int g = 0; g * wave < 5; g++) { const QueryRange r = chunk_queries(P, g, g + 1, wave); sum += r.s1 - r.s0 + r.q1 - r.q0; }
            printf("lattice %d reverse %d: %zu of %zu queries planned on %zu slots\n", lattice, reverse, P.order.size(), q_row.size(), P.want_step.size());
        }
    sum += (int64_t)plan_queries({}, {}, nullptr, 0.0, nullptr, nullptr, 0).want_off.size();
    std::vector<int64_t> goff(1, 0);
    for (int g = 0; g < 40; g++) goff.push_back(goff.back() + (int64_t)(1 + g * 7 % 13) * 31 * 64);
    for (int64_t budget : {(int64_t)1, (int64_t)100000, goff.back(), (int64_t)1 << 40}) sum += (int64_t)chunk_groups(goff, budget).size();
    for (int64_t budget : {(int64_t)0, (int64_t)999, (int64_t)1 << 40})
        for (int64_t per : {(int64_t)0, (int64_t)37, (int64_t)100000})
            for (int nd : {1, 3, 1000, 1 << 27}) sum += batch_cap(budget, per, 1, 4, nd) + batch_cap(budget, per, 4, 4, nd);
    printf("plan ok (%lld)\n", (long long)sum);
    return 0;
}
