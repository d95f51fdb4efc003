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
    // a parent of two track shards (3 and 4 rows) x two column pairs (sd = 4 from engines of sd = 2): the deal of five queries of
    // which the first shard gets none, the placement by rows and by queries with a row NaN in one pair and a row NaN in both, the
    // statistics of 2 and 3 tracks with a NaN row of a maximum, offsets with runs of 1, 2 and 3 distinct values
    const int64_t N = 7, rows[2][2] = {{0, 3}, {3, 4}}, qr[5] = {4, 6, 3, 5, 4};
    const double qo[5] = {0.5, 0.0, 1.25, 0.5, 0.75}, nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> mean((size_t)N * 4, nan), cov((size_t)N * 16, 0.0), qmean(5 * 4, nan), qcov(5 * 16, 0.0);
    for (int t = 0; t < 2; t++)
        for (int pair = 0; pair < 2; pair++) {
            const int64_t lo = rows[t][0], m = rows[t][1];
            std::vector<double> a((size_t)m * 2, 1.0 + pair), V((size_t)m * 4, 2.0 + pair);
            if (t == 1) { V[2] = nan; if (pair == 0) V[1] = nan; }
            place_columns(mean.data(), N, 2 * pair, a.data(), m, 2, lo);
            place_cov_block(cov.data(), N, 4, 2 * pair, V.data(), m, 2, lo);
            const QueryDeal D = deal_queries(lo, m, qr, qo, 5);
            const int64_t mq = (int64_t)D.idx.size();
            std::vector<double> qa((size_t)mq * 2, 3.0), qV((size_t)mq * 4, 4.0);
            if (mq) qV[0] = nan;
            place_columns(qmean.data(), 5, 2 * pair, qa.data(), mq, 2, 0, D.idx.data());
            place_cov_block(qcov.data(), 5, 4, 2 * pair, qV.data(), mq, 2, 0, D.idx.data());
            place_block(qcov.data(), 5, 4, 2 * pair, qV.data(), mq, 2, 0, D.idx.data());
            sum += mq;
        }
    for (double v : mean) sum += (int64_t)v;
    for (double v : cov) sum += std::isnan(v) ? 1 : 0;
    for (double v : qcov) sum += std::isnan(v) ? 1 : 0;
    std::vector<double> stats(5 * 4 * 3, nan), s2(2 * 4 * 3, 5.0), s3(3 * 4 * 3, 6.0);
    s3[2 + 3 * 2] = nan;
    place_track_stats(stats.data(), 5, 0, s2.data(), 2, 4, 3, 2, 0);
    place_track_stats(stats.data(), 5, 2, s3.data(), 3, 4, 3, 2, 40);
    place_track_stats(stats.data(), 5, 2, s3.data(), 3, 4, 3, -1, 40);
    for (double v : stats) sum += std::isnan(v) ? 1 : (int64_t)v;
    const int64_t r1[3] = {7, 7, 7}, r2[4] = {3, 9, 3, 3}, r3[6] = {5, 2, 5, 5, 5, 2};
    const double o1[3] = {0.5, 0.5, 0.5}, o2[4] = {0.25, 0.1, 0.0, 0.25}, o3[6] = {0.3, 0.0, 0.1, 0.2, 0.3, 0.0};
    const int64_t most[3] = {max_distinct_offsets(r1, o1, 3), max_distinct_offsets(r2, o2, 4), max_distinct_offsets(r3, o3, 6)};
    if (most[0] != 1 || most[1] != 2 || most[2] != 3 || max_distinct_offsets(nullptr, nullptr, 0) != 0) { printf("max_distinct_offsets is off\n"); return 1; }
    for (int64_t limit : {(int64_t)3, (int64_t)4})
        for (int k = 0; k < 3; k++) sum += most[k] + 1 >= limit ? 1 : 0;
    printf("plan ok (%lld)\n", (long long)sum);
    return 0;
}
