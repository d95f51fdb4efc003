// prox_san.cpp -- TEST INFRASTRUCTURE: the tile plan and the walk of ssde_path_proximity's kernels (csrc/ssde_prox.hpp through
// hostsim_prox.hpp) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (prox.mk builds it with
// -fsanitize=address,undefined; tests/test_prox_hostsim.py runs it).  Pair sizes 0, 1, 255, 256, 257 and 600 in one list, every model
// and width, with and without weights, a NaN point and 0 / 8 radii; it checks the plan's tables, and the twin's minimum, index and
// counts against a plain loop.  Exit status 0 and "prox_san ok" when nothing is wrong.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "hostsim_prox.hpp"

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { fails++; std::fprintf(stderr, "prox_san: line %d: %s\n", __LINE__, #c); } } while (0)

uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
double unif() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) / 9007199254740992.0;
}

template <int MODEL, int D>
void run_case(bool weights, int n_radii, bool with_nan) {
    using namespace ssde;
    constexpr int SD = DenseDims<MODEL, D>::SD;
    const int64_t sizes[] = {0, 1, 255, 256, 257, 600};
    const int n_pairs = 6, n_draws = 3;
    std::vector<int64_t> ptr(1, 0);
    for (int64_t s : sizes) ptr.push_back(ptr.back() + s);
    const int64_t np = ptr.back(), nq = 2 * np;
    const ProxPlan P = plan_prox_tiles(ptr.data(), n_pairs);
    EXPECT(P.n_tiles == 0 + 1 + 1 + 1 + 2 + 3 && P.tiles_max == 3);
    int64_t covered = 0;
    for (int64_t i = 0; i < P.n_tiles; i++) {
        const int64_t p = P.tile_pair[(size_t)i];
        EXPECT(P.tile_first[(size_t)i] >= ptr[(size_t)p] && P.tile_first[(size_t)i] + P.tile_count[(size_t)i] <= ptr[(size_t)p + 1]);
        EXPECT(P.tile_idx0[(size_t)i] == P.tile_first[(size_t)i] - ptr[(size_t)p]);
        EXPECT(P.tile_count[(size_t)i] >= 1 && P.tile_count[(size_t)i] <= PROX_TILE);
        EXPECT(i >= P.pair_tile[(size_t)p] && i < P.pair_tile[(size_t)p + 1]);
        covered += P.tile_count[(size_t)i];
    }
    EXPECT(covered == np);
    std::vector<double> pos((size_t)nq * SD * n_draws), w((size_t)np), stats((size_t)n_pairs * (2 + n_radii) * n_draws);
    for (double& x : pos) x = 4.0 * unif() - 2.0;
    for (double& x : w) x = unif();
    const int64_t bad_point = ptr[4] + 256;                                        // in the pair of 257, its second tile
    if (with_nan) pos[(size_t)(bad_point + nq * (DenseDims<MODEL, D>::z(0) + SD * 1))] = std::nan("");     // draw 1, side A
    double radii[PROX_NRAD];
    for (int r = 0; r < PROX_NRAD; r++) radii[r] = r == 7 ? INFINITY : 0.25 * (r + 1);
    hostsim_prox_run<MODEL, D>(pos.data(), np, n_draws, ptr.data(), n_pairs, weights ? w.data() : nullptr, radii, n_radii, stats.data());
    const int n_stat = 2 + n_radii;
    for (int q = 0; q < n_draws; q++)
        for (int p = 0; p < n_pairs; p++) {
            const double* st = stats.data() + p + n_pairs * ((int64_t)n_stat * q);
            const bool nan = sizes[p] == 0 || (with_nan && q == 1 && p == 4);
            if (nan) { for (int k = 0; k < n_stat; k++) EXPECT(std::isnan(st[(int64_t)n_pairs * k])); continue; }
            double best = INFINITY;
            int64_t arg = -1, within = 0;
            for (int64_t i = ptr[(size_t)p]; i < ptr[(size_t)p + 1]; i++) {
                double pa[D], pb[D];
                for (int c = 0; c < D; c++) {
                    pa[c] = pos[(size_t)(i + nq * (DenseDims<MODEL, D>::z(c) + SD * q))];
                    pb[c] = pos[(size_t)(i + np + nq * (DenseDims<MODEL, D>::z(c) + SD * q))];
                }
                const double dist = path_dist<D>(pa, pb);
                if (dist < best) { best = dist; arg = i - ptr[(size_t)p]; }
                if (n_radii > 0 && dist <= radii[0]) within++;
            }
            EXPECT(st[0] == best && st[n_pairs] == (double)arg);
            if (n_radii > 0 && !weights) EXPECT(st[(int64_t)n_pairs * 2] == (double)within);
            if (n_radii == PROX_NRAD && !weights) EXPECT(st[(int64_t)n_pairs * 9] == (double)sizes[p]);
        }
}

}  // namespace

int main() {
    using namespace ssde;
    for (int wt = 0; wt < 2; wt++)
        for (int nr : {0, 1, PROX_NRAD})
            for (int bad = 0; bad < 2; bad++) {
                run_case<M_CTCRW, 1>(wt, nr, bad); run_case<M_CTCRW, 2>(wt, nr, bad);
                run_case<M_OU_SSM, 1>(wt, nr, bad); run_case<M_OU_SSM, 2>(wt, nr, bad);
                run_case<M_BM_SSM, 1>(wt, nr, bad); run_case<M_BM_SSM, 2>(wt, nr, bad);
            }
    if (fails) { std::fprintf(stderr, "prox_san: %d checks failed\n", fails); return 1; }
    std::printf("prox_san ok\n");
    return 0;
}
