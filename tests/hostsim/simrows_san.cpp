// simrows_san.cpp -- TEST INFRASTRUCTURE: the host twin of ssde_simulate_rows (csrc/ssde_simrows.hpp through hostsim_simrows.hpp) as
// a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (simrows.mk builds it with
// -fsanitize=address,undefined; tests/test_simrows_hostsim.py runs it).  Small problems -- tracks of 0, 1, 2, 5 and 33 rows, four
// replicates with a coefficient row each, the three recursions, one to three columns, an intercept-only, a two-column and a
// six-column block -- into buffers of exactly the documented sizes.  It checks what needs no second implementation: every written
// observation is finite and the rows of no track are left unwritten, a track of fewer than two rows is NaN in every statistic and
// no other is, counts are whole numbers in 0 .. rows - 1 and the count under +inf is rows - 1, max L <= sum L, sum D^2 >= 0; one
// replicate simulated alone (rep0 = 2, its own coefficient row) is bitwise the batch's; a log-link linear predictor of 800 in one
// coefficient row makes that replicate's statistics NaN and no other's.  Exit status 0 and "simrows_san ok" when nothing is wrong.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hostsim_simrows.hpp"

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { fails++; std::fprintf(stderr, "simrows_san: line %d: %s\n", __LINE__, #c); } } while (0)

double unit(uint64_t& s) {                                  // a small generator of its own: (-1, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((s >> 11) & 0xFFFFFFFFFFFFull) / (double)0x1000000000000ull * 2.0 - 1.0;
}

void run_case(int kind, int d, bool with_error, bool blow_up) {
    using namespace ssde;
    const int64_t row0[6] = {0, 0, 1, 3, 8, 41};
    const int64_t n = 41, M = 5, R = 4;
    const int q = d + (kind == SIMROWS_BM ? 1 : 2);
    uint64_t s = 77u + (uint64_t)kind * 13u + (uint64_t)d;
    std::vector<double> times((size_t)n), xlin((size_t)n * 2), xsm((size_t)n * 5);
    double t = 0.0;
    for (int64_t i = 0; i < n; i++) { t += 0.05 + 0.8 * (unit(s) + 1.0); times[(size_t)i] = t; xlin[(size_t)i] = 1.0; xlin[(size_t)(n + i)] = unit(s); }
    for (double& e : xsm) e = 0.5 * (unit(s) + 1.0);
    // parameter 0 (mu_1): two fixed columns; the first scale parameter: the intercept and five random columns; the rest: the intercept
    std::vector<int32_t> kf((size_t)q, 1), kr((size_t)q, 0);
    std::vector<const double*> xf((size_t)q, nullptr), xr((size_t)q, nullptr);
    std::vector<uint8_t> link((size_t)q, 0);
    kf[0] = 2; xf[0] = xlin.data();
    kr[(size_t)d] = 5; xr[(size_t)d] = xsm.data();
    int n_coef = 0;
    for (int j = 0; j < q; j++) { link[(size_t)j] = j < d ? 0 : 1; n_coef += kf[(size_t)j] + kr[(size_t)j]; }
    std::vector<double> coeff((size_t)R * n_coef), so((size_t)R);
    for (double& e : coeff) e = 0.4 * unit(s);
    const int off_last = n_coef - kf[(size_t)(q - 1)] - kr[(size_t)(q - 1)];
    if (blow_up) coeff[(size_t)(1 * n_coef + off_last)] = 800.0;                       // replicate 1: the last parameter's intercept, exp(800 + ..)
    for (int64_t k = 0; k < R; k++) so[(size_t)k] = 0.05 * (double)(k + 1);
    const double z0[8] = {0.5, -0.5, 0.25, 0, 0, 0, 0, 0}, thr[2] = {0.5, INFINITY};
    const int n_stat = 3 * d + 2 + 2;
    TwinSimrows T{kind, d, q, n, M, row0, times.data(), kf.data(), xf.data(), kr.data(), xr.data(), link.data(), coeff.data(), (int)R, n_coef,
                  with_error ? so.data() : nullptr, z0, 0x123456789abcdefull, 3, R, thr, 2};
    std::vector<double> obs((size_t)(n * d * R)), stats((size_t)(M * n_stat * R));
    for (double& e : obs) e = std::nan("");
    EXPECT(hostsim_simrows_run(T, obs.data(), stats.data()) == 0);
    for (int64_t k = 0; k < R; k++) {
        const bool blown = blow_up && k == 1;
        if (!blown)
            for (int64_t e = 0; e < n * d; e++) EXPECT(std::isfinite(obs[(size_t)(e + n * d * k)]));
        for (int64_t tr = 0; tr < M; tr++) {
            const int64_t len = row0[tr + 1] - row0[tr];
            auto st = [&](int sx) { return stats[(size_t)(tr + M * (sx + n_stat * k))]; };
            for (int sx = 0; sx < n_stat; sx++) EXPECT(std::isnan(st(sx)) == (len < 2 || blown));
            if (len < 2 || blown) continue;
            for (int c = 0; c < d; c++) EXPECT(st(3 * c + 1) >= 0.0);
            EXPECT(st(3 * d) >= st(3 * d + 1) && st(3 * d + 1) >= 0.0);
            EXPECT(st(3 * d + 2) >= 0.0 && st(3 * d + 2) <= (double)(len - 1) && st(3 * d + 2) == std::floor(st(3 * d + 2)));
            EXPECT(st(3 * d + 3) == (double)(len - 1));
        }
    }
    // replicate 2 alone, stats alone and obs alone: bitwise the batch's
    TwinSimrows T1 = T;
    T1.coeff = coeff.data() + 2 * n_coef; T1.n_coeff_rows = 1; T1.sigma_obs = with_error ? so.data() + 2 : nullptr; T1.rep0 = 5; T1.n_rep = 1;
    std::vector<double> obs1((size_t)(n * d)), stats1((size_t)(M * n_stat));
    EXPECT(hostsim_simrows_run(T1, obs1.data(), nullptr) == 0);
    EXPECT(hostsim_simrows_run(T1, nullptr, stats1.data()) == 0);
    EXPECT(std::memcmp(obs1.data(), obs.data() + n * d * 2, obs1.size() * sizeof(double)) == 0);
    EXPECT(std::memcmp(stats1.data(), stats.data() + M * n_stat * 2, stats1.size() * sizeof(double)) == 0);
}

}  // namespace

int main() {
    // the series of G meets the written form where they change over, and G(x) -> x^3 / 3
    {
        const double x = 0.25, ome = -std::expm1(-x), ome2 = -std::expm1(-2.0 * x);
        const double below = ssde::simrows_g(std::nextafter(x, 0.0), ome, ome2), at = ssde::simrows_g(x, ome, ome2);
        EXPECT(std::fabs(below - at) <= 1e-13 * at);
        EXPECT(std::fabs(ssde::simrows_g(1e-6, 1e-6, 2e-6) / (1e-18 / 3.0) - 1.0) <= 1e-6);
    }
    for (int kind = 0; kind < 3; kind++)
        for (int d = 1; d <= 3; d++)
            for (int with_error = 0; with_error < 2; with_error++)
                for (int blow_up = 0; blow_up < 2; blow_up++) run_case(kind, d, with_error, blow_up);
    if (fails) { std::fprintf(stderr, "simrows_san: %d checks failed\n", fails); return 1; }
    std::printf("simrows_san ok\n");
    return 0;
}
