// bands_san.cpp -- TEST INFRASTRUCTURE: the host twin of ssde_par_bands (csrc/ssde_bands.hpp through hostsim_bands.hpp) as a
// stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (bands.mk builds it with -fsanitize=address,undefined;
// tests/test_bands_hostsim.py runs it).  Small problems -- three parameters (an intercept alone, three columns, four fixed and five
// random columns), seven rows -- at tails of 2 (n_post = 2 and 7) and of exactly 64 (n_post = 2500 at level 0.95), with the draws'
// rows duplicated (ties) and with a NaN in one design row.  It checks what needs no second implementation: a tail buffer is sorted
// after every insert and never holds more than m values, every buffer fills, the pointwise band is ordered and the simultaneous one
// is ordered by the sign of se, a log link's outputs are positive, the NaN row is NaN in every output and no other row is, and crit
// with the NaN row is bitwise crit of the problem without that row.  Exit status 0 and "bands_san ok" when nothing is wrong.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "hostsim_bands.hpp"

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { fails++; std::fprintf(stderr, "bands_san: line %d: %s\n", __LINE__, #c); } } while (0)

double unit(uint64_t& s) {                                  // a small generator of its own: (-1, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((s >> 11) & 0xFFFFFFFFFFFFull) / (double)0x1000000000000ull * 2.0 - 1.0;
}

void run_case(int n_post, double level, bool ties, bool nan_row, int resp) {
    using namespace ssde;
    const int64_t n = 7;
    const int q = 3;
    const int32_t kf[q] = {1, 3, 4}, kr[q] = {0, 0, 5};
    const uint8_t link[q] = {0, 1, 1};
    const int n_coef = 1 + 3 + 9;
    uint64_t s = 12345u + (uint64_t)n_post;
    std::vector<double> xf1((size_t)n * 3), xf2((size_t)n * 4), xr2((size_t)n * 5), coeff((size_t)(1 + n_post) * n_coef);
    for (auto* v : {&xf1, &xf2, &xr2})
        for (double& e : *v) e = unit(s);
    for (int64_t i = 0; i < n; i++) { xf1[(size_t)i] = 1.0; xf2[(size_t)i] = 1.0; }
    if (nan_row) xf1[(size_t)(4 + n * 1)] = std::nan("");
    for (int c = 0; c < n_coef; c++) coeff[(size_t)c] = 1.0 + 0.5 * unit(s);
    for (int k = 1; k <= n_post; k++)
        for (int c = 0; c < n_coef; c++) {
            const int src = ties ? (k + 1) / 2 * 2 : k;                             // draws 1, 2 alike, 3, 4 alike, ...
            uint64_t t = 99u + (uint64_t)src * 131u + (uint64_t)c;
            coeff[(size_t)k * n_coef + c] = coeff[(size_t)c] + 0.3 * unit(t);
        }
    const double* xfp[q] = {nullptr, xf1.data(), xf2.data()};
    const double* xrp[q] = {nullptr, nullptr, xr2.data()};
    const TwinBands T{n, q, kf, xfp, kr, xrp, link, coeff.data(), n_post, resp, level, 1.959963984540054};
    const BandsPlan P = bands_plan(n_post, level);
    std::vector<double> est((size_t)n * q), lo(est), up(est), se(est), sl(est), su(est), crit((size_t)q), md((size_t)q * n_post);
    long inserts = 0;
    const int st = hostsim_bands_run(T, est.data(), lo.data(), up.data(), se.data(), sl.data(), su.data(), crit.data(), md.data(),
                                     [&](auto&& buf, int cnt) {
                                         inserts++;
                                         EXPECT(cnt >= 1 && cnt <= P.m);
                                         for (int r = 1; r < cnt; r++) EXPECT(buf(r - 1) <= buf(r));
                                     });
    EXPECT(st == 0);
    EXPECT(inserts >= 2L * P.m * (n * q - (nan_row ? 1 : 0)));        // every buffer fills; the NaN row inserts nothing
    for (int j = 0; j < q; j++) {
        EXPECT(crit[(size_t)j] >= 0.0 && std::isfinite(crit[(size_t)j]));
        for (int k = 0; k < n_post; k++) EXPECT(md[(size_t)j * n_post + k] >= 0.0);
        for (int64_t i = 0; i < n; i++) {
            const size_t e = (size_t)(i + n * j);
            if (nan_row && j == 1 && i == 4) {
                EXPECT(std::isnan(est[e]) && std::isnan(lo[e]) && std::isnan(up[e]) && std::isnan(se[e]) && std::isnan(sl[e]) && std::isnan(su[e]));
                continue;
            }
            EXPECT(std::isfinite(est[e]) && std::isfinite(se[e]));
            EXPECT(lo[e] <= up[e]);
            EXPECT(se[e] >= 0.0 ? sl[e] <= su[e] : sl[e] >= su[e]);
            if (resp && link[j]) EXPECT(est[e] > 0.0 && lo[e] > 0.0 && sl[e] > 0.0);
        }
    }
    if (nan_row) {                                                                   // the NaN row adds nothing: crit without the row is crit with it
        std::vector<double> crit2((size_t)q);
        std::vector<double> xf1b((size_t)(n - 1) * 3), xf2b((size_t)(n - 1) * 4), xr2b((size_t)(n - 1) * 5);
        auto drop = [&](const std::vector<double>& a, std::vector<double>& b, int cols) {
            for (int c = 0; c < cols; c++)
                for (int64_t i = 0, w = 0; i < n; i++)
                    if (i != 4) b[(size_t)(w++ + (n - 1) * c)] = a[(size_t)(i + n * c)];
        };
        drop(xf1, xf1b, 3); drop(xf2, xf2b, 4); drop(xr2, xr2b, 5);
        const double* xfq[q] = {nullptr, xf1b.data(), xf2b.data()};
        const double* xrq[q] = {nullptr, nullptr, xr2b.data()};
        const TwinBands T2{n - 1, q, kf, xfq, kr, xrq, link, coeff.data(), n_post, resp, level, T.z};
        EXPECT(hostsim_bands_run(T2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, crit2.data(), nullptr, [](auto&&, int) {}) == 0);
        EXPECT(crit2[1] == crit[1]);
    }
}

}  // namespace

int main() {
    EXPECT(ssde::bands_plan(2, 0.95).m == 2 && ssde::bands_plan(7, 0.95).m == 2);
    EXPECT(ssde::bands_plan(2500, 0.95).m_lo == 64 && ssde::bands_plan(2500, 0.95).m_up == 64);
    EXPECT(ssde::bands_plan(1000, 0.90).m_lo == 51 && ssde::bands_plan(1000, 0.5).m_lo == 251);
    for (int resp = 0; resp < 2; resp++)
        for (int n_post : {2, 7, 2500})
            for (int ties = 0; ties < 2; ties++)
                for (int nan_row = 0; nan_row < 2; nan_row++) run_case(n_post, 0.95, ties, nan_row, resp);
    if (fails) { std::fprintf(stderr, "bands_san: %d checks failed\n", fails); return 1; }
    std::printf("bands_san ok\n");
    return 0;
}
