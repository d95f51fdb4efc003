// ahead_san.cpp -- TEST INFRASTRUCTURE: the host twin of ssde_forecast_scores (csrc/ssde_ahead.hpp through hostsim_ahead.hpp) as a
// stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (ahead.mk builds it with -fsanitize=address,undefined;
// tests/test_ahead_host.py runs it).  A CTCRW of two response columns and an OU_SSM of one, each with a track of seven rows holding
// an NA row, a track of a single row and a track of two blocks and five rows, horizons (1, 2, 5, 33), with 0 / 3 / 8 thresholds,
// every output alone and all together; it checks what needs no second implementation: horizon 1 is the record's whitened
// innovation, a target fewer than k rows into its track and an NA target are not written, the statistics are the counts and sums
// of the rows written, threshold 0 counts every target and a huge one none, the lead time at horizon 1 is the sum of the intervals
// before the targets, and an output asked for alone is the same numbers.  Exit status 0 and "ahead_san ok" when nothing is wrong.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "hostsim_ahead.hpp"

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { fails++; std::fprintf(stderr, "ahead_san: line %d: %s\n", __LINE__, #c); } } while (0)

template <int MODEL, int D>
void run_case(int n_thr) {
    using namespace ssde;
    typedef DenseDims<MODEL, D> DM;
    typedef SmoothRec<MODEL, D> RC;
    constexpr int SD = DM::SD, Q = DM::Q;
    const int64_t long_rows = 2 * ssde_plan::AHEAD_BLOCK + 5;
    const int64_t n = 8 + long_rows, n_tracks = 3;
    const int64_t row0[] = {0, 7, 8}, nrows[] = {7, 1, long_rows};
    const int n_h = 4;
    const int32_t hz[n_h] = {1, 2, 5, 33};
    std::vector<double> times((size_t)n), obs((size_t)n * D), parmat((size_t)n * Q), a0((size_t)n_tracks * SD, 0.0), p0f((size_t)SD * SD, 0.0);
    for (int64_t i = 0; i < n; i++) {
        times[(size_t)i] = 0.5 * (double)i + 0.01 * (double)(i * i % 5);
        for (int c = 0; c < D; c++) obs[(size_t)(i + c * n)] = std::sin(0.7 * (double)i + c) + 0.3 * (double)i;
        for (int c = 0; c < D; c++) parmat[(size_t)(i * Q + c)] = 0.05;
        for (int c = D; c < Q; c++) parmat[(size_t)(i * Q + c)] = 0.3 - 0.2 * (double)(c - D) + 0.01 * (double)(i % 3);
    }
    const int64_t na_rows[] = {3, 8 + 40};
    for (int64_t r : na_rows)
        for (int c = 0; c < D; c++) obs[(size_t)(r + c * n)] = std::nan("");
    for (int c = 0; c < SD; c++) p0f[(size_t)(c + SD * c)] = (MODEL == M_CTCRW) ? ((c & 1) ? 10.0 : 1.0) : 10.0;
    for (int64_t m = 0; m < n_tracks; m++)
        for (int c = 0; c < D; c++) a0[(size_t)(m * SD + DM::z(c))] = obs[(size_t)(row0[m] + c * n)];
    const TwinProblem pb{1, n, n_tracks, row0, nrows, times.data(), obs.data(), parmat.data(), nullptr, 0.04, p0f.data(), a0.data()};
    const double thr_all[AHEAD_NTHR] = {0.0, 1e300, 0.5, 1.0, 0.25, 2.0, 1e3, 0.75};
    const int n_stat = AHEAD_NSTAT0 + n_thr;
    std::vector<double> z((size_t)n * n_h * D, -1.0), lpd((size_t)n * n_h, -1.0), st((size_t)n_tracks * n_h * n_stat, -1.0);
    std::vector<double> z1(z), lpd1(lpd), st1(st);
    hostsim_ahead_run<MODEL, D>(pb, nullptr, hz, n_h, thr_all, n_thr, z.data(), lpd.data(), st.data());
    hostsim_ahead_run<MODEL, D>(pb, nullptr, hz, n_h, thr_all, n_thr, z1.data(), nullptr, nullptr);
    hostsim_ahead_run<MODEL, D>(pb, nullptr, hz, n_h, thr_all, n_thr, nullptr, lpd1.data(), nullptr);
    hostsim_ahead_run<MODEL, D>(pb, nullptr, hz, n_h, thr_all, n_thr, nullptr, nullptr, st1.data());
    EXPECT(z == z1 && lpd == lpd1 && st == st1);
    std::vector<double> recs;
    for (int64_t m = 0; m < n_tracks; m++) {
        const int64_t ns = twin_record_track<MODEL, D>(pb, m, recs);
        for (int j = 0; j < n_h; j++) {
            const double* t = &st[(size_t)((m * n_h + j) * n_stat)];
            if (ns <= 0) {                                                             // the one-row track: nothing written
                for (int k = 0; k < n_stat; k++) EXPECT(t[k] == -1.0);
                continue;
            }
            double cnt = 0.0, lsum = 0.0, qsum = 0.0, lead1 = 0.0;
            int over[AHEAD_NTHR] = {0};
            for (int64_t i = row0[m]; i < row0[m] + nrows[m]; i++) {
                bool na = false;
                for (int64_t r : na_rows) na = na || r == i;
                const bool want = i - hz[j] >= row0[m] && !na;
                const double l = lpd[(size_t)(i * n_h + j)];
                if (!want) {
                    EXPECT(l == -1.0);
                    for (int c = 0; c < D; c++) EXPECT(z[(size_t)((i * n_h + j) * D + c)] == -1.0);
                    continue;
                }
                double q = 0.0;
                for (int c = 0; c < D; c++) {
                    const double v = z[(size_t)((i * n_h + j) * D + c)];
                    EXPECT(std::isfinite(v));
                    q += v * v;
                    if (hz[j] == 1) {                                                  // the filter's own innovation
                        const double e = recs[(size_t)((i - row0[m] - 1) * RC::R + RC::E + c)];
                        EXPECT(std::fabs(v - e) <= 1e-12 * (1.0 + std::fabs(e)));
                    }
                }
                EXPECT(std::isfinite(l));
                cnt += 1.0; lsum += l; qsum += q;
                lead1 += times[(size_t)i] - times[(size_t)(i - 1)];
                for (int k = 0; k < n_thr; k++) over[k] += q > thr_all[k];
            }
            EXPECT(t[0] == cnt && (cnt > 0.0 || hz[j] >= nrows[m]));
            EXPECT(std::fabs(t[1] - lsum) <= 1e-12 * (1.0 + std::fabs(lsum)));
            EXPECT(std::fabs(t[2] - qsum) <= 1e-12 * (1.0 + qsum));
            EXPECT(t[3] >= 0.0 && (t[4] > 0.0) == (cnt > 0.0));
            if (hz[j] == 1) EXPECT(std::fabs(t[4] - lead1) <= 1e-12 * (1.0 + lead1));
            for (int k = 0; k < n_thr; k++) EXPECT(t[AHEAD_NSTAT0 + k] == (double)over[k]);
            if (n_thr >= 2) { EXPECT(t[AHEAD_NSTAT0] == cnt); EXPECT(t[AHEAD_NSTAT0 + 1] == 0.0); }
        }
    }
}

// a target whose S has no Cholesky factor is not scored: a hand-made chain state with a negative position variance and no noise
void no_factor_case() {
    using namespace ssde;
    typedef AheadSide<M_BM_SSM, 1> AS;
    DenseLane<M_BM_SSM, 1, 0> L;
    const double a0[1] = {0.5}, p0[1] = {-2.0};
    L.init(a0, p0);
    double side[AS::SW] = {0.0};
    side[AS::Y] = 1.0; side[AS::H] = 1e-6; side[AS::DT] = 1.0;
    AheadScore<1> o;
    ahead_score<M_BM_SSM, 1>(L, [&](int k) -> double { return side[k]; }, o);
    EXPECT(!o.scored);
    side[AS::H] = 3.0;                                                               // S = 1: scored, z = y - m
    ahead_score<M_BM_SSM, 1>(L, [&](int k) -> double { return side[k]; }, o);
    EXPECT(o.scored && o.z[0] == 0.5 && o.q == 0.25 && o.e2 == 0.25);
    side[AS::NA] = 1.0;                                                              // ... and not when the row is NA
    ahead_score<M_BM_SSM, 1>(L, [&](int k) -> double { return side[k]; }, o);
    EXPECT(!o.scored);
}

}  // namespace

int main() {
    no_factor_case();
    for (int nt : {0, 3, ssde::AHEAD_NTHR}) { run_case<ssde::M_CTCRW, 2>(nt); run_case<ssde::M_OU_SSM, 1>(nt); }
    if (fails) { std::fprintf(stderr, "ahead_san: %d checks failed\n", fails); return 1; }
    std::printf("ahead_san ok\n");
    return 0;
}
