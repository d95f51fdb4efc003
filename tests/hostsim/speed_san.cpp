// speed_san.cpp -- TEST INFRASTRUCTURE: the host twin of ssde_path_speed (csrc/ssde_speed.hpp through hostsim_speed.hpp) as a
// stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (speed.mk builds it with -fsanitize=address,undefined;
// tests/test_speed_hostsim.py runs it).  Two small CTCRW tracks, one of seven rows with an NA row and one of a single row, for one
// and two response columns, with and without weights, 0 / 3 / 8 thresholds, statistics alone, counts alone and both; it checks what
// needs no second implementation: the one-row track is NaN, the maximum bounds the mean, its row is a state row, +inf counts every
// draw and 0 none, and a draw range cut in two gives the same statistics and counts that add up.  Exit status 0 and "speed_san ok"
// when nothing is wrong.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "hostsim_speed.hpp"

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { fails++; std::fprintf(stderr, "speed_san: line %d: %s\n", __LINE__, #c); } } while (0)

template <int D>
void run_case(bool weights, int n_thr) {
    using namespace ssde;
    constexpr int SD = 2 * D, Q = D + 2;
    const int64_t n = 8, n_tracks = 2, n_draws = 6;
    const int64_t row0[] = {0, 7}, nrows[] = {7, 1};
    std::vector<double> times((size_t)n), obs((size_t)n * D), parmat((size_t)n * Q), a0((size_t)n_tracks * SD, 0.0), p0f((size_t)SD * SD, 0.0);
    for (int64_t i = 0; i < n; i++) {
        times[(size_t)i] = 0.5 * (double)i + 0.01 * (double)(i * i % 5);
        for (int c = 0; c < D; c++) obs[(size_t)(i + c * n)] = std::sin(0.7 * (double)i + c) + 0.3 * (double)i;
        for (int c = 0; c < D; c++) parmat[(size_t)(i * Q + c)] = 0.05;
        parmat[(size_t)(i * Q + D)] = 0.3; parmat[(size_t)(i * Q + D + 1)] = 0.1;
    }
    for (int c = 0; c < D; c++) obs[(size_t)(3 + c * n)] = std::nan("");                 // the NA row
    for (int c = 0; c < SD; c++) p0f[(size_t)(c + SD * c)] = (c & 1) ? 10.0 : 1.0;
    for (int64_t m = 0; m < n_tracks; m++)
        for (int c = 0; c < D; c++) a0[(size_t)(m * SD + 2 * c)] = obs[(size_t)(row0[m] + c * n)];
    const TwinProblem pb{1, n, n_tracks, row0, nrows, times.data(), obs.data(), parmat.data(), nullptr, 0.04, p0f.data(), a0.data()};
    std::vector<double> w((size_t)n);
    for (int64_t i = 0; i < n; i++) w[(size_t)i] = 0.25 + 0.1 * (double)i;
    const double thr_all[SPEED_NTHR] = {0.0, INFINITY, 0.5, 1.0, 0.25, 2.0, 1e3, 0.75};
    const int n_stat = 5 + n_thr;
    std::vector<double> st((size_t)n_draws * n_tracks * n_stat, -1.0), st_only(st), part(st);
    std::vector<uint32_t> cnt((size_t)n * n_thr, 0u), cnt_only(cnt), cnt_part(cnt);
    const double* wp = weights ? w.data() : nullptr;
    hostsim_speed_run<M_CTCRW, D>(pb, 7, 2, (int)n_draws, nullptr, n, wp, thr_all, n_thr, st.data(), n_thr ? cnt.data() : nullptr);
    hostsim_speed_run<M_CTCRW, D>(pb, 7, 2, (int)n_draws, nullptr, n, wp, thr_all, n_thr, st_only.data(), nullptr);
    if (n_thr) hostsim_speed_run<M_CTCRW, D>(pb, 7, 2, (int)n_draws, nullptr, n, wp, thr_all, n_thr, nullptr, cnt_only.data());
    hostsim_speed_run<M_CTCRW, D>(pb, 7, 2, 2, nullptr, n, wp, thr_all, n_thr, part.data(), n_thr ? cnt_part.data() : nullptr);
    hostsim_speed_run<M_CTCRW, D>(pb, 7, 4, 4, nullptr, n, wp, thr_all, n_thr, part.data() + 2 * n_tracks * n_stat, n_thr ? cnt_part.data() : nullptr);
    double wsum = 0.0;
    for (int64_t i = 1; i < 7; i++) wsum += weights ? w[(size_t)i] : 1.0;
    for (int64_t q = 0; q < n_draws; q++) {
        const double* t0 = &st[(size_t)((q * n_tracks + 0) * n_stat)];
        const double* t1 = &st[(size_t)((q * n_tracks + 1) * n_stat)];
        for (int k = 0; k < n_stat; k++) {
            EXPECT(std::isfinite(t0[k]));
            EXPECT(t1[k] == -1.0);                                                        // the one-row track: nothing written
            EXPECT(t0[k] == st_only[(size_t)((q * n_tracks) * n_stat + k)] && t0[k] == part[(size_t)((q * n_tracks) * n_stat + k)]);
        }
        EXPECT(t0[1] >= 0.0 && t0[0] <= t0[1] * wsum * (1.0 + 1e-12));
        EXPECT(t0[2] >= 1.0 && t0[2] <= 6.0 && t0[2] == std::floor(t0[2]));
        EXPECT(std::hypot(t0[3], t0[4]) <= wsum * (1.0 + 1e-12));
        if (D == 1) EXPECT(t0[4] == 0.0);
        if (n_thr >= 2) { EXPECT(t0[5] == 0.0); EXPECT(std::fabs(t0[6] - wsum) <= 1e-12 * wsum); }
    }
    for (int r = 0; r < n_thr; r++)
        for (int64_t i = 0; i < n; i++) {
            const uint32_t c = cnt[(size_t)(i + n * r)];
            EXPECT(c == cnt_only[(size_t)(i + n * r)] && c == cnt_part[(size_t)(i + n * r)] && c <= (uint32_t)n_draws);
            if (i == 0 || i == 7 || r == 0) EXPECT(c == 0u);
            else if (r == 1) EXPECT(c == (uint32_t)n_draws);
        }
}

}  // namespace

int main() {
    for (int wt = 0; wt < 2; wt++)
        for (int nt : {0, 3, ssde::SPEED_NTHR}) { run_case<1>(wt, nt); run_case<2>(wt, nt); }
    if (fails) { std::fprintf(stderr, "speed_san: %d checks failed\n", fails); return 1; }
    std::printf("speed_san ok\n");
    return 0;
}
