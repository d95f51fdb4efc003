// loo_san.cpp -- TEST INFRASTRUCTURE: the host twin of ssde_smooth_loo (csrc/ssde_loo.hpp through hostsim_loo.hpp) as a stand-alone
// program under AddressSanitizer and UndefinedBehaviorSanitizer (loo.mk builds it with -fsanitize=address,undefined;
// tests/test_loo_hostsim.py runs it).  Two small cases -- a CTCRW of two response columns and an OU_SSM of three, each with a track
// of seven rows holding an NA row and a track of a single row -- with 0 / 3 / 8 thresholds, every output alone and all together; it
// checks what needs no second implementation: rows without a fix to leave out are not written, the covariance is symmetric with a
// positive diagonal, lpd is the Gaussian log density of the residual it is returned with (the log determinant formed by
// elimination here), the statistics are the sums, the maximum and the counts of the rows written, threshold 0 counts every row
// and a huge one none, and an output asked for alone is the same numbers.  Exit status 0 and "loo_san ok" when nothing is wrong.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "hostsim_loo.hpp"

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { fails++; std::fprintf(stderr, "loo_san: line %d: %s\n", __LINE__, #c); } } while (0)

template <int MODEL, int D>
void run_case(int n_thr) {
    using namespace ssde;
    typedef DenseDims<MODEL, D> DM;
    constexpr int SD = DM::SD, Q = DM::Q;
    const int64_t n = 8, n_tracks = 2;
    const int64_t row0[] = {0, 7}, nrows[] = {7, 1};
    std::vector<double> times((size_t)n), obs((size_t)n * D), parmat((size_t)n * Q), a0((size_t)n_tracks * SD, 0.0), p0f((size_t)SD * SD, 0.0);
    for (int64_t i = 0; i < n; i++) {
        times[(size_t)i] = 0.5 * (double)i + 0.01 * (double)(i * i % 5);
        for (int c = 0; c < D; c++) obs[(size_t)(i + c * n)] = std::sin(0.7 * (double)i + c) + 0.3 * (double)i;
        for (int c = 0; c < D; c++) parmat[(size_t)(i * Q + c)] = 0.05;
        for (int c = D; c < Q; c++) parmat[(size_t)(i * Q + c)] = 0.3 - 0.2 * (double)(c - D);
    }
    for (int c = 0; c < D; c++) obs[(size_t)(3 + c * n)] = std::nan("");                 // the NA row
    for (int c = 0; c < SD; c++) p0f[(size_t)(c + SD * c)] = (MODEL == M_CTCRW) ? ((c & 1) ? 10.0 : 1.0) : 10.0;
    for (int64_t m = 0; m < n_tracks; m++)
        for (int c = 0; c < D; c++) a0[(size_t)(m * SD + DM::z(c))] = obs[(size_t)(row0[m] + c * n)];
    const TwinProblem pb{1, n, n_tracks, row0, nrows, times.data(), obs.data(), parmat.data(), nullptr, 0.04, p0f.data(), a0.data()};
    const double thr_all[LOO_NTHR] = {0.0, 1e300, 0.5, 1.0, 0.25, 2.0, 1e3, 0.75};
    const int n_stat = 4 + n_thr;
    std::vector<double> mean((size_t)n * D, -1.0), cov((size_t)n * D * D, -1.0), res((size_t)n * D, -1.0), lpd((size_t)n, -1.0),
        st((size_t)n_tracks * n_stat, -1.0);
    std::vector<double> mean1(mean), cov1(cov), res1(res), lpd1(lpd), st1(st);
    hostsim_loo_run<MODEL, D>(pb, nullptr, thr_all, n_thr, mean.data(), cov.data(), res.data(), lpd.data(), st.data());
    hostsim_loo_run<MODEL, D>(pb, nullptr, thr_all, n_thr, mean1.data(), nullptr, nullptr, nullptr, nullptr);
    hostsim_loo_run<MODEL, D>(pb, nullptr, thr_all, n_thr, nullptr, cov1.data(), nullptr, nullptr, nullptr);
    hostsim_loo_run<MODEL, D>(pb, nullptr, thr_all, n_thr, nullptr, nullptr, res1.data(), nullptr, nullptr);
    hostsim_loo_run<MODEL, D>(pb, nullptr, thr_all, n_thr, nullptr, nullptr, nullptr, lpd1.data(), nullptr);
    hostsim_loo_run<MODEL, D>(pb, nullptr, thr_all, n_thr, nullptr, nullptr, nullptr, nullptr, st1.data());
    EXPECT(mean == mean1 && cov == cov1 && res == res1 && lpd == lpd1 && st == st1);
    double lsum = 0.0, qmax = -1.0, qrow = -1.0;
    int rows = 0, over[LOO_NTHR] = {0};
    for (int64_t i = n - 1; i >= 0; i--) {
        const bool fix = i >= 1 && i <= 6 && i != 3;
        if (!fix) {
            EXPECT(lpd[(size_t)i] == -1.0);
            for (int a = 0; a < D; a++) EXPECT(mean[(size_t)(i * D + a)] == -1.0 && res[(size_t)(i * D + a)] == -1.0);
            for (int a = 0; a < D * D; a++) EXPECT(cov[(size_t)(i * D * D + a)] == -1.0);
            continue;
        }
        // log det by elimination without pivoting (positive definite), q from the residual
        double A[D][D], ld = 0.0, q = 0.0;
        for (int a = 0; a < D; a++)
            for (int b = 0; b < D; b++) {
                A[a][b] = cov[(size_t)((i * D + a) * D + b)];
                EXPECT(A[a][b] == cov[(size_t)((i * D + b) * D + a)]);
            }
        for (int a = 0; a < D; a++) {
            EXPECT(A[a][a] > 0.0);
            ld += std::log(A[a][a]);
            for (int b = a + 1; b < D; b++) {
                const double f = A[b][a] / A[a][a];
                for (int c = a; c < D; c++) A[b][c] -= f * A[a][c];
            }
        }
        for (int a = 0; a < D; a++) {
            EXPECT(std::isfinite(mean[(size_t)(i * D + a)]) && std::isfinite(res[(size_t)(i * D + a)]));
            q += res[(size_t)(i * D + a)] * res[(size_t)(i * D + a)];
        }
        const double want = -0.5 * (D * std::log(2.0 * M_PI) + ld + q);
        EXPECT(std::fabs(lpd[(size_t)i] - want) <= 1e-10 * (1.0 + std::fabs(want)));
        lsum += lpd[(size_t)i];
        if (rows == 0 || q >= qmax) { qmax = q; qrow = (double)i; }
        rows++;
        for (int k = 0; k < n_thr; k++) over[k] += q > thr_all[k];
    }
    const double* t0 = &st[0];
    const double* t1 = &st[(size_t)n_stat];
    for (int k = 0; k < n_stat; k++) EXPECT(t1[k] == -1.0);                               // the one-row track: nothing written
    EXPECT(t0[0] == 5.0 && rows == 5);
    EXPECT(t0[1] == lsum);                                                              // the same sum in the same order
    EXPECT(std::fabs(t0[2] - qmax) <= 1e-12 * (1.0 + qmax) && t0[3] == qrow);
    for (int k = 0; k < n_thr; k++) EXPECT(t0[4 + k] == (double)over[k]);
    if (n_thr >= 2) { EXPECT(t0[4] == 5.0); EXPECT(t0[5] == 0.0); }
}

// Where only the second factor fails: a hand-made record of a track's last row (d = 1) whose F^-1 is a positive subnormal, so
// M = F^-1 > 0 has its factor and D = 1 / M overflows.  The row is served (mean and covariance are formed), it is not white.
void second_factor_case() {
    using namespace ssde;
    typedef SmoothRec<M_BM_SSM, 1> RC;
    double rec[RC::R] = {0.0};
    rec[RC::A] = 1.5; rec[RC::V] = 0.25; rec[RC::FI] = 4e-320; rec[RC::E] = 0.1; rec[RC::T + 1] = 1.0;
    double r[1] = {0.0}, N[1][1] = {{0.0}};
    LooRow<1> o;
    loo_back_row<M_BM_SSM, 1, 1>(r, N, true, [&](int k) -> double { return rec[k]; }, o);
    EXPECT(o.served && !o.white);
    EXPECT(std::isinf(o.cov[0][0]) && o.cov[0][0] > 0.0);
    EXPECT(N[0][0] == 4e-320 && r[0] == 0.25 * 4e-320);
    rec[RC::FI] = 0.0;                                                                  // a row without an update: not served
    rec[RC::V] = 0.0; rec[RC::E] = std::nan("");
    loo_back_row<M_BM_SSM, 1, 1>(r, N, true, [&](int k) -> double { return rec[k]; }, o);
    EXPECT(!o.served && !o.white);
    rec[RC::FI] = 2.0; rec[RC::V] = 0.5;                                                // an update whose residual is NaN (F < 0 upstream)
    loo_back_row<M_BM_SSM, 1, 1>(r, N, true, [&](int k) -> double { return rec[k]; }, o);
    EXPECT(!o.served);
    rec[RC::E] = 0.5 * std::sqrt(2.0);                                                  // ... and the same row with one: served, white
    loo_back_row<M_BM_SSM, 1, 1>(r, N, true, [&](int k) -> double { return rec[k]; }, o);
    EXPECT(o.served && o.white && o.cov[0][0] == 0.5 && o.mean[0] == 1.5 && std::fabs(o.z[0] - rec[RC::E]) <= 1e-15);
}

}  // namespace

int main() {
    second_factor_case();
    for (int nt : {0, 3, ssde::LOO_NTHR}) { run_case<ssde::M_CTCRW, 2>(nt); run_case<ssde::M_OU_SSM, 3>(nt); }
    if (fails) { std::fprintf(stderr, "loo_san: %d checks failed\n", fails); return 1; }
    std::printf("loo_san ok\n");
    return 0;
}
