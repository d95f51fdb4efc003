// lagforms_time.cpp -- what the bulk's forms (csrc/ssde_lagforms.hpp) cost on one host core: a random symmetric M and s, smooth
// decaying taps, the cut given on the command line (default 48, the headline's; the check's cut is 16 taps shorter), d = 2.
// Build with the library's host flags:  hipcc -O3 -std=c++17 --offload-arch=gfx950 -x hip tools/lagforms_time.cpp -o lagforms_time
// Prints, per part, the microseconds per call (best and median of 21 batches of 2000 calls): the tap sums, the raw sums on the
// baseline build and on the wide one, the whole of lag_forms_host; and the largest relative difference of the raw sums from serial
// long-double sums, with whether the two builds agree to the bit.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../smoothsde_amd/csrc/ssde_lagforms.hpp"

namespace {

template <class F>
void time_part(const char* name, F fn) {
    std::vector<double> us;
    for (int b = 0; b < 21; b++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < 2000; i++) fn(i);
        us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / 2000.0);
    }
    std::sort(us.begin(), us.end());
    std::printf("  %-28s best %.3f us, median %.3f us per call\n", name, us.front(), us[us.size() / 2]);
}

}  // namespace

int main(int argc, char** argv) {
    using namespace ssde;
    const int K = argc > 1 ? std::atoi(argv[1]) : 48;
    if (K < LAG_CHECK || K > LAG_KMAX) { std::fprintf(stderr, "K: %d .. %d\n", LAG_CHECK, LAG_KMAX); return 2; }
    std::vector<double> M((size_t)LAG_N * LAG_N), s(2 * LAG_N);
    uint64_t st = 7;
    auto unif = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)(st >> 11) / 9007199254740992.0 - 0.5; };
    for (int i = 0; i < LAG_N; i++)
        for (int k = i; k < LAG_N; k++) M[(size_t)i * LAG_N + k] = M[(size_t)k * LAG_N + i] = (i == k ? 3e6 : 0.0) + 1e6 * unif() / (1 + k - i);
    for (double& v : s) v = 1e3 * unif();
    static LagFormArgs A;
    std::memset(&A, 0, sizeof(A));
    A.M = M.data(); A.s = s.data(); A.n = 1e8; A.K = K; A.Kc = K - LAG_CHECK; A.d = 2; A.mask = 13;
    for (int i = 0; i <= K; i++) { A.lam[i] = std::pow(0.8, i) * (i & 1 ? -1.0 : 1.0); A.rr[i] = 0.5 * std::pow(0.85, i); }
    A.cm[0] = 0.01; A.cm[1] = -0.02;
    for (int i = 0; i < 48; i++) A.statc[i] = 0.1 + 0.01 * i;
    lag_tap_sums(A);
    double raw0[2][LAG_NRAW], raw1[2][LAG_NRAW];
    lag_forms_sums_isa(A, raw0, 0);
    lag_forms_sums_isa(A, raw1, 1);
    const bool same = std::memcmp(raw0, raw1, sizeof(raw0)) == 0;
    // S of both cuts by serial long-double sums
    double worst = 0.0;
    for (int c = 0; c < 2; c++) {
        const int Kc = c ? A.Kc : A.K;
        long double S = 0.0L;
        for (int i = 0; i <= Kc; i++) {
            long double v = 0.0L;
            for (int k = 0; k <= Kc; k++) v += (long double)M[(size_t)i * LAG_N + k] * A.lam[k];
            long double Si = A.lam[i] * v;
            for (int a = 0; a < 2; a++) {
                Si -= 2.0L * A.sum_lam[c] * A.cm[a] * A.lam[i] * s[a * LAG_N + i];
                if (i == 0) Si += (long double)A.n * A.cm[a] * A.cm[a] * A.sum_lam[c] * A.sum_lam[c];
            }
            S += Si;
        }
        worst = std::fmax(worst, (double)(fabsl(S - raw0[c][0]) / fabsl(S)));
    }
    std::printf("bulk forms on the host: K %d, check %d, d 2, wide build %s; S against long double: %.2e relative; baseline and wide %s\n",
                K, A.Kc, lag_forms_wide() ? "present" : "absent", worst, same ? "agree to the bit" : "DIFFER");
    double sink = 0.0;
    LagFormOut o;
    time_part("tap sums", [&](int i) { A.lam[1] = -0.8 + 1e-12 * i; lag_tap_sums(A); sink += A.sum_lam[0]; });
    time_part("raw sums, baseline build", [&](int i) { A.lam[1] = -0.8 + 1e-12 * i; lag_forms_sums_isa(A, raw0, 0); sink += raw0[0][0]; });
    time_part("raw sums, wide build", [&](int i) { A.lam[1] = -0.8 + 1e-12 * i; lag_forms_sums_isa(A, raw1, 1); sink += raw1[0][0]; });
    time_part("tap sums + lag_forms_host", [&](int i) { A.lam[1] = -0.8 + 1e-12 * i; lag_tap_sums(A); lag_forms_host(A, o); sink += o.acc[0]; });
    std::printf("  (sink %.3g)\n", sink);
    return same ? 0 : 1;
}
