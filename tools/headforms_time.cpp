// headforms_time.cpp -- what the head's forms (csrc/ssde_headforms.hpp) cost on one host core: random G and s, the headline's
// theta (sigma_obs 0.1, tau 2, nu 1, unit grid, mu fixed: directions sigma_obs / tau / nu), the cut given on the command line
// (default 64).  Build with the library's host flags:  hipcc -O3 -std=c++17 -x c++ tools/headforms_time.cpp -o headforms_time
// Prints the gain rows, the probe columns and the microseconds per call (best and median of 21 batches of 2000 calls).
// The per-part account: build it again with -DSSDE_HEAD_TIME_NO_DOTS, -DSSDE_HEAD_TIME_NO_PROBES, -DSSDE_HEAD_TIME_NO_MOMENTS (the dot
// products, the probe-column updates, the per-direction moment recursion compiled out) and with all three (the rest); a part's cost
// is the full call's time less the time without it, and the parts overlap where those differences sum to less than the call.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../smoothsde_amd/csrc/ssde_headforms.hpp"

int main(int argc, char** argv) {
    using namespace ssde;
    const int cut = argc > 1 ? std::atoi(argv[1]) : 64, mask = argc > 2 ? std::atoi(argv[2]) : 13;
    if (cut < 1 || cut > HEAD_C) { std::fprintf(stderr, "cut: 1 .. %d\n", HEAD_C); return 2; }
    // G = sum of 10^4 x 2 outer products of a smooth random w would cost as much to build as it matters little: B'B of a small random B
    std::vector<double> G((size_t)HEAD_NW * HEAD_NW, 0.0), s(2 * HEAD_NW, 0.0);
    uint64_t st = 99;
    auto unif = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)(st >> 11) / 9007199254740992.0 - 0.5; };
    for (int k = 0; k < 16; k++) {
        double w[HEAD_NW];
        for (int i = 0; i < HEAD_NW; i++) w[i] = unif();
        for (int p = 0; p < HEAD_NW; p++) {
            for (int q = 0; q < HEAD_NW; q++) G[(size_t)p * HEAD_NW + q] += w[p] * w[q];
            s[(k & 1) * HEAD_NW + p] += w[p];
        }
    }
    CtcrwTrans tr;
    const double tau = 2.0, nu = 1.0, h = 0.01;
    ctcrw_trans(1.0, tau, 1.0 / tau, 2.0 * nu / std::sqrt(M_PI * tau), tr);
    std::vector<double> gain;
    CtcrwCov<15> C;
    C.init(1.0, 0.0, 10.0);
    int last = 0, stable = 0;
    for (int t = 0; t < 4000 && stable < 4; t++) {
        CtcrwGain g;
        const CtcrwCov<15> prev = C;
        ctcrw_cov_step<2, 15>(C, tr, h, false, g);
        double r[HEAD_GROW] = {g.iF, g.k1, g.k2, g.bm};
        for (int j = 0; j < NDIRP; j++) { r[4 + j] = g.diF[j]; r[7 + j] = g.dk1[j]; r[10 + j] = g.dk2[j]; }
        gain.insert(gain.end(), r, r + HEAD_GROW);
        last = t;
        auto close = [](double a, double b) { return std::fabs(a - b) <= 2e-15 * std::fmax(std::fabs(a), std::fabs(b)); };
        bool same = close(C.p11, prev.p11) && close(C.p12, prev.p12) && close(C.p22, prev.p22);
        for (int j = 0; j < NDIRP && same; j++) same = close(C.d11[j], prev.d11[j]) && close(C.d12[j], prev.d12[j]) && close(C.d22[j], prev.d22[j]);
        stable = same ? stable + 1 : 0;
    }
    std::vector<double> Gp((size_t)HEAD_LDW * HEAD_LDW), sp(2 * HEAD_LDW);
    head_pad_stats(G.data(), s.data(), Gp.data(), sp.data());
    HeadFormArgs A;
    A.G = Gp.data(); A.s = sp.data(); A.n = 1e4; A.cut = cut; A.d = 2; A.mask = mask; A.gain = gain.data(); A.gain_last = last;
    A.tr = tr; A.mu[0] = A.mu[1] = 0.0; A.full_probes = false;
    HeadFormWork* W = new HeadFormWork;
    HeadFormOut o;
    if (!head_forms_host(A, *W, o)) { std::fprintf(stderr, "the forms declined\n"); return 1; }
    std::vector<double> us;
    double sink = 0.0;
    for (int b = 0; b < 21; b++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < 2000; i++) { A.mu[0] = 1e-9 * i; head_forms_host(A, *W, o); sink += o.acc[0]; }
        us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / 2000.0);
    }
    std::sort(us.begin(), us.end());
    const char* without =
#if defined(SSDE_HEAD_TIME_NO_DOTS) && defined(SSDE_HEAD_TIME_NO_PROBES) && defined(SSDE_HEAD_TIME_NO_MOMENTS)
        "without dots, probe updates and moments: ";
#elif defined(SSDE_HEAD_TIME_NO_DOTS)
        "without the dots: ";
#elif defined(SSDE_HEAD_TIME_NO_PROBES)
        "without the probe updates: ";
#elif defined(SSDE_HEAD_TIME_NO_MOMENTS)
        "without the moment recursion: ";
#else
        "";
#endif
    std::printf("%s", without);
    std::printf("head forms on the host: cut %d, mask %d, gain rows %d, probe columns %d (+2 offsets): best %.2f us, median %.2f us per call (sink %.3g)\n",
                cut, mask, last + 1, o.n_full, us.front(), us[us.size() / 2], sink);
    delete W;
    return 0;
}
