// headforms_san.cpp -- TEST INFRASTRUCTURE: the head of the lag-statistics path from Gram statistics (csrc/ssde_headforms.hpp) as a
// stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (headforms.mk builds it with
// -fsanitize=address,undefined; tests/test_headforms_host.py runs it).  A batch of seven tracks of 128 rows and two coordinates: the
// statistics track by track, the gain table by the covariance half of the filter until it has settled, then for cuts 1, 2, 17, 32, 64
// and 128, four direction masks and mu zero / non-zero the forms against the lanes' own step (ctcrw_mean_step) run row by row per
// track, and the shifted-column shortcut against the run with every column a probe.  Exit status 0 and "headforms_san ok" when
// nothing is wrong.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../smoothsde_amd/csrc/ssde_headforms.hpp"

namespace {

int fails = 0;
#define EXPECT(c) do { if (!(c)) { fails++; std::fprintf(stderr, "headforms_san: line %d: %s\n", __LINE__, #c); } } while (0)

double unif(uint64_t& st) {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(st >> 11) / 9007199254740992.0 - 0.5;
}

}  // namespace

int main() {
    using namespace ssde;
    const int d = 2, n_tracks = 7, rows = HEAD_C;
    uint64_t st = 12345;
    std::vector<double> y((size_t)n_tracks * rows * d), a0((size_t)n_tracks * 2 * d);
    for (int k = 0; k < n_tracks; k++) {
        double pos[2] = {10.0 * unif(st), 10.0 * unif(st)}, vel[2] = {unif(st), unif(st)};
        for (int a = 0; a < d; a++) { a0[(size_t)k * 4 + 2 * a] = pos[a] + 0.1 * unif(st); a0[(size_t)k * 4 + 2 * a + 1] = 0.3 * unif(st); }
        for (int t = 0; t < rows; t++)
            for (int a = 0; a < d; a++) {
                vel[a] = 0.6 * vel[a] + unif(st);
                pos[a] += vel[a];
                y[((size_t)k * rows + t) * d + a] = pos[a] + 0.2 * unif(st);
            }
    }
    std::vector<double> G((size_t)HEAD_NW * HEAD_NW, 0.0), s(2 * HEAD_NW, 0.0);
    for (int k = 0; k < n_tracks; k++) head_track_stats(y.data() + (size_t)k * rows * d, a0.data() + (size_t)k * 4, d, G.data(), s.data());
    for (int p = 0; p < HEAD_NW; p++)
        for (int q = 0; q < p; q++) EXPECT(G[(size_t)p * HEAD_NW + q] == G[(size_t)q * HEAD_NW + p]);
    std::vector<double> Gp((size_t)HEAD_LDW * HEAD_LDW), sp(2 * HEAD_LDW);
    head_pad_stats(G.data(), s.data(), Gp.data(), sp.data());
    // theta: sigma_obs 0.2, tau 2, nu 1 on a unit grid; the gain table until the covariance has stopped moving (at most 40 rows here)
    CtcrwTrans tr;
    const double tau = 2.0, nu = 1.0, h = 0.04;
    ctcrw_trans(1.0, tau, 1.0 / tau, 2.0 * nu / std::sqrt(M_PI * tau), tr);
    std::vector<double> gain;
    CtcrwCov<15> C;
    C.init(1.0, 0.0, 10.0);
    int last = 0;
    for (int t = 0; t < 40; t++) {
        CtcrwGain g;
        const double p_before = C.p11;
        ctcrw_cov_step<2, 15>(C, tr, h, false, g);
        double r[HEAD_GROW] = {g.iF, g.k1, g.k2, g.bm};
        for (int j = 0; j < NDIRP; j++) { r[4 + j] = g.diF[j]; r[7 + j] = g.dk1[j]; r[10 + j] = g.dk2[j]; }
        gain.insert(gain.end(), r, r + HEAD_GROW);
        last = t;
        if (t > 8 && std::fabs(C.p11 - p_before) <= 1e-15 * std::fabs(C.p11)) break;
    }
    EXPECT(last >= 4 && last < 39);
    HeadFormWork* W = new HeadFormWork;
    const int cuts[] = {1, 2, 17, 32, 64, 128}, masks[] = {15, 13, 1, 0};
    double worst = 0.0, worst_shift = 0.0;
    for (int cut : cuts)
        for (int mask : masks)
            for (int with_mu = 0; with_mu < 2; with_mu++) {
                const double mu[2] = {with_mu ? 0.3 : 0.0, with_mu ? -0.2 : 0.0};
                HeadFormArgs A;
                A.G = Gp.data(); A.s = sp.data(); A.n = n_tracks; A.cut = cut; A.d = d; A.mask = mask; A.gain = gain.data(); A.gain_last = last;
                A.tr = tr; A.mu[0] = mu[0]; A.mu[1] = mu[1]; A.full_probes = false;
                HeadFormOut o, of;
                EXPECT(head_forms_host(A, *W, o));
                A.full_probes = true;
                EXPECT(head_forms_host(A, *W, of));
                EXPECT(of.n_full == cut + 1 && o.n_full <= of.n_full);
                // the lanes' own step, track by track
                double ref[6] = {0, 0, 0, 0, 0, 0};
                for (int k = 0; k < n_tracks; k++) {
                    CtcrwMean<2, 15> M;
                    M.init(a0.data() + (size_t)k * 4);
                    for (int t = 0; t < cut; t++) {
                        const double* r = gain.data() + (size_t)(t < last ? t : last) * HEAD_GROW;
                        CtcrwGain g;
                        g.iF = r[0]; g.k1 = r[1]; g.k2 = r[2]; g.bm = r[3];
                        for (int j = 0; j < NDIRP; j++) { g.diF[j] = r[4 + j]; g.dk1[j] = r[7 + j]; g.dk2[j] = r[10 + j]; }
                        ctcrw_mean_step<2, 15>(M, tr, g, mu, y.data() + ((size_t)k * rows + t) * d, true);
                    }
                    const double z[NDIRP] = {0.0, 0.0, 0.0};
                    double out[6];
                    ctcrw_finish_parts<2, 15>(0.0, z, M, out);
                    for (int i = 0; i < 6; i++) ref[i] += out[i];
                }
                if (!(mask & DIR_SIG)) ref[1] = 0.0;
                if (!(mask & DIR_MU)) ref[2] = ref[3] = 0.0;
                if (!(mask & DIR_P1)) ref[4] = 0.0;
                if (!(mask & DIR_P2)) ref[5] = 0.0;
                for (int i = 0; i < 6; i++) {
                    const double sc = std::fmax(std::fabs(ref[i]), 1.0);
                    const double e = std::fabs(o.acc[i] - ref[i]) / sc, es = std::fabs(o.acc[i] - of.acc[i]) / sc;
                    worst = std::fmax(worst, e); worst_shift = std::fmax(worst_shift, es);
                    EXPECT(e <= 1e-10);
                    EXPECT(es <= 1e-12);
                    EXPECT((mask & (i == 0 ? 0xff : i == 1 ? DIR_SIG : i < 4 ? DIR_MU : i == 4 ? DIR_P1 : DIR_P2)) || o.acc[i] == 0.0 || i == 0);
                }
            }
    // a row that is not scored keeps the kernel
    {
        std::vector<double> g2(gain);
        g2[3 * HEAD_GROW] = 0.0;
        HeadFormArgs A;
        A.G = Gp.data(); A.s = sp.data(); A.n = n_tracks; A.cut = 64; A.d = d; A.mask = 15; A.gain = g2.data(); A.gain_last = last;
        A.tr = tr; A.mu[0] = A.mu[1] = 0.0; A.full_probes = false;
        HeadFormOut o;
        EXPECT(!head_forms_host(A, *W, o));
        A.gain = gain.data(); A.cut = HEAD_C + 1;
        EXPECT(!head_forms_host(A, *W, o));
    }
    delete W;
    std::printf("headforms_san: against the lanes' step %.3e, shortcut against full probes %.3e (gain rows %d)\n", worst, worst_shift, last + 1);
    if (fails) return 1;
    std::printf("headforms_san ok\n");
    return 0;
}
