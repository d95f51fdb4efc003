// tests/gainfeed/gainfeed_host.cpp -- host test program of smoothsde_amd/csrc/ssde_gain_feed.hpp (tests/test_gain_feed_host.py builds
// and runs it with g++):
//   check            the packing of a gain table into the by-value form and the LDS slab it expands to, against stage_gain's rule written
//                    out here from its definition (k_iso_shared.inc: slab row rr of a slab that starts at table row row0 is table row
//                    min(row0 + rr, last), 16 doubles a row) -- rows = 1, a few, the capacity; the CTCRW and the scalar column sets; the
//                    slabs at row0 = 0 and 64; and what must be refused (no rows, one row too many, a column the packing drops).
//   rows d dt log_tau log_nu n lo hi p11 p12 p22
//                    the rows of the CTCRW gain table (P0 = blocks [p11 p12; p12 p22]) at n values of log sigma_obs from lo to hi, one per line:
//                    tests/test_gpu_head_feed.py chooses its parameters by them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../smoothsde_amd/csrc/ssde_gain_feed.hpp"

using namespace ssde;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

constexpr int SLAB_ROWS = 64;

// a table of `rows` rows as build_gain_table writes them: scal = the scalar family's columns (0-2, 4-9), else CTCRW's (0-12)
static std::vector<double> make_table(int rows, bool scal) {
    std::vector<double> t((size_t)rows * HEAD_GAIN_STRIDE, 0.0);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < HEAD_GAIN_STRIDE; c++) {
            const bool used = scal ? (c <= 2 || (c >= 4 && c <= 9)) : c < HEAD_GAIN_COLS;
            if (used) t[(size_t)r * HEAD_GAIN_STRIDE + c] = 1.0 + r * 0.37 + c * 1e-3 + (scal ? 100.0 : 0.0);
        }
    return t;
}

static void check_case(int rows, int capacity, bool scal) {
    const std::vector<double> t = make_table(rows, scal);
    std::vector<double> v((size_t)capacity * HEAD_GAIN_COLS, -7.0);
    EXPECT(head_gain_pack(t.data(), rows, capacity, v.data()));
    for (size_t i = (size_t)rows * HEAD_GAIN_COLS; i < v.size(); i++) EXPECT(v[i] == -7.0);      // nothing past the rows is written
    for (int row0 = 0; row0 <= SLAB_ROWS; row0 += SLAB_ROWS)
        for (int rr = 0; rr < SLAB_ROWS; rr++)
            for (int c = 0; c < HEAD_GAIN_STRIDE; c++) {
                const int src = row0 + rr < rows - 1 ? row0 + rr : rows - 1;                   // stage_gain: min(row0 + rr, gain_last)
                const double want = t[(size_t)src * HEAD_GAIN_STRIDE + c];
                const double got = head_gain_slab_at(v.data(), rows, row0 + rr, c);
                if (memcmp(&want, &got, 8) != 0) { printf("rows %d scal %d row0 %d rr %d c %d: %.17g != %.17g\n", rows, (int)scal, row0, rr, c, got, want); fails++; }
                EXPECT(head_gain_index(rows, row0 + rr, c < HEAD_GAIN_COLS ? c : HEAD_GAIN_COLS - 1) < rows * HEAD_GAIN_COLS);
            }
}

static int check() {
    static_assert(head_gain_capacity(2296) == 17, "4096 - sizeof(IsoArgs) - 8 bytes hold 17 rows of 13 doubles");
    static_assert(sizeof(HeadGainT<17>) == 8 + 17 * 13 * 8, "row count, then the packed rows");
    static_assert(head_gain_capacity(4096 - 8 - 104) == 1 && head_gain_capacity(4096 - 8 - 103) == 0, "whole rows only");
    for (int capacity : {16, 17})
        for (int scal = 0; scal < 2; scal++)
            for (int rows : {1, 2, 5, capacity - 1, capacity}) check_case(rows, capacity, scal != 0);
    // refused: no rows, one row too many, a column past the packed ones that is not zero
    std::vector<double> t = make_table(18, false), v(18 * HEAD_GAIN_COLS, -7.0);
    EXPECT(!head_gain_pack(t.data(), 0, 17, v.data()));
    EXPECT(!head_gain_pack(t.data(), 18, 17, v.data()));
    t[3 * HEAD_GAIN_STRIDE + 14] = 1e-300;
    EXPECT(!head_gain_pack(t.data(), 5, 17, v.data()));
    EXPECT(head_gain_pack(t.data(), 3, 17, v.data()));
    for (size_t i = 3 * HEAD_GAIN_COLS; i < v.size(); i++) EXPECT(v[i] == -7.0);
    printf(fails ? "gainfeed: %d failures\n" : "gainfeed: ok\n", fails);
    return fails ? 1 : 0;
}

static int rows_cmd(int argc, char** argv) {
    if (argc != 12) return 2;
    const int d = atoi(argv[2]), n = atoi(argv[6]);
    const double dt = atof(argv[3]), tau = exp(atof(argv[4])), nu = exp(atof(argv[5])), lo = atof(argv[7]), hi = atof(argv[8]);
    CtcrwTrans tr;
    ctcrw_trans(dt, tau, 1.0 / tau, 2.0 * nu / sqrt(M_PI * tau), tr);
    const double p0[3] = {atof(argv[9]), atof(argv[10]), atof(argv[11])};
    for (int i = 0; i < n; i++) {
        const double ls = n > 1 ? lo + (hi - lo) * i / (n - 1) : lo, sig = exp(ls);
        printf("%.17g %d\n", ls, d == 1 ? ctcrw_gain_rows<1>(tr, sig * sig, p0, 100000) : ctcrw_gain_rows<2>(tr, sig * sig, p0, 100000));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "check")) return check();
    if (argc >= 2 && !strcmp(argv[1], "rows")) return rows_cmd(argc, argv);
    printf("usage: %s check | rows d dt log_tau log_nu n lo hi p11 p12 p22\n", argv[0]);
    return 2;
}
