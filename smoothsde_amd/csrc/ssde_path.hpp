// ssde_path.hpp -- summaries of posterior state paths (ssde_path_stats): the per-(lane, draw) math, DESIGN.md §3.12.
//
// The backward walk of ssde_draws.hpp forms draw q's state at one row after the other, from the track's last row to its first;
// path_step folds the row's POSITION (state column 2a of a CTCRW, a otherwise) into a PathAcc -- the path length so far, the
// positions at the two ends, the weighted rows inside every region and a not-finite flag -- and path_finish turns the accumulator
// into the n_stat = 2 + n_regions numbers of the call.  Only rows of the caller's data take part: a lattice-padded handle samples
// its padded rows (the recursion needs them) and hands them in with is_row = false.  Host- and device-compilable, like
// ssde_draws.hpp; every loop has a constant trip count, so the accumulators stay in registers.
#ifndef SSDE_PATH_HPP
#define SSDE_PATH_HPP

#include <math.h>

#include "ssde_draws.hpp"

#ifndef SSDE_PATH_MAX_REGIONS
#define SSDE_PATH_MAX_REGIONS 8
#endif

#if defined(__clang__)
#define SSDE_PLOOP _Pragma("unroll")
#else
#define SSDE_PLOOP
#endif

namespace ssde {

constexpr int PATH_NREG = SSDE_PATH_MAX_REGIONS;
constexpr int PATH_NSTAT_MAX = 2 + PATH_NREG;

// one (lane, draw): `held` is the position at the caller's row seen last (the EARLIEST so far: the walk runs backwards), `end` the
// position at the first one seen (the track's last state row)
template <int D>
struct PathAcc {
    double len, held[D], end[D], reg[PATH_NREG];
    int rows, bad;
};

template <int D>
SSDE_HD void path_init(PathAcc<D>& a) {
    a.len = 0.0; a.rows = 0; a.bad = 0;
    SSDE_PLOOP for (int c = 0; c < D; c++) { a.held[c] = 0.0; a.end[c] = 0.0; }
    SSDE_PLOOP for (int r = 0; r < PATH_NREG; r++) a.reg[r] = 0.0;
}

template <int D>
SSDE_HD double path_dist(const double (&p)[D], const double (&q)[D]) {
    if (D == 1) return fabs(p[0] - q[0]);
    double s = 0.0;
    SSDE_PLOOP for (int c = 0; c < D; c++) s += (p[c] - q[c]) * (p[c] - q[c]);
    return sqrt(s);
}

// The state just drawn at one row: alpha; is_row: the row is a row of the caller's data; w: its weight; regions: n_regions rows of
// lo_1, hi_1, lo_2, hi_2 (the second pair is not read for D = 1), region(k) double k of that table.  A weight is added only where the
// row is inside, so a non-finite weight enters the sums it is added to and no other.
template <int MODEL, int D, int SD, class G>
SSDE_HD void path_step(PathAcc<D>& a, const double (&alpha)[SD], bool is_row, double w, G&& region, int n_regions) {
    typedef DenseDims<MODEL, D> DM;
    if (!is_row) return;
    double p[D];
    SSDE_PLOOP for (int c = 0; c < D; c++) {
        p[c] = alpha[DM::z(c)];
        if (!(fabs(p[c]) <= 1.7976931348623157e308)) a.bad = 1;     // NaN or +-inf
    }
    if (a.rows == 0) {
        SSDE_PLOOP for (int c = 0; c < D; c++) a.end[c] = p[c];
    } else {
        a.len += path_dist<D>(p, a.held);
    }
    SSDE_PLOOP for (int c = 0; c < D; c++) a.held[c] = p[c];
    a.rows++;
    SSDE_PLOOP for (int r = 0; r < PATH_NREG; r++) {
        if (r < n_regions) {
            bool in = true;
            SSDE_PLOOP for (int c = 0; c < D; c++) in = in && region(4 * r + 2 * c) <= p[c] && p[c] < region(4 * r + 2 * c + 1);
            if (in) a.reg[r] += w;
        }
    }
}

// out[0 .. 2 + n_regions): length, net displacement, the region sums; every one NaN where a position was not finite (or no row of
// the caller's was seen).  Elements past 2 + n_regions are set to 0 and mean nothing.
template <int D>
SSDE_HD void path_finish(const PathAcc<D>& a, int n_regions, double (&out)[PATH_NSTAT_MAX]) {
    const bool nan = a.bad || a.rows == 0;
    const double qn = __builtin_nan("");
    out[0] = nan ? qn : a.len;
    out[1] = nan ? qn : path_dist<D>(a.end, a.held);
    SSDE_PLOOP for (int r = 0; r < PATH_NREG; r++) out[2 + r] = r >= n_regions ? 0.0 : (nan ? qn : a.reg[r]);
}

}  // namespace ssde
#endif
