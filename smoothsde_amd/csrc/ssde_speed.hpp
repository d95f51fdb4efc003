// ssde_speed.hpp -- speed along posterior state paths (ssde_path_speed): the per-(lane, draw) math, DESIGN.md §3.17.
//
// The backward walk of ssde_draws.hpp forms draw q's state at one row after the other, from the track's last row to its first;
// speed_step folds the row's VELOCITY (state column 2a + 1 of a CTCRW; no other model's state holds one) into a SpeedAcc -- the
// weighted sum of the speeds, the largest speed and its row, the two components of the resultant of the headings, the weighted rows
// at or below every threshold and a not-finite flag -- and hands back the row's 0 / 1 threshold indicators, which the caller adds
// over its draws into the per-row counts.  speed_finish turns the accumulator into the n_stat = 5 + n_thr numbers of the call.
// Only rows of the caller's data take part: a lattice-padded handle samples its padded rows (the recursion needs them) and hands
// them in with is_row = false.  Host- and device-compilable, like ssde_path.hpp; every loop has a constant trip count, so the
// accumulators stay in registers.
#ifndef SSDE_SPEED_HPP
#define SSDE_SPEED_HPP

#include <math.h>
#include <stdint.h>

#include "ssde_draws.hpp"

#ifndef SSDE_SPEED_MAX_THR
#define SSDE_SPEED_MAX_THR 8
#endif

#if defined(__clang__)
#define SSDE_SLOOP _Pragma("unroll")
#else
#define SSDE_SLOOP
#endif

namespace ssde {

constexpr int SPEED_NTHR = SSDE_SPEED_MAX_THR;
constexpr int SPEED_NSTAT_MAX = 5 + SPEED_NTHR;

// one (lane, draw): `mx` is the largest speed so far and `mx_row` the caller's row it was seen at (a double: the statistic is one,
// and rows below 2^53 are exact), `res` the resultant sum of w v / s
template <int D>
struct SpeedAcc {
    double sum, mx, mx_row, res[2], band[SPEED_NTHR];
    int rows, bad;
};

template <int D>
SSDE_HD void speed_init(SpeedAcc<D>& a) {
    a.sum = 0.0; a.mx = 0.0; a.mx_row = 0.0; a.rows = 0; a.bad = 0;
    a.res[0] = 0.0; a.res[1] = 0.0;
    SSDE_SLOOP for (int r = 0; r < SPEED_NTHR; r++) a.band[r] = 0.0;
}

SSDE_HD bool speed_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }     // neither NaN nor +-inf

// The state just drawn at one row: alpha; is_row: the row is a row of the caller's data, crow that row; w: its weight; thr(r):
// threshold r of n_thr.  below[r] is set to 1 where the row's speed is finite and <= thr(r), else to 0 (every entry, also past
// n_thr).  The walk runs from the track's last row to its first, so replacing the maximum on >= leaves the SMALLEST row of a tie.
// A band's weight is added only where the row is below, so a non-finite weight enters the sums it is added to and no other.
template <int MODEL, int D, int SD, class G>
SSDE_HD void speed_step(SpeedAcc<D>& a, const double (&alpha)[SD], bool is_row, int64_t crow, double w, G&& thr, int n_thr,
                        int (&below)[SPEED_NTHR]) {
    static_assert(MODEL == M_CTCRW && SD == 2 * D && D >= 1 && D <= 2, "a velocity column is a CTCRW's, one or two response columns");
    SSDE_SLOOP for (int r = 0; r < SPEED_NTHR; r++) below[r] = 0;
    if (!is_row) return;
    double v[D];
    SSDE_SLOOP for (int c = 0; c < D; c++) {
        v[c] = alpha[2 * c + 1];
        if (!speed_finite(v[c])) a.bad = 1;
    }
    double s;
    if (D == 1) {
        s = fabs(v[0]);
    } else {
        s = 0.0;
        SSDE_SLOOP for (int c = 0; c < D; c++) s += v[c] * v[c];
        s = sqrt(s);
    }
    a.sum += w * s;
    if (a.rows == 0 || s >= a.mx) { a.mx = s; a.mx_row = (double)crow; }
    if (s > 0.0) {
        SSDE_SLOOP for (int c = 0; c < D; c++) a.res[c] += w * (v[c] / s);
    }
    a.rows++;
    const bool fin = speed_finite(s);
    SSDE_SLOOP for (int r = 0; r < SPEED_NTHR; r++) {
        if (r < n_thr) {
            const bool in = fin && s <= thr(r);
            if (in) a.band[r] += w;
            below[r] = in ? 1 : 0;
        }
    }
}

// out[0 .. 5 + n_thr): the weighted sum of speeds, the largest speed, its row, the resultant (its second component 0 for D = 1),
// the band sums; every one NaN where a velocity was not finite (or no row of the caller's was seen).  Elements past 5 + n_thr are
// set to 0 and mean nothing.
template <int D>
SSDE_HD void speed_finish(const SpeedAcc<D>& a, int n_thr, double (&out)[SPEED_NSTAT_MAX]) {
    const bool nan = a.bad || a.rows == 0;
    const double qn = __builtin_nan("");
    out[0] = nan ? qn : a.sum;
    out[1] = nan ? qn : a.mx;
    out[2] = nan ? qn : a.mx_row;
    out[3] = nan ? qn : a.res[0];
    out[4] = nan ? qn : (D == 2 ? a.res[1] : 0.0);
    SSDE_SLOOP for (int r = 0; r < SPEED_NTHR; r++) out[5 + r] = r >= n_thr ? 0.0 : (nan ? qn : a.band[r]);
}

}  // namespace ssde
#endif
