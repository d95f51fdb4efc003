// ssde_windows.hpp -- the time-window policy of the register and row-varying paths, as pure functions over plain
// structs: the stationary closed-loop radius, the warm-up and chunk plan, the geometry that follows the plan, the retry /
// rounding-floor / probation state machine around an evaluation, and the item plan and retry rule of the Hessian pass.  Host code
// only, no HIP type: the engine (ssde_engine*.hip, ssde_hess.hip) calls it next to its launches, tests/hostsim compiles it with g++
// and tests/test_windows_host.py and tests/test_hess_plan_host.py drive it without a GPU.
#ifndef SSDE_WINDOWS_HPP
#define SSDE_WINDOWS_HPP
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <optional>
#include <vector>

#include "../../include/ssde.h"
#include "ssde_math.hpp"

namespace ssde_engine {

constexpr double SSDE_WINDOW_TOL = 1e-11;  // largest tolerated relative hand-over disagreement

// Measured.  T0_COST: a row of the transient window, in stationary rows.  W0_RATIO: cost of a row of window 0 (every direction) over a
// row of a later window (one derived) on the general kernel -- 0 .. 1.45 swept, 3 % on CTCRW at 1.2, nothing on the scalar models.
constexpr double T0_COST = 3.0, W0_RATIO = 1.2;
// HEAD_T0_COST: a row of the transient window [0, t0) of a LONE wave (one wave per SIMD or fewer: the head of the lag-statistics path),
// in stationary rows of such a wave.  T0_COST was measured under throughput; this one from stamps inside the waves of the bench's
// batch (profiles/r08_b_phase_stamps.txt; per wave: r08_a_wave_clock.txt): the wave of the transient window walks its 16 gain-table
// rows in 6.3 us and its 48 stationary rows in direction form in 7.8 us -- 0.22 us a row, bound by its own dependent instructions;
// a stationary-only wave walks 48 rows in 5.2 - 6.5 us -- 0.12 us a row, one 8-row block per memory round trip.
constexpr double HEAD_T0_COST = 1.8;
constexpr int HEAD_WAVE_SLOTS = 1024;      // SIMDs of the chip: one wave each is one round of the head's launch
// A head whose windows are exactly the waves of ONE workgroup (HEAD_WG_WAVES = WG_WAVES of ssde_device.hpp, one wave per SIMD of a CU)
// checks its hand-overs in LDS and needs no dependent finalize launch for them (k_iso_shared.inc: iso_shared_wg_kernel).
// HEAD_WG_CREDIT: what that saves, in stationary rows of a lone wave (0.12 us a row) -- the two-launch form's extra microseconds per
// evaluation over the one-launch form on the same four windows of the bench's batch, finalize launch and read-back copy together:
// 5.7 us (medians 0.0478 against 0.0421 ms per step, profiles/r09_a_head_wg_ab.txt), 5.7 / 0.12 rows.
constexpr int HEAD_WG_WAVES = 4;
constexpr double HEAD_WG_CREDIT = 47.0;

// the layout constants the policy reads: WIN_ALIGN and SHARED_U of ssde_device.hpp, LAG_A and LAG_KMAX of ssde_lagstats.hpp (a
// host-only header does not include the former; the engine's one instance is WINDOW_CONSTS, ssde_engine.hpp)
struct WindowConsts { int win_align, shared_u, lag_a, lag_kmax; };

// ---- the stationary radius ---------------------------------------------------------------------------------------------------------
// Iterate the (data-independent) covariance recursion until it is stationary and return the spectral radius of the closed-loop
// matrix T - K Z there.  p0 = {p11, p12, p22} (CTCRW) or {p} (scalar models).
inline double stationary_rho(const ssde::CtcrwTrans& tr, double hobs, const double* p0) {
    double p11 = p0[0], p12 = p0[1], p22 = p0[2], k1 = 0, k2 = 0;
    for (int it = 0; it < 20000; it++) {
        const double F = p11 + hobs, iF = 1.0 / F;
        const double tp11 = p11 + tr.t12 * p12, tp12 = p12 + tr.t12 * p22, tp21 = tr.e * p12, tp22 = tr.e * p22;
        k1 = tp11 * iF; k2 = tp21 * iF;
        const double n11 = tp11 * (1.0 - k1) + tp12 * tr.t12 + tr.q11, n12 = -tp11 * k2 + tp12 * tr.e + tr.q12,
                     n22 = -tp21 * k2 + tp22 * tr.e + tr.q22;
        const double ch = std::fabs(n11 - p11) + std::fabs(n12 - p12) + std::fabs(n22 - p22);
        p11 = n11; p12 = n12; p22 = n22;
        if (ch <= 1e-15 * (std::fabs(p11) + std::fabs(p22))) break;
    }
    // L = [[1 - k1, t12], [-k2, e]]
    const double trc = (1.0 - k1) + tr.e, det = (1.0 - k1) * tr.e + k2 * tr.t12;
    const double disc = trc * trc - 4.0 * det;
    return disc >= 0.0 ? std::max(std::fabs(0.5 * (trc + std::sqrt(disc))), std::fabs(0.5 * (trc - std::sqrt(disc))))
                       : std::sqrt(std::fabs(det));
}
inline double stationary_rho(const ssde::ScalTrans& tr, double hobs, const double* p0) {
    double p = p0[0], k = 0;
    for (int it = 0; it < 20000; it++) {
        const double F = p + hobs, tp = tr.t * p;
        k = tp / F;
        const double np_ = tp * (tr.t - k) + tr.q;
        const double ch = std::fabs(np_ - p);
        p = np_;
        if (ch <= 1e-15 * std::fabs(p)) break;
    }
    return std::fabs(tr.t - k);
}

// an evaluation's transformed parameters, as the lanes get them (IsoArgs): CTCRW tau, beta = 1 / tau, sigma = 2 nu / sqrt(pi tau); OU
// tau, sigma = kappa; BM sigma; h = the observation variance
struct WindowParams { double tau, beta, sigma, h, p0[3]; };

// ... at an evaluation's parameters (1: no usable interval)
inline double stationary_rho(int model, double dt, const WindowParams& a) {
    if (!(dt > 0.0) || !std::isfinite(dt)) return 1.0;
    if (model == SSDE_MODEL_CTCRW) {
        ssde::CtcrwTrans tr;
        ssde::ctcrw_trans(dt, a.tau, a.beta, a.sigma, tr);
        return stationary_rho(tr, a.h, a.p0);
    }
    ssde::ScalTrans tr;
    if (model == SSDE_MODEL_OU_SSM) ssde::ou_trans(dt, a.tau, a.sigma, tr);
    else ssde::bm_trans(dt, a.sigma, tr);
    return stationary_rho(tr, a.h, a.p0);
}
// ... at constant working-scale parameters p1 = par[d], p2 = par[d + 1]
inline double closed_loop_rho(int model, double dt, double p1, double p2, double hobs, const double* p0) {
    WindowParams a = {0.0, 0.0, 0.0, hobs, {p0[0], model == SSDE_MODEL_CTCRW ? p0[1] : 0.0, model == SSDE_MODEL_CTCRW ? p0[2] : 0.0}};
    if (model == SSDE_MODEL_CTCRW) {
        a.tau = exp(p1);
        const double nu = exp(p2);
        a.beta = 1.0 / a.tau;
        a.sigma = 2.0 * nu / sqrt(M_PI * a.tau);
    } else if (model == SSDE_MODEL_OU_SSM) {
        a.tau = exp(p1);
        a.sigma = exp(p2);
    } else {
        a.sigma = exp(p1);
    }
    return stationary_rho(model, dt, a);
}

// ---- the warm-up -------------------------------------------------------------------------------------------------------------------
// Rows after which what a window did not see has decayed: rho^W <= 1e-18, plus `slack` rows for the t * rho^t growth of the forward
// sensitivity recursions, at least 16; SSDE_WINDOW (testing: deliberately short overlaps) replaces the estimate; the policy's boost
// multiplies either.  Not yet rounded to the window alignment (align_rows): the planners compare it with the track first.
inline int64_t warmup_rows(double rho, int slack, const std::optional<int>& knob, int boost) {
    int64_t w = (int64_t)std::ceil(std::log(1e-18) / std::log(std::max(rho, 1e-300))) + slack;
    w = std::max<int64_t>(w, 16);
    if (knob) w = *knob;
    return w * boost;
}
inline int64_t align_rows(int64_t w, int align) { return (w + align - 1) / align * align; }

// ---- the plan ----------------------------------------------------------------------------------------------------------------------
// what ssde_create found out about the batch and the engine's limits at this evaluation
struct WindowFacts {
    int model = 0;
    bool uniform_dt = false;
    double dt_uniform = 0.0, dt_min = 0.0, dt_max = 0.0;
    int max_chunks = 1, want_chunks = 1, want_chunks_d = 0, glen_max = 0, n_groups = 0;
    bool use_shared = false;
    int drift = 0;
    bool cv_adj = false, cv_one_wave = false, chunks_forced = false;
    std::optional<int> window;                   // SSDE_WINDOW
    double cv_eta_lo[2] = {0, 0}, cv_eta_hi[2] = {0, 0};
    // the geometry's
    bool any_dirty = false, quiet_ok = false, lag_ready = false;
    int quiet_window = 0;                        // SSDE_QUIET_WINDOW
    int block_rows = 1;                          // iso_block_rows(model): rows per block of the quiet-row flags
    // the lag statistics at early cuts (ssde_lagstats.hpp): SSDE_OPT_LAG_EARLY, and bit c: cut lag_cut_min + c lag_cut_step is built
    bool lag_early = false;
    unsigned lag_cut_mask = 0;
    int lag_cut_min = 0, lag_cut_step = 1;
};

struct WindowPlan {
    int n_chunks = 1, window = 0;
    int warmup = 0;        // usable warm-up length even when one window is planned (0: no usable forgetting)
    double rho = 1.0;      // spectral radius of the closed-loop matrix
};

// Warm-up length of a time window: iterate the covariance recursion at the smallest interval of the batch until it is stationary,
// take the spectral radius rho of the closed-loop matrix there, and ask for rho^W <= 1e-18 (warmup_rows).  The device-side hand-over
// check decides whether the estimate was good enough; it never has to be trusted.
inline WindowPlan plan_windows(const WindowFacts& f, const WindowConsts& c, const WindowParams& a, int boost) {
    WindowPlan p;
    if (f.max_chunks <= 1) return p;
    const double dt = f.uniform_dt ? f.dt_uniform : f.dt_min;
    double rho = stationary_rho(f.model, dt, a);
    if (f.drift == 3 && dt > 0.0 && std::isfinite(dt)) {
        // row-varying tau / nu: the slowest-forgetting corner of the ranges the linear predictors can reach on this design
        // (the hand-over check decides whether that was enough, as everywhere)
        rho = 0.0;
        const double dts[2] = {dt, f.uniform_dt ? dt : f.dt_max};
        for (int k = 0; k < 8; k++) {
            const double r = closed_loop_rho(f.model, dts[k & 1], (k & 2) ? f.cv_eta_hi[0] : f.cv_eta_lo[0],
                                             (k & 4) ? f.cv_eta_hi[1] : f.cv_eta_lo[1], a.h, a.p0);
            rho = std::max(rho, std::isfinite(r) ? r : 1.0);
        }
    }
    p.rho = rho;
    if (!(rho < 0.9995) || !std::isfinite(rho)) return p;  // no usable forgetting: sequential filter
    // The stationary CTCRW lanes run the filter as 1/D(q)^2 recursions (k_iso_shared.hip): with closed-loop poles
    // close to 1 their intermediate signals grow like 1/(1-rho)^2 and cancel in the innovation -- below rho = 0.97
    // that costs < 1e-12 relative; above, the evaluation stays on the sequential direction-form filter
    if (f.use_shared && !f.drift && f.model == SSDE_MODEL_CTCRW && rho > 0.97) return p;
    // (16 rows of slack; the reverse sweep carries none -- state and adjoint forget like rho^t -- and every warm-up row costs it a
    //  forward AND a backward row.  10^4 x 10^3 rows, 18 columns: W 48 -> 32, kernel 0.617 -> 0.572 ms, hand-over check
    //  9e-15 -> 6e-14 against the 1e-11 it has to meet)
    const int64_t w = warmup_rows(rho, f.cv_adj ? 0 : 16, f.window, boost);
    if (w > (int64_t)f.glen_max) return p;     // longer than a track: sequential filter
    const int W = (int)align_rows(w, c.win_align);
    // a window must be long enough to amortise its warm-up
    const int glmax = f.glen_max;
    int nc = f.want_chunks;
    if (f.drift == 3 && !f.cv_one_wave && !f.chunks_forced) { while (nc > 1 && (glmax / nc) < 2 * c.win_align) nc--; }     // (the cost below decides, not a rule)
    else if (f.cv_adj && !f.chunks_forced) {
        // one wave per (group, window) and per SIMD; a window walks its warm-up, its rows and -- for the backward recursion -- W rows
        // past its end forwards (~0.8 us a row), then its rows and that tail backwards (~1.2 us a row): rounds x that is what the
        // launch takes.  With SIMDs idle (few groups) windows shorter than their warm-up pay: the redundant rows run in parallel.
        nc = std::max(1, std::min(f.max_chunks, glmax / (2 * c.win_align)));
        const int ng = f.n_groups;                            // (the grid pads the groups to eight: those waves leave at once)
        int best = 1;
        double best_cost = (double)((ng + 1023) / 1024) * 2.0 * glmax;
        for (int k = 2; k <= nc; k++) {
            const double len = (double)glmax / k;
            const double cost = (double)(((int64_t)ng * k + 1023) / 1024) * (0.8 * (len + 2.0 * W) + 1.2 * (len + W));
            if (cost < best_cost) { best_cost = cost; best = k; }
        }
        nc = best;
    }
    else
    while (nc > 1 && (glmax / nc) < 2 * W) nc--;
    if (f.drift == 3 && !f.cv_one_wave && !f.chunks_forced) {
        // one workgroup per (group, window) and per CU: rounds x (rows of a window + its warm-up) is what the launch takes
        int best = 1;
        double best_cost = (double)((f.n_groups + 255) / 256) * glmax;
        for (int k = 2; k <= nc; k++) {
            const double cost = (double)(((int64_t)f.n_groups * k + 255) / 256) * ((double)glmax / k + W);
            if (cost < best_cost) { best_cost = cost; best = k; }
        }
        nc = best;
    }
    p.n_chunks = nc;
    p.window = nc > 1 ? W : 0;
    p.warmup = W;
    return p;
}

// ---- the geometry that follows the plan --------------------------------------------------------------------------------------------
// the first row of the shared-covariance kernels' stationary regime: the gain table's last row, rounded up to their prefetch block
inline int stationary_row(int gain_last, int shared_u) { return (gain_last + shared_u - 1) / shared_u * shared_u; }

// General kernel, every window on its own wave: window 0 carries EVERY direction (windows >= 1 derive one, k_iso.hip) but has no
// warm-up rows.  With equal windows its waves are the last to finish and the whole launch waits for them (CTCRW: 212 against 163
// instructions per row).  Balance: window 0 = [0, L0) with r L0 = L1 + W, the others split [L0, L) equally -- the geometry
// window_bounds already has for a transient window (t0 = L0), with nothing to subtract from window 1 (it has a wave of its own).
// Returns L0 in whole alignment units, 0 where the tracks are too short for it.
inline int balanced_window0(int glen, int nc, int window, bool can_derive, int win_align) {
    const double r = can_derive ? W0_RATIO : 1.0;
    const double L0 = ((double)glen / (nc - 1) + window) / (r + 1.0 / (nc - 1));
    const int t0 = (int)(L0 / win_align) * win_align;
    return (t0 >= 2 * win_align && t0 + 2 * window < glen) ? t0 : 0;
}

// what the geometry needs of this evaluation beyond the plan
struct WindowEval {
    int n_parts = 1;              // direction parts of the launch
    bool can_derive = false;      // windows >= 1 of the general kernel derive a direction: window 0 costs W0_RATIO a row
    bool hess_req = false;        // the Hessian kernels run instead of the evaluation
    int gain_last = 0;            // last row of the gain table
    bool gain_usable = false;     // ... which is stationary, with a non-zero 1 / F
};

struct WindowGeometry {
    WindowPlan plan;              // the plan in force (the head's own when the bulk comes from the lag statistics)
    int n_chunks = 1, window = 0; // windows launched (the transient window included) and their warm-up
    int t0 = 0, t0_delta = 0;     // the transient window [0, t0); rows taken off window 1, whose wave runs it too (0 with t0 > 0: it has a wave of its own)
    bool dual = false;            // mixed batch: the general launch runs a plan of its own ...
    int n_chunks_d = 0, t0_d = 0; // ... of this many windows, window 0 = [0, t0_d)
    int lag_K = 0;                // > 0: rows past lag_cut from the lag statistics, with this many taps
    int lag_cut = 0;              // the first bulk row: LAG_A, or t0 where the statistics of that cut exist (head_early_cut): the head is then window 0 alone
    int s_stat = 0;               // stationary_row of the gain table
    int quiet_window = 0;         // rows of memory of the quiet rows (0: none), in blocks: quiet_w, first quiet block: quiet_b0
    int quiet_w = 0, quiet_b0 = 0;
};

// The head of the lag-statistics path (rows [0, LAG_A) of every track) planned for latency.  Its launch is a few hundred waves on a
// chip of 1024 SIMDs, so what it takes is the dependent chain of rows of its longest wave, times the rounds of waves the grid needs --
// not the rows it walks in all: redundant warm-up rows on idle SIMDs cost nothing.  Compared, in stationary rows:
//   * the shared-wave geometry the throughput rules give (g as it comes in: the transient window on the wave of window 1, which is
//     shortened by t0_delta), its longest wave by window_bounds' rules (ssde_device.hpp);
//   * the transient window on a wave of its own (t0_delta = 0) and k = 1 .. max_chunks - 1 stationary windows dealt [t0, LAG_A)
//     equally: chain(k) = max(HEAD_T0_COST t0, W + ceil(units / k) WIN_ALIGN), rounds(k) = ceil(groups padded to 8 x (k + 1) / 1024);
//     k + 1 == HEAD_WG_WAVES is credited with HEAD_WG_CREDIT rows: those windows are one workgroup, which finishes in one launch.
// The cheapest is taken; at equal cost the shorter stationary chain (the transient's cost is a measured average: the plan should
// not hinge on it where more windows are free), then the fewer windows.  The shared-wave geometry stays unless one is strictly cheaper:
// with more groups than wave slots the rounds term keeps it.  Buffers are sized by max_chunks, which bounds k + 1.
inline void head_latency_plan(const WindowFacts& f, const WindowConsts& c, WindowGeometry& g) {
    const int WA = c.win_align, W = g.window, t0 = g.t0, rest = c.lag_a - t0;
    if (t0 <= 0 || rest <= 0 || g.n_chunks < 2) return;
    const int64_t g8 = ((int64_t)f.n_groups + 7) / 8 * 8;
    auto rounds = [&](int waves) { return (double)std::max<int64_t>(1, (g8 * waves + HEAD_WAVE_SLOTS - 1) / HEAD_WAVE_SLOTS); };
    auto ceil_div = [](int a, int b) { return (a + b - 1) / b; };
    const double transient = HEAD_T0_COST * t0;
    // the shared-wave geometry: window 1 and the longest other window, as window_bounds deals them
    double best_cost;
    {
        const int nw = g.n_chunks - 1, delta = g.t0_delta;
        const int cl = ceil_div(ceil_div(rest + delta, WA), nw) * WA;
        int len1, len_other = 0;
        if (cl <= delta + WA) {                       // (its short-track branch: a token window 1, the others share the rest)
            len1 = nw > 1 ? std::min(rest, 2 * WA) : rest;
            if (nw > 1) len_other = ceil_div(ceil_div(rest - len1, WA), nw - 1) * WA;
        } else {
            len1 = cl - delta;
            if (nw > 1) len_other = cl;
        }
        const double chain = std::max(transient + W + len1, len_other > 0 ? (double)(W + len_other) : 0.0);
        best_cost = rounds(nw) * chain;
    }
    const int units = ceil_div(rest, WA);
    const int kmax = std::min(std::max(2, f.max_chunks) - 1, std::max(1, units - 1));     // (k >= units: window_bounds would leave windows empty)
    int best_k = 0, best_stat = 0;
    for (int k = 1; k <= kmax; k++) {
        const int stat = W + ceil_div(units, k) * WA;
        const double cost = rounds(k + 1) * std::max(transient, (double)stat) - (k + 1 == HEAD_WG_WAVES ? HEAD_WG_CREDIT : 0.0);
        if (cost < best_cost || (best_k > 0 && cost == best_cost && stat < best_stat)) { best_cost = cost; best_k = k; best_stat = stat; }
    }
    if (best_k > 0) { g.n_chunks = best_k + 1; g.t0_delta = 0; }
}

// The bulk cut at the transient's end.  The forms need stationary gains for K rows before the first bulk row, and the
// head's plan already puts t0 = align(s_stat + W) with lag_K = W: rows [t0, LAG_A) are streamed only because the statistics stand at
// the fixed cut LAG_A.  Where statistics for the cut t0 exist the head is window 0 alone.  Decided after the head plan as it stands,
// and no other field moves: the transient window on a wave of its own (the latency plan's geometry), CTCRW, the option on, no forced
// window count, no Hessian request, no plan that has given up; K < t0 (the forms read lags 0 .. K of statistics built for lags < t0).
// A failed check boosts the warm-up, which moves t0 -- possibly off the list of cuts, and then the late cut runs.
inline int head_early_cut(const WindowFacts& f, const WindowConsts& c, const WindowGeometry& g, bool gave_up, const WindowEval& e) {
    if (!(f.lag_early && f.model == SSDE_MODEL_CTCRW && g.lag_K > 0 && g.t0 > 0 && g.t0_delta == 0 && !f.chunks_forced && !e.hess_req &&
          !gave_up && g.lag_K < g.t0 && g.t0 < c.lag_a)) return c.lag_a;
    const int k = g.t0 - f.lag_cut_min;
    if (k < 0 || f.lag_cut_step < 1 || k % f.lag_cut_step != 0 || k / f.lag_cut_step >= 32) return c.lag_a;
    return ((f.lag_cut_mask >> (k / f.lag_cut_step)) & 1u) ? g.t0 : c.lag_a;
}

inline WindowGeometry window_geometry(const WindowFacts& f, const WindowConsts& c, const WindowParams& a, const WindowPlan& first,
                                      int boost, bool gave_up, const WindowEval& e) {
    WindowGeometry g;
    g.lag_cut = c.lag_a;
    g.plan = first;
    g.n_chunks = first.n_chunks; g.window = first.window;
    g.s_stat = stationary_row(e.gain_last, c.shared_u);
    if (f.use_shared) {
        // Rows past LAG_A from the lag statistics, decided here for this evaluation: the cut K the window plan asks
        // for must fit the statistics (K <= LAG_KMAX) and the head (the stationary gains from row s_stat, K rows before LAG_A);
        // a plan that has given up, or gains that never became stationary, stream every row
        if (f.lag_ready && !f.drift && !e.hess_req && e.n_parts == 1 && !gave_up && e.gain_usable && first.warmup > 0 &&
            first.warmup <= c.lag_kmax && g.s_stat + first.warmup <= c.lag_a) g.lag_K = first.warmup;
        if (g.lag_K > 0) {
            // the head: every track capped at LAG_A rows, planned as a batch of that length
            WindowFacts head = f;
            head.glen_max = c.lag_a;
            g.plan = plan_windows(head, c, a, boost);
            g.n_chunks = g.plan.n_chunks; g.window = g.plan.window;
        }
        const int glen = g.lag_K > 0 ? c.lag_a : f.glen_max;
        // the covariance transient gets its own short window [0, t0): every other window (warm-up
        // included) then lies in the stationary regime and runs the lean kernel
        // A batch with more track groups than SIMDs needs no time windows to fill the chip, but the lean
        // stationary kernel only exists for windows past the covariance transient: split every track into
        // the transient window and ONE stationary window (same wave, so no extra work items)
        if (f.drift) {
            // every row costs the same here (HBM-bound; the table rows and the stationary rows run the same step): plain equal windows
        } else
        if (g.n_chunks == 1 && g.plan.warmup > 0 && f.max_chunks >= 2 && !f.chunks_forced) {
            g.window = g.plan.warmup;
            const int t0c = (int)align_rows(g.s_stat + g.window, c.win_align);
            if (t0c + 2 * g.window < glen) { g.t0 = t0c; g.n_chunks = 2; }
            else g.window = 0;
        } else
        if (g.n_chunks > 1) {
            g.t0 = (int)align_rows(g.s_stat + g.window, c.win_align);
            if (g.t0 + 2 * g.window >= glen) { g.t0 = 0; }                   // tracks too short to bother
            else if (g.n_chunks < f.max_chunks) g.n_chunks += 1;            // window 0 + the planned ones
        }
    }
    // the transient window (gain table, direction form) runs on the wave that owns window 1: that window is
    // shortened by what the transient rows cost, in stationary rows (T0_COST x t0)
    g.t0_delta = (int)(T0_COST * g.t0 + c.win_align - 1) / c.win_align * c.win_align;
    // ... except in the head of the lag-statistics path where a wave of its own is cheaper (t0 > 0 with t0_delta == 0, the meaning
    // the general kernel's balanced window 0 already has); a forced window count (SSDE_CHUNKS) keeps the throughput geometry: A/B
    if (g.lag_K > 0 && !f.chunks_forced) head_latency_plan(f, c, g);
    g.lag_cut = head_early_cut(f, c, g, gave_up, e);
    if (!f.use_shared && !f.drift && g.n_chunks > 1) {
        const int t0 = balanced_window0(f.glen_max, g.n_chunks, g.window, e.can_derive, c.win_align);
        if (t0 > 0) { g.t0 = t0; g.t0_delta = 0; }
    }
    // (CTCRW: the transfer-function lanes lose digits when the closed-loop poles approach 1 -- the limit plan_windows has for them)
    // (a plan that has given up on windows gives up on quiet rows too: with them the retry would run the identical plan again)
    if (f.quiet_ok && !gave_up && e.gain_usable && g.plan.warmup > 0 && e.n_parts == 1 &&
        !(f.model == SSDE_MODEL_CTCRW && g.plan.rho > 0.97)) {
        const int U = f.block_rows;
        g.quiet_window = g.plan.warmup;
        // (testing: a memory of its own, deliberately short -- the check at the switch has to notice; a retry doubles it like a warm-up)
        if (f.quiet_window > 0) g.quiet_window = f.quiet_window * boost;
        g.quiet_w = (g.quiet_window + U - 1) / U;
        g.quiet_b0 = g.s_stat / U + 1;
    }
    // Mixed batch: the general launch gets a plan of its own -- enough windows to fill its waves, each at least two warm-ups long,
    // window 0 balanced as in the all-general case
    if (f.use_shared && f.any_dirty && f.want_chunks_d > 0 && g.n_chunks > 1 && f.max_chunks > 1 && !gave_up) {
        int nc = f.want_chunks_d;
        while (nc > 1 && (f.glen_max / nc) < 2 * g.window) nc--;
        if (nc > 1) {
            g.dual = true;
            g.n_chunks_d = nc;
            g.t0_d = balanced_window0(f.glen_max, nc, g.window, e.can_derive, c.win_align);
        }
    }
    return g;
}

// ---- the retry policy --------------------------------------------------------------------------------------------------------------
// what a decision asks of every engine of the handle (apply_chunks): their chunk limits are per engine, the policy is the handle's
enum class ChunkAction {
    none,
    sequential_saving,   // give up on windows: remember the chunk limits, then one sequential window
    sequential,          // ... again, after a probation that failed: the limits remembered then still stand
    restore              // probation of a plan that had given up: the remembered limits
};
// E: anything with max_chunks, want_chunks, saved_max_chunks, saved_want_chunks (ssde_handle; the tests' stand-in)
template <class E>
inline void apply_chunks(E& e, ChunkAction act) {
    if (act == ChunkAction::sequential_saving) { e.saved_max_chunks = e.max_chunks; e.saved_want_chunks = e.want_chunks; }
    if (act == ChunkAction::sequential_saving || act == ChunkAction::sequential) { e.max_chunks = 1; e.want_chunks = 1; }
    if (act == ChunkAction::restore) { e.max_chunks = e.saved_max_chunks; e.want_chunks = e.saved_want_chunks; }
}

// An evaluation with the window policy around it: re-evaluate with a wider warm-up until the time windows agree, narrow again on
// probation after `cooldown` calm evaluations.  Every decision is taken on the REDUCED check value (a sum of non-negative per-shard /
// per-rank maxima, compared with the single-engine tolerance: conservative), so the shards of a parent and the ranks of a communicator
// move in lockstep and the collective inside an evaluation is entered by everyone the same number of times.
struct WindowPolicy {
    int window_boost = 1;          // multiplies the estimated warm-up after a failed hand-over check
    bool gave_up = false;          // windows given up: every engine runs one sequential window, without quiet rows or lag statistics
    // recovery from a widened plan: after `cooldown` evaluations accepted at the first try the boost is halved (or a given-up window
    // plan restored) on probation; a failure on probation restores the level that worked and doubles the cooldown
    int calm = 0, cooldown = 32, probe_from = 0;
    bool probing = false;
    double check_floor = 0.0;      // > 0: a disagreement that a 4x longer warm-up did NOT reduce -- rounding in the states, not a short warm-up; accepted up to here
    double check_max = 0.0;        // largest accepted hand-over disagreement since create
    double last_check = 0.0;
    int n_retries = 0;

    // what the planners multiply their warm-up by
    int boost() const { return window_boost; }

    // one call of ssde_eval: the attempt counter and the check values of the last two attempts that each made this call quadruple the warm-up
    struct Call {
        int attempt = 0;
        double seen[2] = {-1.0, -1.0};
    };
    // what an attempt showed
    struct Attempt {
        double check;          // the reduced hand-over check
        bool finite;           // the value is finite
        bool one_window;       // one window ran, without quiet rows or lag statistics: no hand-over that could disagree
        bool dist;             // shards or ranks: the others may have had something to disagree, and everyone decides alike
        bool replans;          // the path plans from the ranges its PREVIOUS evaluation saw (row-varying paths)
    };
    struct Verdict {
        bool retry;
        ChunkAction engines;
    };

    Verdict after_attempt(Call& c, const Attempt& a) {
        const Verdict accept = {false, ChunkAction::none}, again = {true, ChunkAction::none};
        last_check = a.check;
        // hand-over check of the time windows (k_iso.hip): widen the warm-up and re-evaluate
        // until the windows agree with each other; 64x the estimate ends in one sequential window
        if (last_check <= std::max(SSDE_WINDOW_TOL, check_floor)) return accept;
        // ROUNDING FLOOR.  What a short warm-up leaves behind decays with its length; a SMALL disagreement that stays where it is
        // while the warm-up is quadrupled TWICE (16 x the rows) is not the warm-up's: it is rounding in the states themselves (fixes
        // that are very precise against the movement between them: P11 ~ sigma_obs^2 next to P22 ~ 1, the gains 1 - O(sigma_obs^2)),
        // the same in one sequential window, where nothing would notice it.  Such a floor is accepted from here on (up to 4 x what was
        // seen, never beyond 1e-8) and the plan goes back to the warm-up it had -- instead of ending in ONE window per track, two orders
        // of magnitude slower on long tracks, for the same digits.  (A slowly forgetting mode of small amplitude is NOT flat over 16 x
        // the rows: tests/test_gpu_drift.py::test_forced_short_warm_up_is_caught_and_repaired.  The value is the reduced one: shards
        // and ranks decide alike.)
        if (c.seen[0] > 0.0 && c.seen[1] > 0.0 && c.seen[0] <= 1e-8 && c.seen[1] <= 1e-8 && last_check <= 1e-8 &&
            c.seen[1] >= 0.5 * c.seen[0] && last_check >= 0.5 * c.seen[1] && a.finite) {
            check_floor = std::min(1e-8, 4.0 * std::max(last_check, std::max(c.seen[0], c.seen[1])));
            // (kept as it is: "/ 16" takes back exactly two quadruplings.  A call whose first check was not flat with the next two finds
            //  the floor one attempt later, after three: its boost stays at x4 of what the call started from)
            window_boost = std::max(1, window_boost / 16);
            return accept;
        }
        // (one window has no hand-over to disagree -- unless quiet rows ran: their switch check is folded into the same
        //  value, and a longer memory, finally none at all, is the repair)
        if (!a.dist && a.one_window) return accept;
        // a non-finite nllk is rejected by the caller whatever the windows did: no retry, and no lasting
        // widening of the plan because an optimiser probed an absurd parameter once
        if (!a.finite) return accept;
        // (a plan that has given up runs one window WITHOUT quiet rows, so nothing is left to disagree; the cap is for whatever that
        //  reasoning missed: the failure is then reported through check_max instead of spinning -- ADVICE r04.  Kept as it is: "> 6"
        //  allows seven retries)
        if (c.attempt > 6) return accept;
        n_retries++;
        calm = 0;
        const int attempt = c.attempt++;
        if (probing && attempt == 0) {
            // the narrower plan tried on probation does not hold here: back to the one that worked, and wait twice
            // as long before the next try
            probing = false;
            cooldown = std::min(cooldown * 2, 1 << 14);
            if (probe_from == 0) { gave_up = true; return {true, ChunkAction::sequential}; }
            window_boost = probe_from;
            return again;
        }
        // the row-varying paths plan from the parameter ranges their PREVIOUS evaluation saw: after a jump in the parameters the first
        // retry needs no boost, just this evaluation's own ranges
        if (a.replans && attempt == 0) return again;
        if (attempt >= 3) {                                            // give up on windows: sequential filter
            // (kept as it is: the boost stays where the retries left it -- x64 -- under the sequential plan)
            const bool first = !gave_up;
            gave_up = true;
            return {true, first ? ChunkAction::sequential_saving : ChunkAction::sequential};
        }
        c.seen[0] = c.seen[1]; c.seen[1] = last_check;
        window_boost *= 4;
        return again;
    }

    // after the accepted attempt; forced: SSDE_CHUNKS set the window count, which is then the tester's for good
    ChunkAction end_call(const Call& c, bool finite, bool forced) {
        if (finite && !(last_check <= check_max)) check_max = last_check;
        // (the floor belongs to the regime that showed it: an evaluation whose windows agree outright ends it, so that a later, genuinely
        //  short warm-up is not waved through under an old allowance)
        if (last_check <= SSDE_WINDOW_TOL) check_floor = 0.0;
        // A widened plan is not for life: one slow-forgetting parameter vector in a line search would otherwise tax every
        // later evaluation.  Every evaluation is checked, so narrowing on probation is safe -- a failure costs one retry.
        if (c.attempt != 0 || forced) return ChunkAction::none;
        calm++;
        if (probing && calm >= 4) probing = false;           // the narrower plan holds
        if (calm >= cooldown && (gave_up || window_boost > 1)) {
            calm = 0;
            probing = true;
            if (gave_up) {
                probe_from = 0;
                gave_up = false;
                return ChunkAction::restore;
            }
            probe_from = window_boost;
            window_boost = std::max(1, window_boost / 2);
        }
        return ChunkAction::none;
    }

    // ssde_widen_windows (factor >= 1; the caller sends every engine to one sequential window for factor <= 0), ssde_relax_windows
    void widen(int factor) { if (factor > 0 && window_boost < (1 << 20)) window_boost *= factor; }
    void relax() { window_boost = std::max(1, window_boost / 2); }
};

// ---- the Hessian pass of the lane = direction path (ssde_hess.hip: hess_tv_device, k_tv_hess.hip) ---------------------------------
// Its windows are window_bounds' equal windows (t0 = 0) with a warm-up of its own; one wave per (track, pair block, window).
constexpr double SSDE_HESS_WINDOW_TOL = 1e-10;   // largest tolerated hand-over disagreement of a hyper-dual component

// the first attempt's warm-up: second-order tangents forget like t^2 rho^t -- twice the evaluation's warm-up and one alignment
// unit, 0 (one sequential window per track) where the evaluation has none; SSDE_HESS_WINDOW (rows, already aligned) replaces either
// (testing: the hand-over check decides, as everywhere)
inline int hess_first_warmup(int tv_window, const std::optional<int>& knob, int win_align) {
    if (knob) return *knob;
    return tv_window > 0 ? 2 * tv_window + win_align : 0;
}
// windows of a track of L steps: as many as keep `waves` waves busy over M tracks x n_pb pair blocks, each at least two alignment
// units of scored rows, and only on tracks of at least two warm-ups
inline int hess_window_cap(int waves, int64_t M, int n_pb) { return (int)std::max<int64_t>(1, (waves + M * n_pb - 1) / (M * n_pb)); }
inline int hess_track_windows(int L, int W, int nc_cap, int win_align) {
    if (!(W > 0 && L >= 2 * W)) return 1;
    return std::max(1, std::min(nc_cap, (L + 2 * win_align - 1) / (2 * win_align)));
}
// The work items in (track, pair block, window) order: the windows of one (track, pair block) are neighbours in the list, which is
// what hess_finish_kernel's hand-over check (item against item + 1) assumes.  Item: {track, window c, of nc, pair block} (TvItem).
template <class Item, class Lengths>
inline void hess_item_plan(const Lengths& track_steps, int64_t M, int n_pb, int W, int waves, int win_align, std::vector<Item>& items) {
    items.clear();
    const int nc_cap = hess_window_cap(waves, M, n_pb);
    for (int64_t t = 0; t < M; t++) {
        const int nc = hess_track_windows((int)track_steps[(size_t)t], W, nc_cap, win_align);
        for (int b = 0; b < n_pb; b++)
            for (int c = 0; c < nc; c++) items.push_back(Item{(int32_t)t, c, nc, b});
    }
}
// after a failed hand-over check of attempt `attempt` (0-based): four times the warm-up; one sequential window (0) after the
// fourth failure or where a track no longer holds two warm-ups
inline int hess_next_warmup(int W, int attempt, int glen_max) {
    W = attempt >= 3 ? 0 : 4 * W;
    if ((int64_t)2 * W > glen_max) W = 0;
    return W;
}
// what ssde_last_hess_plan reports of the last ssde_hess: the accepted attempt's warm-up, the most windows a track was cut into,
// the attempts it took and the accepted hand-over check; all 0 where no windowed pass ran.  Several engines: the largest of each.
struct HessPlanInfo {
    int warm_up = 0, windows_max = 0, attempts = 0;
    double check = 0.0;
    void merge(const HessPlanInfo& o) {
        warm_up = std::max(warm_up, o.warm_up); windows_max = std::max(windows_max, o.windows_max);
        attempts = std::max(attempts, o.attempts); check = std::max(check, o.check);
    }
};

}  // namespace ssde_engine
#endif
