// ssde_knobs.hpp -- the SSDE_* environment variables the engine reads; DESIGN.md section 8 says what each is for, and
// tests/test_knobs_host.py holds the two in step.  Host code only.  knobs_from_env names every variable once and is the only code of
// the library that calls getenv: build() calls it once per handle (ssde_engine_build.hip), nothing reads the environment per evaluation.
#ifndef SSDE_KNOBS_HPP
#define SSDE_KNOBS_HPP
#include <algorithm>
#include <cstdlib>
#include <optional>
#include <string>

namespace ssde_engine {
// One member per variable; a default-initialised Knobs is the engine with no variable set.  std::optional: the variable's absence means
// something no value does.
struct Knobs {
    // presence-only switches (SSDE_NO_QUIET=0 switches quiet rows off like any other value): a fast path off, or a rule overridden
    bool no_quiet = false, quiet_always = false, no_na_sort = false;                      // quiet rows of the general kernel
    bool no_shared = false, no_tv = false, no_direct_fast = false, no_graph = false, no_derive = false, no_lattice = false, no_regroup = false;
    bool no_drift = false, no_drift_general = false, no_drift_pp = false, drift_pp_all = false;
    bool no_colvar = false, no_colvar_full = false, cv_no_share = false, cv_no_mu_cols = false, cv_no_few = false, tv_no_lean = false;
    bool no_exact_hess = false, publish = false, trace = false;
    std::optional<int> chunks, window, adj_tail, tv_waves, tv_minlen;   // time-window geometry (window, adj_tail, tv_waves >= 1; tv_minlen a multiple of WIN_ALIGN)
    std::optional<int> hess_window;                  // first warm-up of the Hessian pass's windows, rows (>= 1, rounded up to WIN_ALIGN)
    std::optional<int> drift_min_tracks, cv_adj;     // a track count decides for the register lanes / 0: forward tangents everywhere, 2: the reverse sweep for few columns too
    std::optional<int> lagstats;                     // 0: never built, 2: built whatever the rule says, 1: the rule (as unset)
    std::optional<bool> fused_finalize;              // 1: the finalising work inside iso_shared_kernel (slower); 0: always a finalize launch after
                                                     // iso_shared_kernel; unset: one workgroup per group where the plan allows it (iso_shared_wg_kernel)
    std::optional<std::string> iso_split, wave_clock;   // "fused" / "split" / explicit masks ("3,4,8"); the file the per-wave stamps go to at destroy
    int quiet_window = 0, adj_diag = 0;              // rows of memory after a missing row (0: the plan's warm-up); timing-experiment bits of iso_adj_kernel
    double grid_rtol = 1e-12;                        // how far an interval may be from the grid step and still count as regular (lattice_pad)
};

// win_align: WIN_ALIGN of ssde_device.hpp (SSDE_TV_MINLEN is rounded down to it, SSDE_HESS_WINDOW up), which a host-only header does not include
inline Knobs knobs_from_env(int win_align) {
    static const struct { const char* name; bool Knobs::*flag; } switches[] = {
        {"SSDE_NO_QUIET", &Knobs::no_quiet}, {"SSDE_QUIET_ALWAYS", &Knobs::quiet_always}, {"SSDE_NO_NA_SORT", &Knobs::no_na_sort}, {"SSDE_NO_SHARED", &Knobs::no_shared}, {"SSDE_NO_TV", &Knobs::no_tv},
        {"SSDE_NO_DIRECT_FAST", &Knobs::no_direct_fast}, {"SSDE_NO_GRAPH", &Knobs::no_graph}, {"SSDE_NO_DERIVE", &Knobs::no_derive}, {"SSDE_NO_LATTICE", &Knobs::no_lattice}, {"SSDE_NO_REGROUP", &Knobs::no_regroup},
        {"SSDE_NO_DRIFT", &Knobs::no_drift}, {"SSDE_NO_DRIFT_GENERAL", &Knobs::no_drift_general}, {"SSDE_NO_DRIFT_PP", &Knobs::no_drift_pp}, {"SSDE_DRIFT_PP_ALL", &Knobs::drift_pp_all}, {"SSDE_NO_COLVAR", &Knobs::no_colvar},
        {"SSDE_NO_COLVAR_FULL", &Knobs::no_colvar_full}, {"SSDE_CV_NO_SHARE", &Knobs::cv_no_share}, {"SSDE_CV_NO_MU_COLS", &Knobs::cv_no_mu_cols}, {"SSDE_CV_NO_FEW", &Knobs::cv_no_few}, {"SSDE_TV_NO_LEAN", &Knobs::tv_no_lean},
        {"SSDE_NO_EXACT_HESS", &Knobs::no_exact_hess}, {"SSDE_PUBLISH", &Knobs::publish}, {"SSDE_TRACE", &Knobs::trace}};
    auto num = [](const char* name) { const char* e = getenv(name); return e ? std::optional<int>(atoi(e)) : std::nullopt; };
    auto str = [](const char* name) { const char* e = getenv(name); return e && *e ? std::optional<std::string>(e) : std::nullopt; };   // (empty: no value)
    auto at_least = [](int lo, std::optional<int> v) { return v ? std::optional<int>(std::max(lo, *v)) : v; };
    Knobs k;
    for (const auto& s : switches) k.*s.flag = getenv(s.name) != nullptr;
    k.chunks = num("SSDE_CHUNKS");
    k.window = at_least(1, num("SSDE_WINDOW"));
    k.adj_tail = at_least(1, num("SSDE_ADJ_TAIL"));
    k.tv_waves = at_least(1, num("SSDE_TV_WAVES"));
    if (auto v = num("SSDE_TV_MINLEN")) k.tv_minlen = std::max(win_align, *v / win_align * win_align);
    if (auto v = num("SSDE_HESS_WINDOW")) k.hess_window = (std::min(std::max(1, *v), 1 << 24) + win_align - 1) / win_align * win_align;   // (64 x it fits an int)
    k.quiet_window = std::max(0, num("SSDE_QUIET_WINDOW").value_or(0));
    k.iso_split = str("SSDE_ISO_SPLIT");
    k.drift_min_tracks = num("SSDE_DRIFT_MIN_TRACKS");
    k.cv_adj = num("SSDE_CV_ADJ");
    if (auto v = num("SSDE_LAGSTATS")) k.lagstats = *v == 0 ? 0 : *v == 2 ? 2 : 1;
    if (auto v = num("SSDE_FUSED_FINALIZE")) k.fused_finalize = *v != 0;
    if (const char* e = getenv("SSDE_GRID_RTOL")) k.grid_rtol = std::max(0.0, atof(e));
    k.adj_diag = num("SSDE_ADJ_DIAG").value_or(0);
    k.wave_clock = str("SSDE_WAVE_CLOCK");
    return k;
}
}  // namespace ssde_engine
#endif
