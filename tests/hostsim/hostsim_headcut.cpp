// test-only host build of the window geometry with the early bulk cut (csrc/ssde_windows.hpp: head_early_cut), for
// tests/test_head_cut_plan_host.py.
#include <cmath>
#include <vector>

#include "../../smoothsde_amd/csrc/ssde_windows.hpp"

using namespace ssde_engine;

extern "C" {

// facts: the order of hostsim_lib.WINDOW_FACTS, then [lag_early, lag_cut_mask, lag_cut_min, lag_cut_step]; consts, params, ev as
// hostsim_window_geometry takes them; out = [n_chunks, window, t0, t0_delta, dual, n_chunks_d, t0_d, lag_K, s_stat, quiet_window,
// quiet_w, quiet_b0, lag_cut, the plan in force (n_chunks, window, warmup)]
void hostsim_headcut_geometry(const double* v, const int* c4, const double* p, int boost, int gave_up, const double* ev, double* out) {
    WindowFacts f;
    f.model = (int)v[0]; f.uniform_dt = v[1] != 0.0; f.dt_uniform = v[2]; f.dt_min = v[3]; f.dt_max = v[4];
    f.max_chunks = (int)v[5]; f.want_chunks = (int)v[6]; f.want_chunks_d = (int)v[7]; f.glen_max = (int)v[8]; f.n_groups = (int)v[9];
    f.use_shared = v[10] != 0.0; f.drift = (int)v[11]; f.cv_adj = v[12] != 0.0; f.cv_one_wave = v[13] != 0.0; f.chunks_forced = v[14] != 0.0;
    if (v[15] >= 0.0) f.window = (int)v[15];
    f.cv_eta_lo[0] = v[16]; f.cv_eta_lo[1] = v[17]; f.cv_eta_hi[0] = v[18]; f.cv_eta_hi[1] = v[19];
    f.any_dirty = v[20] != 0.0; f.quiet_ok = v[21] != 0.0; f.lag_ready = v[22] != 0.0; f.quiet_window = (int)v[23]; f.block_rows = (int)v[24];
    f.lag_early = v[25] != 0.0; f.lag_cut_mask = (unsigned)v[26]; f.lag_cut_min = (int)v[27]; f.lag_cut_step = (int)v[28];
    const WindowConsts c = {c4[0], c4[1], c4[2], c4[3]};
    const WindowParams a = {p[0], p[1], p[2], p[3], {p[4], p[5], p[6]}};
    const WindowPlan first = plan_windows(f, c, a, boost);
    WindowEval e;
    e.n_parts = (int)ev[0]; e.can_derive = ev[1] != 0.0; e.hess_req = ev[2] != 0.0; e.gain_last = (int)ev[3]; e.gain_usable = ev[4] != 0.0;
    const WindowGeometry g = window_geometry(f, c, a, first, boost, gave_up != 0, e);
    const double r[16] = {(double)g.n_chunks, (double)g.window, (double)g.t0, (double)g.t0_delta, g.dual ? 1.0 : 0.0, (double)g.n_chunks_d,
                          (double)g.t0_d, (double)g.lag_K, (double)g.s_stat, (double)g.quiet_window, (double)g.quiet_w, (double)g.quiet_b0,
                          (double)g.lag_cut, (double)g.plan.n_chunks, (double)g.plan.window, (double)g.plan.warmup};
    for (int i = 0; i < 16; i++) out[i] = r[i];
}

}  // extern "C"
