// ssde_engine_iso.hip -- one evaluation on the register Kalman path (constant coefficients, or a row-varying drift): decode the
// parameters, plan the windows and their geometry (ssde_windows.hpp), the gain table of the shared-covariance kernels, the launches (shared / general / drift / mixed batch) and
// the finalising launch (hand-over checks + fixed-order sums).  Called from eval_device (ssde_engine.hip).
#include "ssde_engine.hpp"
#include "ssde_lagforms.hpp"
#include "ssde_headforms.hpp"
#include "ssde_tf.hpp"

#include <chrono>

using namespace ssde_engine;

namespace {

// what the window plan and its geometry read of the handle (ssde_windows.hpp)
WindowFacts window_facts(const ssde_handle* h) {
    WindowFacts f;
    f.model = h->model; f.uniform_dt = h->uniform_dt; f.dt_uniform = h->dt_uniform; f.dt_min = h->dt_min; f.dt_max = h->dt_max;
    f.max_chunks = h->max_chunks; f.want_chunks = h->want_chunks; f.want_chunks_d = h->want_chunks_d;
    f.glen_max = h->glen_max; f.n_groups = h->n_groups; f.use_shared = h->use_shared; f.drift = h->drift;
    f.cv_adj = h->cv_adj; f.cv_one_wave = h->cv_one_wave(); f.chunks_forced = h->chunks_forced; f.window = h->knobs.window;
    for (int j = 0; j < 2; j++) { f.cv_eta_lo[j] = h->cv_eta_lo[j]; f.cv_eta_hi[j] = h->cv_eta_hi[j]; }
    f.any_dirty = h->n_clean_groups < h->n_groups; f.quiet_ok = h->quiet_ok; f.lag_ready = h->lag_ready;
    f.quiet_window = h->knobs.quiet_window; f.block_rows = iso_block_rows(h->model);
    f.lag_early = h->lag_early; f.lag_cut_mask = h->lag_cut_mask; f.lag_cut_min = LAG_CUT_MIN; f.lag_cut_step = LAG_CUT_STEP;
    return f;
}

// Shared-covariance path: run the covariance half of the filter (ssde_math.hpp) ONCE on the host
// for the regular grid -- it does not depend on the observations -- until it is bitwise
// stationary, upload the gains, and return the data-independent likelihood terms
// (D/2 sum log F and its derivatives, weighted by how many tracks reach each row).
// (the stationarity test of the covariance recursion -- gain_close, ctcrw_cov_settled, GAIN_SETTLED_ROWS -- lives in ssde_gain_feed.hpp)

// a slot of the ring for this evaluation's table: the ring protects the pinned slot of an ASYNCHRONOUS caller's earlier evaluation
// (ssde_eval_device); a synchronous ssde_eval has read its result back before the next call: no event traffic on that path
int gain_ring_slot(ssde_handle* h, int& slot) {
    slot = h->par_next;
    h->par_next = (h->par_next + 1) % PAR_RING;
    if (h->use_shared && (!h->sync_call || h->par_ev_pending[slot])) { HIPCHK(h, hipEventSynchronize(h->par_ev[slot])); h->par_ev_pending[slot] = false; }
    return SSDE_OK;
}
int gain_ring_copy(ssde_handle* h, IsoArgs& a, int slot, int rows, hipStream_t s) {
    double* host = h->gain_pinned + (size_t)slot * h->gain_rows_cap * GAIN_ROW;
    double* dev = h->gain_ring.p + (size_t)slot * h->gain_rows_cap * GAIN_ROW;
    if (h->use_shared) {                                    // (otherwise only the stationary constants are wanted)
        HIPCHK(h, hipMemcpyAsync(dev, host, (size_t)rows * GAIN_ROW * 8, hipMemcpyHostToDevice, s));
        if (!h->sync_call) { HIPCHK(h, hipEventRecord(h->par_ev[slot], s)); h->par_ev_pending[slot] = true; }
    }
    a.gain = dev;
    return SSDE_OK;
}

// defer: the launch may take the table by value (the head of the lag-statistics path, iso_shared_wg_kernel) -- the rows go to the
// handle's scratch, no ring slot is taken, no event touched and nothing copied; a.gain stays NULL until feed_gain_table has seen
// the geometry.  Otherwise: a ring slot, the pinned rows and the copy, as ever.
template <int D>
int build_gain_table(ssde_handle* h, IsoArgs& a, int mask, hipStream_t s, double add[4], bool defer = false) {
    int slot = -1;
    double* host;
    if (defer) {
        if (h->gain_scratch.size() < h->gain_rows_cap * GAIN_ROW) h->gain_scratch.resize(h->gain_rows_cap * GAIN_ROW);
        host = h->gain_scratch.data();
    } else {
        const int st = gain_ring_slot(h, slot);
        if (st) return st;
        host = h->gain_pinned + (size_t)slot * h->gain_rows_cap * GAIN_ROW;
    }
    const int tmax = h->glen_max;                 // rows 0 .. tmax-1 can be asked for
    // running sums of log F and of its derivatives, row by row (member buffers: no allocation per evaluation)
    std::vector<double>& cum_ld = h->gain_cum[0];
    std::vector<double>* cum_g = &h->gain_cum[1];
    for (int j = 0; j < 1 + NDIRP; j++) { if ((int)h->gain_cum[j].capacity() < tmax) h->gain_cum[j].reserve(tmax); h->gain_cum[j].clear(); }
    int last = 0, stable = 0;
    (void)mask;
    // Stationarity test.  In floating point the recursion ends in a last-bit limit cycle rather than a
    // bitwise fixed point, so "stationary" = every component moved by less than 2e-15 relative for 4 rows
    // in a row; the row reached then is used for all later rows (a 1e-15 relative perturbation of gains
    // that themselves carry rounding errors of that size).
    auto close = gain_close;
    if (h->model == SSDE_MODEL_CTCRW) {
        CtcrwCov<15> C;
        C.init(a.p0[0], a.p0[1], a.p0[2]);
        double ld = 0.0;
        for (int t = 0; t < tmax; t++) {
            const CtcrwCov<15> prev = C;
            CtcrwGain G;
            const double F = C.p11 + a.h;
            ctcrw_cov_step<D, 15>(C, a.ctr, a.h, false, G);
            double* r = host + (size_t)t * GAIN_ROW;
            r[0] = G.iF; r[1] = G.k1; r[2] = G.k2; r[3] = G.bm;
            for (int j = 0; j < NDIRP; j++) { r[4 + j] = G.diF[j]; r[7 + j] = G.dk1[j]; r[10 + j] = G.dk2[j]; }
            r[13] = r[14] = r[15] = 0.0;
            ld += (G.iF != 0.0) ? std::log(std::fabs(F)) : 0.0;
            cum_ld.push_back(ld);
            for (int j = 0; j < NDIRP; j++) cum_g[j].push_back(C.gld[j]);
            last = t;
            stable = ctcrw_cov_settled(C, prev) ? stable + 1 : 0;
            if (stable >= GAIN_SETTLED_ROWS) break;
        }
        h->stat_p[0] = C.p11; h->stat_p[1] = C.p12; h->stat_p[2] = C.p22;
        for (int j = 0; j < NDIRP; j++) { h->stat_p[3 + 3 * j] = C.d11[j]; h->stat_p[4 + 3 * j] = C.d12[j]; h->stat_p[5 + 3 * j] = C.d22[j]; }
    } else {
        ScalCov<15> C;
        C.init(a.p0[0]);
        double ld = 0.0;
        for (int t = 0; t < tmax; t++) {
            const ScalCov<15> prev = C;
            ScalGain G;
            const double F = C.p + a.h;
            if (h->model == SSDE_MODEL_OU_SSM) scal_cov_step<D, 15, true>(C, a.str, a.h, false, G);
            else scal_cov_step<D, 15, false>(C, a.str, a.h, false, G);
            double* r = host + (size_t)t * GAIN_ROW;
            for (int k = 0; k < GAIN_ROW; k++) r[k] = 0.0;
            r[0] = G.iF; r[1] = G.k; r[2] = G.c;
            for (int j = 0; j < NDIRP; j++) { r[4 + j] = G.diF[j]; r[7 + j] = G.dk[j]; }
            ld += (G.iF != 0.0) ? std::log(std::fabs(F)) : 0.0;
            cum_ld.push_back(ld);
            for (int j = 0; j < NDIRP; j++) cum_g[j].push_back(C.gld[j]);
            last = t;
            bool same = close(C.p, prev.p);
            for (int j = 0; j < NDIRP && same; j++) same = close(C.dp[j], prev.dp[j]);
            stable = same ? stable + 1 : 0;
            if (stable >= GAIN_SETTLED_ROWS) break;
        }
        for (int i = 0; i < 12; i++) h->stat_p[i] = 0.0;
        h->stat_p[0] = C.p;
        for (int j = 0; j < NDIRP; j++) h->stat_p[3 + 3 * j] = C.dp[j];
    }
    const int rows = last + 1;
    h->last_gain_rows = rows;
    // (quiet rows of the general kernel: the covariance after the last row, and what a further row adds to sum log F / sum dF / F)
    h->gain_stationary = stable >= GAIN_SETTLED_ROWS && last >= 1;
    if (last >= 1) {
        h->stat_ld = cum_ld[last] - cum_ld[last - 1];
        for (int j = 0; j < NDIRP; j++) h->stat_gld[j] = cum_g[j][last] - cum_g[j][last - 1];
    }
    a.gain = nullptr;
    if (!defer) { const int st = gain_ring_copy(h, a, slot, rows, s); if (st) return st; }
    a.gain_last = last;
    for (int k = 0; k < GAIN_ROW; k++) a.gain_stat[k] = host[(size_t)last * GAIN_ROW + k];
    fill_stat_consts(h->model, h->d, a);
    // data-independent terms: a track with ns scored rows contributes cum(ns - 1); past the
    // stationary row every further row adds the same increment
    auto cum_at = [&](const std::vector<double>& c, int idx) {
        if (idx <= last) return c[idx];
        const double inc = last > 0 ? c[last] - c[last - 1] : c[last];
        return c[last] + inc * (double)(idx - last);
    };
    double s_ld = 0.0, s_g[NDIRP] = {0, 0, 0};
    for (auto& e : h->clean_ns_hist) {
        s_ld += (double)e.second * cum_at(cum_ld, e.first - 1);
        for (int j = 0; j < NDIRP; j++) s_g[j] += (double)e.second * cum_at(cum_g[j], e.first - 1);
    }
    add[0] = 0.5 * D * s_ld;
    for (int j = 0; j < NDIRP; j++) add[1 + j] = 0.5 * D * s_g[j];
    return SSDE_OK;
}

// A deferred table (build_gain_table) once the geometry is known: by value in the launch's argument block when the launch is the
// wg entry and the rows fit (ssde_gain_feed.hpp) -- no copy, no ring slot, no event: the table belongs to its launch, so no evaluation
// in flight can see another's --, through the ring and the copy otherwise.
int feed_gain_table(ssde_handle* h, IsoArgs& a, bool wg, hipStream_t s, HeadGain& gv) {
    const int rows = a.gain_last + 1;
    gv.rows = 0;
    if (wg && head_gain_pack(h->gain_scratch.data(), rows, HEAD_GAIN_ROWS, gv.v)) { gv.rows = rows; return SSDE_OK; }
    int slot;
    const int st = gain_ring_slot(h, slot);
    if (st) return st;
    memcpy(h->gain_pinned + (size_t)slot * h->gain_rows_cap * GAIN_ROW, h->gain_scratch.data(), (size_t)rows * GAIN_ROW * 8);
    return gain_ring_copy(h, a, slot, rows, s);
}

// The bulk's forms at this evaluation (ssde_lagforms.hpp): the taps are the impulse responses of the lanes' own stationary step
// (TfCtcrw::step_stat, ssde_tf.hpp, here on the host) to a unit increment -- u for lam, r for rr -- and the constants those lanes
// finish with.  K taps for the forms, K - LAG_CHECK for the check.  (M, s, n: the caller's)
void lag_form_taps(const IsoArgs& a, int d, int mask, int K, LagFormArgs& f) {
    TfCtcrw<1, DIR_SIG | DIR_MU> T;
    T.setup(a);
    T.cm[0] = 0.0;                              // (the mu dt terms enter through s and n)
    double y = 0.0;
    T.init(&y);
    y = 1.0;                                    // dy_0 = 1, then 0
    for (int t = 0; t < LAG_N; t++) f.lam[t] = f.rr[t] = 0.0;
    for (int t = 0; t <= K && t < LAG_N; t++) {         // (taps beyond the cut are zero: nothing reads them)
        T.reset_acc();
        T.step_stat(&y);
        f.lam[t] = T.su[0];
        f.rr[t] = T.r1[0];
    }
    f.K = K; f.Kc = K - LAG_CHECK; f.d = d; f.mask = mask;
    lag_tap_sums(f);
    for (int i = 0; i < 2; i++) f.cm[i] = i < d ? a.statc[29 + i] : 0.0;
    for (int i = 0; i < 48; i++) f.statc[i] = a.statc[i];
}

// The same for OU_SSM / BM_SSM (BasisScal::step_stat, ssde_tf.hpp, here on the host): the responses of u, A1 and A3 -- as the row's
// products read them, before the step -- to a unit impulse in the level (OU_SSM) or a unit step in the level, which is a unit
// increment (BM_SSM), with the step's constant inputs taken out; those give the affine parts, the fixed point of the same step
// under y == ref (OU_SSM) or under increments == 0 (BM_SSM), in closed form: with c = t - k the closed-loop factor,
//     OU_SSM:  x* - mu = k (ref - mu) / (1 - c)   (1 - c = b + k)
//              kap_u = ref - x* = b (ref - mu) / (1 - c),  kap_A1 = kap_u / (1 - c),  kap_A3 = (dt_ x* + db mu) / (1 - c) = dt_ (x* - mu) / (1 - c)
//     BM_SSM:  kap_u = -mu dt / k = -mu dt / (1 - c),  kap_A1 = kap_u / (1 - c),  A3 == 0
// and mx* = b / (1 - c) for both.
template <int MODEL>
void lag_form_taps_scal_model(const IsoArgs& a, int K, LagScalArgs& f) {
    BasisScal<MODEL, 1, DIR_SIG | DIR_MU | DIR_P1 | DIR_P2> T;
    T.setup(a);
    T.cmu[0] = T.dbmu[0] = 0.0;                 // (the constant inputs enter through the affine parts)
    double y = 0.0;
    T.init(&y);
    for (int t = 0; t < LAG_N; t++) f.lam[t] = f.t1[t] = f.t3[t] = 0.0;
    for (int t = 0; t <= K && t < LAG_N; t++) {         // (taps beyond the cut are zero: nothing reads them)
        y = (MODEL == M_OU_SSM && t > 0) ? 0.0 : 1.0;
        f.lam[t] = y - T.x[0]; f.t1[t] = T.A1[0]; f.t3[t] = T.A3[0];
        T.step_stat(&y);
    }
}
void lag_form_taps_scal(int model, const IsoArgs& a, int d, int mask, int K, const double* ref, LagScalArgs& f) {
    if (model == SSDE_MODEL_OU_SSM) lag_form_taps_scal_model<M_OU_SSM>(a, K, f);
    else lag_form_taps_scal_model<M_BM_SSM>(a, K, f);
    f.K = K; f.Kc = K - LAG_CHECK; f.d = d; f.mask = mask; f.has_p2 = model == SSDE_MODEL_OU_SSM;
    const double* c = a.statc;
    const double k = c[1], omc = 1.0 - c[2], b = c[4], dt_ = c[5];
    for (int i = 0; i < 2; i++) {
        f.ku[i] = f.k1[i] = f.k3[i] = 0.0;
        if (i >= d) continue;
        if (model == SSDE_MODEL_OU_SSM) {
            const double dm = ref[i] - a.mu[i];
            f.ku[i] = b * dm / omc;
            f.k3[i] = dt_ * (k * dm / omc) / omc;
        } else {
            f.ku[i] = -c[19 + i] / omc;
        }
        f.k1[i] = f.ku[i] / omc;
    }
    f.mxs = b / omc;
    for (int i = 0; i < 48; i++) f.statc[i] = a.statc[i];
}

// ... and their result into the reducing launch's arguments, as the window after the `n_windows` that live in the partial sums
// (cut: the first bulk row -- LAG_A, or an early cut whose statistics the handle holds)
int lag_forms_into(ssde_handle* h, const IsoArgs& a, int order, int K, int n_windows, ReduceArgs& ra, int cut) {
    // the reductions recognise the by-value window as the one after the windows of direction part 0 (reduce_slot, reduce_all_wave):
    // one part, one plan, and the sums run over exactly the windows that live in the partial sums
    if (a.n_parts != 1 || a.dual || ra.n_value_parts != n_windows || ra.chunks_per_part != n_windows || ra.n_parts != n_windows) {
        h->err = "lag statistics: the reduction's windows do not match the head's plan";
        return SSDE_ERR_ARG;
    }
    LagFormOut o;
    const int mask = order >= 1 ? a.part_mask[0] : 0;
    const int ci = cut < LAG_A ? lag_cut_index(cut) : -1;
    if (cut < LAG_A && (ci < 0 || !((h->lag_cut_mask >> ci) & 1u) || h->model != SSDE_MODEL_CTCRW || K >= cut)) {
        h->err = "lag statistics: no statistics for the evaluation's cut";
        return SSDE_ERR_ARG;
    }
    if (h->model == SSDE_MODEL_CTCRW) {
        LagFormArgs f;
        lag_form_taps(a, h->d, mask, K, f);
        f.M = h->lag_M_host.data(); f.s = h->lag_s_host.data(); f.n = h->lag_n;
        if (ci >= 0) { f.M = h->lag_cut_M_host[ci].data(); f.s = h->lag_cut_s_host[ci].data(); f.n = h->lag_cut_n[ci]; }
        lag_forms_host(f, o);
    } else {
        LagScalArgs f;
        lag_form_taps_scal(h->model, a, h->d, mask, K, h->lag_ref, f);
        f.M = h->lag_M_host.data(); f.s = h->lag_s_host.data(); f.n = h->lag_n;
        lag_forms_scal_host(f, o);
    }
    ra.lag_part = n_windows;
    for (int k = 0; k < NACC_MAX; k++) ra.lag_acc[k] = o.acc[k];
    ra.lag_chk = o.chk;
    return SSDE_OK;
}

// The reduction's arguments: which accumulator of which part feeds which output slot (needed BEFORE the main launch when the
// finalising work is fused into it).  Reads the handle's layout and the launch's arguments, writes ra.
void fill_reduce_args(const ssde_handle* h, const IsoArgs& a, int order, const double add[4], ReduceArgs& ra) {
    const ParLayout& L = h->L;
    for (int i = 0; i < 4; i++) { ra.add[i] = add[i]; ra.add_slot[i] = -1; }
    if (h->use_shared) {
        ra.add_slot[0] = 0;
        if (order >= 1) {
            const int pj[NDIRP] = {0, L.off_fe + L.fe_off[h->d], h->q > h->d + 1 ? L.off_fe + L.fe_off[h->d + 1] : 0};
            for (int j = 0; j < NDIRP; j++)
                if (pj[j] < L.n_full && !h->fixed[pj[j]] && (j < 2 || h->q > h->d + 1)) ra.add_slot[1 + j] = (int16_t)(1 + pj[j]);
        }
    }
    const int nacc = h->cv_adj ? adj_nacc(h->model, h->d, h->n_stream_cols, a.cv_mu_cols != 0)
                   : h->drift == 3 ? 2 + CV_KC + h->d : 4 + h->d + (h->drift ? h->n_stream_cols : 0);
    const int ncr = (a.dual && a.n_chunks_d > a.n_chunks) ? a.n_chunks_d : a.n_chunks;     // windows the final sums run over
    ra.n_parts = a.n_parts * ncr; ra.nacc = nacc; ra.n_blocks = h->n_groups;
    ra.n_value_parts = ncr; ra.chunks_per_part = ncr;
    ra.chk = h->chk.p; ra.n_chk = a.n_chunks > 1 ? a.n_parts * (a.n_chunks - 1) * h->n_groups : 0;
    // (the bulk's forms are one more window, by value: lag_forms_into)
    if (order >= 1 && h->cv_adj) {
        // accumulators of k_iso_adj.hip: [value | log sigma_obs | mu_a | par[d] | par[d + 1] | per streamed column: par[d], par[d + 1] (, mu_a)]
        const int nkp = h->model == SSDE_MODEL_BM_SSM ? 1 : 2, nk = adj_nk(h->model, h->d, a.cv_mu_cols != 0);
        if (!h->fixed[0] && !h->has_h) ra.map[0] = 1;
        for (auto& sl : h->slots) {
            if (h->fixed[sl.pidx]) continue;
            const int kind = sl.par_j < h->d ? nkp + sl.par_j : sl.par_j - h->d;
            const int k = sl.col >= 0 ? 4 + h->d + sl.col * nk + kind : (sl.par_j < h->d ? 2 + sl.par_j : 2 + h->d + (sl.par_j - h->d));
            ra.map[k - 1] = (int16_t)(1 + sl.pidx);
        }
    } else
    if (order >= 1 && h->drift == 3) {
        // accumulators of k_iso_colvar.hip, per part: [value | the part's columns | mu_1 .. mu_d | log sigma_obs]
        for (int p = 0; p < CV_WAVES; p++) {
            for (int k = 0; k < CV_KC; k++) {
                const int pidx = h->cv_pidx[(size_t)p * CV_KC + k];
                if (pidx >= 0) ra.map[p * (nacc - 1) + k] = (int16_t)(1 + pidx);
            }
            if (p == h->cv_mu_part)
                for (auto& sl : h->slots)
                    if (sl.par_j < h->d && sl.col < 0 && !h->fixed[sl.pidx]) ra.map[p * (nacc - 1) + CV_KC + sl.par_j] = (int16_t)(1 + sl.pidx);
            if (p == h->cv_sig_part) ra.map[p * (nacc - 1) + CV_KC + h->d] = 1;
        }
    } else
    if (order >= 1 && h->drift) {
        // accumulators of k_iso_drift.hip: [value | sigma_obs | mu intercepts | par d | par d+1 | streamed columns]
        if (!h->fixed[0]) ra.map[0] = 1;
        for (auto& sl : h->slots) {
            if (h->fixed[sl.pidx]) continue;
            const int k = sl.col >= 0 ? 4 + h->d + sl.col : (sl.par_j < h->d ? 2 + sl.par_j : sl.par_j == h->d ? 2 + h->d : 3 + h->d);
            ra.map[k - 1] = (int16_t)(1 + sl.pidx);
        }
    } else
    if (order >= 1) {
        for (int p = 0; p < a.n_parts; p++)
            for (int k = 1; k < nacc; k++) {
                // accumulators are ordered like the constant-coefficient parameter vector: sigma_obs, one per SDE parameter
                const int j = k - 2;     // SDE parameter of accumulator k (k == 1: log_sigma_obs)
                if (j >= h->q) continue;
                const int pidx = j < 0 ? 0 : L.off_fe + L.fe_off[j];
                if (pidx < L.n_full && !h->fixed[pidx]) ra.map[p * (nacc - 1) + (k - 1)] = (int16_t)(1 + pidx);
            }
    }
}

}  // namespace

namespace ssde_engine {

int eval_iso(ssde_handle* h, const double* par, int order, double* out_dev, hipStream_t s, ReduceArgs& ra) {
    const ParLayout& L = h->L;
    IsoArgs a;
    memset(&a, 0, sizeof(a));
    h->last_lag_rows = 0; h->last_lag_cut = 0;
    a.tv.tiles = h->tiles.p; a.tv.group_off = h->group_off.p; a.tv.group_len = h->group_len.p;
    a.tv.lane_nsteps = h->lane_nsteps.p; a.tv.a0 = h->a0.p; a.tv.n_groups = h->n_groups; a.tv.C = h->C; a.tv.c_obs = h->c_obs; a.tv.dt_all = h->dt_all;
    a.partials = h->partials.p;
    if (order >= 1) {
        a.n_parts = h->iso_parts;
        for (int p = 0; p < MAX_PARTS; p++) a.part_mask[p] = h->iso_masks[p];
    } else {
        a.n_parts = 1;
    }
    if (h->drift == 3) { a.n_parts = h->cv_adj ? 1 : h->cv_few ? h->cv_kc / CV_KC : h->cv_single ? 1 : CV_WAVES; a.part_mask[0] = order >= 1 ? 1 : 0; }    // k_iso_colvar.hip: the parts are the waves of a workgroup
    a.any_nan = h->na_any;
    a.uniform_dt = h->uniform_dt ? 1 : 0;
    const double sig = exp(par[0]);                     // nllk_ctcrw.hpp:136
    a.h = sig * sig;                                    // makeH: sigma_obs * sigma_obs
    for (int i = 0; i < h->d; i++) a.mu[i] = par[L.off_fe + L.fe_off[i]];
    for (int i = 0; i < 3; i++) a.p0[i] = h->p0_iso[i];
    if (h->drift == 3) {
        // p_j(i) = intercept_j + sum_k coef_k X_k(i) for the rows of par[d] and par[d + 1] (nllk_ctcrw.hpp:143-156); and the range
        // each can reach on this design (column ranges found at create), for the window plan
        for (int j = 0; j < 2; j++) h->cv_eta_lo[j] = h->cv_eta_hi[j] = 0.0;
        // (a drift with a fixed-effect design of its own -- mu ~ 1 + x -- has NO intercept slot: its column of ones is a streamed
        // column like the others, and the constant part of mu_a is zero)
        for (int i = 0; i < h->d; i++) a.mu[i] = 0.0;
        for (auto& sl : h->slots) {
            const int j = sl.par_j - h->d;
            if (j < 0) {                                        // a design column of the drift: mu_a(i) = intercept + sum_k coef_k X_k(i)
                if (sl.col >= 0) { (sl.par_j == 0 ? a.coefC : a.coefD)[sl.col] = par[sl.pidx]; a.cv_mu_cols = 1; }
                else a.mu[sl.par_j] = par[sl.pidx];
                continue;
            }
            const double b = par[sl.pidx];
            if (sl.col < 0) { a.cv_eta0[j] = b; h->cv_eta_lo[j] += b; h->cv_eta_hi[j] += b; continue; }
            (j == 0 ? a.coefA : a.coefB)[sl.col] = b;
            const double lo = h->cv_col_lo[sl.col], hi = h->cv_col_hi[sl.col];
            h->cv_eta_lo[j] += std::min(b * lo, b * hi);
            h->cv_eta_hi[j] += std::max(b * lo, b * hi);
        }
        a.drift_k = h->n_stream_cols; a.c_col = h->c_obs + h->d + (h->has_h ? h->d * h->d : 0);
        a.cv_full = h->cv_full ? 1 : 0; a.cv_has_h = h->has_h ? 1 : 0;
        for (int i = 0; i < 16; i++) a.cv_p0[i] = h->p0_full[i];
        if (h->has_h) a.h = h->cv_hmax;                         // (the window planner's observation variance; the lanes read H_array[,,i])
        // ... which is loose (a partition-of-unity basis reaches max |coef|, the bound says sum |coef|): once a launch has run,
        // the range it actually saw, widened by a quarter of its width (+ 0.05), bounds the plan; a parameter jump that leaves
        // it fails the hand-over check and the retry plans from that evaluation's own range
        if (h->cv_ranges_pinned)
            for (int j = 0; j < 2; j++) {
                const double lo = h->cv_ranges_pinned[2 * j], hi = h->cv_ranges_pinned[2 * j + 1];
                if (!(lo <= hi) || !std::isfinite(lo) || !std::isfinite(hi)) continue;
                const double m = 0.25 * (hi - lo) + 0.05;
                h->cv_eta_lo[j] = std::max(h->cv_eta_lo[j], lo - m);
                h->cv_eta_hi[j] = std::min(h->cv_eta_hi[j], hi + m);
                if (h->cv_eta_lo[j] > h->cv_eta_hi[j]) { h->cv_eta_lo[j] = lo - m; h->cv_eta_hi[j] = hi + m; }
            }
    } else
    if (h->drift) {
        // mu_a(i) = intercept + sum_k coef_k X_k(i) (nllk_ctcrw.hpp:143-149): the intercept slot (if any) goes where the
        // constant-drift kernels keep mu, the streamed columns get their coefficients by the dimension they feed
        for (int i = 0; i < h->d; i++) a.mu[i] = 0.0;
        for (auto& sl : h->slots) {
            if (sl.col < 0) { if (sl.par_j < h->d) a.mu[sl.par_j] = par[sl.pidx]; continue; }
            if (sl.par_j == 0) a.coefA[sl.col] = par[sl.pidx];
            else { a.coefB[sl.col] = par[sl.pidx]; a.drift_dim1 |= 1u << sl.col; }
        }
        a.drift_k = h->n_stream_cols; a.c_col = h->c_obs + h->d;
        a.pp = h->pp_drift;
    }
    const double p1 = par[L.off_fe + L.fe_off[h->d]];
    const double p2 = (h->q > h->d + 1) ? par[L.off_fe + L.fe_off[h->d + 1]] : 0.0;
    if (h->model == SSDE_MODEL_CTCRW) {
        a.tau = exp(p1);                                // :153
        const double nu = exp(p2);                      // :154
        a.beta = 1.0 / a.tau;                           // :155
        a.sigma = 2.0 * nu / sqrt(M_PI * a.tau);        // :156
        if (h->uniform_dt) ctcrw_trans(h->dt_uniform, a.tau, a.beta, a.sigma, a.ctr);
    } else if (h->model == SSDE_MODEL_OU_SSM) {
        a.tau = exp(p1);
        a.sigma = exp(p2);                              // kappa
        if (h->uniform_dt) ou_trans(h->dt_uniform, a.tau, a.sigma, a.str);
    } else {
        a.sigma = exp(p1);
        if (h->uniform_dt) bm_trans(h->dt_uniform, a.sigma, a.str);
    }
    auto tick = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tk0 = h->knobs.trace ? tick() : 0.0;
    // ---- the plan (ssde_windows.hpp): from what create found, this evaluation's parameters and the policy's boost
    const WindowPolicy& policy = h->policy();
    const WindowFacts wf = window_facts(h);
    const WindowParams wp = {a.tau, a.beta, a.sigma, a.h, {a.p0[0], a.p0[1], a.p0[2]}};
    const WindowPlan plan = plan_windows(wf, WINDOW_CONSTS, wp, policy.boost());
    if (h->knobs.trace) { const double t = tick(); h->trace_us[0] += t - tk0; tk0 = t; }
    a.bnd = h->bnd.p; a.chk = h->chk.p;
    a.bnd_stride = h->drift ? std::max(NSTATE_MAX, h->drift_nstate) : NSTATE_MAX;
    a.chk_out = out_dev + (1 + L.n_full);
    a.derive = (h->knobs.no_derive || h->drift) ? 0 : 1;
    a.stream_nt = h->stream_nt ? 1 : 0;
    a.all_clean = ((h->use_shared && h->n_clean_groups == h->n_groups) || h->drift) ? 1 : 0;      // (drift: one dump layout for every group)
    // (the reverse sweep's records hold the state AND its adjoint; a value-only evaluation writes the states alone -- iso_adj_kernel,
    //  !grad -- and is checked on them alone: the adjoint halves are whatever an earlier evaluation, or a failed attempt of one, left)
    a.nstate_clean = h->drift ? (h->drift == 3 && h->cv_adj && order < 1 ? h->drift_nstate / 2 : h->drift_nstate)
                   : h->use_shared ? shared_nstate(h->sdim, order >= 1 ? a.part_mask[0] : 0, h->model != SSDE_MODEL_BM_SSM) : 0;
    a.group_flags = h->group_flags.p;
    a.group_mode = 0;
    double add[4] = {0, 0, 0, 0};
    if (!h->use_shared && h->quiet_ok) {
        int st = (h->d == 1) ? build_gain_table<1>(h, a, h->iso_free_mask, s, add) : build_gain_table<2>(h, a, h->iso_free_mask, s, add);
        if (st) return st;
        a.gain = nullptr;
        for (double& v : add) v = 0.0;
    }
    // (only the head of the lag-statistics path launches the wg entry: window_geometry, head_latency_plan)
    const bool gain_deferred = h->use_shared && h->lag_ready && !h->drift && !h->knobs.fused_finalize;
    if (h->use_shared) {
        int st = (h->d == 1) ? build_gain_table<1>(h, a, h->iso_free_mask, s, add, gain_deferred)
                             : build_gain_table<2>(h, a, h->iso_free_mask, s, add, gain_deferred);
        if (st) return st;
        if (h->knobs.trace) { const double t = tick(); h->trace_us[1] += t - tk0; tk0 = t; }
        a.group_mode = 3;
    }
    // ---- the geometry that follows the plan: the transient window, the balance of window 0, the mixed batch's second plan, the
    // lag-statistics cut and the quiet rows' memory
    WindowEval we;
    we.n_parts = a.n_parts; we.hess_req = h->hess_req;
    we.can_derive = order >= 1 && a.derive && (a.part_mask[0] & DIR_SIG) && (a.part_mask[0] & (h->model == SSDE_MODEL_BM_SSM ? DIR_P1 : DIR_P2));
    we.gain_last = a.gain_last; we.gain_usable = h->gain_stationary && a.gain_stat[0] != 0.0;
    const WindowGeometry g = window_geometry(wf, WINDOW_CONSTS, wp, plan, policy.boost(), policy.gave_up, we);
    const int lag_K = g.lag_K;
    // the bulk cut at the transient's end (head_early_cut): the head is window 0 alone -- one window from row 0 over tracks capped at the cut
    const int lag_cut = lag_K > 0 ? g.lag_cut : 0;
    const bool early = lag_K > 0 && lag_cut < LAG_A;
    h->plan_warmup = g.plan.warmup; h->plan_rho = g.plan.rho;
    a.n_chunks = g.n_chunks; a.window = g.window; a.t0 = g.t0; a.t0_delta = g.t0_delta;
    if (early) { a.n_chunks = 1; a.t0 = 0; a.t0_delta = 0; }          // (window stays the warm-up in force -- the forms' K: one window reads none, ssde_info reports it)
    h->last_chunks = a.n_chunks; h->last_window = a.window; h->last_t0 = a.t0; h->last_t0_delta = a.t0_delta;
    h->last_quiet_window = g.quiet_window;
    if (early) {
        const int ci = lag_cut_index(lag_cut);
        a.tv.group_len = h->lag_cut_glen[ci].p; a.tv.lane_nsteps = h->lag_cut_ns[ci].p;
        h->last_lag_rows = h->lag_cut_rows[ci];
    } else
    if (lag_K > 0) {                         // the head: every track capped at LAG_A rows
        a.tv.group_len = h->lag_glen.p; a.tv.lane_nsteps = h->lag_ns.p;
        h->last_lag_rows = h->lag_rows;
    }
    h->last_lag_cut = lag_cut;
    if (g.quiet_window > 0) {
        a.nan_bits = h->nan_bits.p; a.nan_words = h->nan_words; a.quiet_flag = h->quiet_flag.p;
        a.quiet_w = g.quiet_w; a.quiet_b0 = g.quiet_b0;
        for (int i = 0; i < 12; i++) a.quiet_p[i] = h->stat_p[i];
        a.quiet_ld = h->stat_ld;
        for (int j = 0; j < NDIRP; j++) a.quiet_gld[j] = h->stat_gld[j];
    }
    // The finalising work inside the main launch (fused_finalize_wave, ssde_device.hpp): the shared-covariance kernel alone on the
    // batch (no group on the general kernel, no drift columns); SSDE_FUSED_FINALIZE=0: the two-launch form (A/B -- bitwise the same)
    const bool shared_alone = h->use_shared && !h->drift && h->n_clean_groups == h->n_groups && !h->hess_req;
    const bool fused = shared_alone && h->fuse_words.p && h->knobs.fused_finalize.value_or(false);
    // One workgroup per track group (iso_shared_wg_kernel): the latency plan's geometry -- the transient window on a wave of its own --
    // with exactly a workgroup's worth of windows.  The hand-overs are checked in LDS; a synchronous single-engine call has the records
    // sent to its mailbox and forms the result on the host (run_once), every other caller gets them in device memory and a finalize
    // launch without check workgroups.  SSDE_FUSED_FINALIZE unset: this form; = 0: the two-launch form on iso_shared_kernel (A/B).
    static_assert(HEAD_WG_WAVES == WG_WAVES, "the plan credits the windows of one workgroup");
    static_assert(HEAD_GROW == GAIN_ROW && HEAD_C == LAG_CUT_MAX && 4 + 2 <= NACC_MAX, "the head's forms read the gain table's rows and cover every early cut");
    // The bulk cut at the transient's end: window 0 alone, its direction parts on the waves of the group's workgroup
    // (iso_shared_cut_kernel) -- the same record, the same two ways out.  SSDE_FUSED_FINALIZE=0 / =1: the single wave of iso_shared_kernel
    // on that window (A/B -- bitwise the same).
    // (d = 2 only: with one response coordinate the parts' value is NOT the single wave's bits -- 4 ulp on a one-track batch, cause not
    //  found.  A d = 1 handle has the option off by default and keeps the late cut with its one-workgroup head; set by hand, its early
    //  cut runs the single wave of iso_shared_kernel and a finalize launch: the tests' form, slower than the late cut's head)
    const bool cut_wg = early && shared_alone && !h->knobs.fused_finalize && a.n_parts == 1 && h->model == SSDE_MODEL_CTCRW && h->d == 2;
    const bool wg = cut_wg || (shared_alone && !h->knobs.fused_finalize && a.n_parts == 1 && a.t0 > 0 && a.t0_delta == 0 && a.n_chunks == WG_WAVES);
    const bool host_finish = wg && h->host_finish_ok && h->mbx_pinned;
    h->last_cut_parts = cut_wg ? cut_n_parts(order >= 1 ? a.part_mask[0] : 0) : 0;
    if (wg) {
        a.wg_form = cut_wg ? 2 : 1;
        if (host_finish) { a.mbx = h->mbx_pinned; a.mbx_seq = ++h->mbx_seq; }
    }
    bool head_form = false;                             // the head came from its statistics: nothing was launched
    HeadGain gv;
    gv.rows = 0;
    HeadLead lead = {nullptr, 0, 0};
    if (cut_wg) { lead.ns_min = h->lag_cut_nsmin[lag_cut_index(lag_cut)].p; lead.lead_stride = h->lag_lead_stride; lead.lead_n = h->lag_lead_n; }
    if (gain_deferred) {
        const int st = feed_gain_table(h, a, wg, s, gv);
        if (st) return st;
        if (h->knobs.trace) { const double t = tick(); h->trace_us[1] += t - tk0; tk0 = t; }
    }
    h->last_gain_feed = gv.rows > 0 ? 1 : 0;
    if (h->use_shared) {
        // two independent launches (NaN-free groups on the shared-covariance kernel, NaN-carrying groups on
        // the general kernel): fork onto a side stream so they share the chip, join before the hand-over check
        const bool any_dirty = h->n_clean_groups < h->n_groups;
        IsoArgs ad = a;                      // the general launch: this plan, or -- mixed batch -- one of its own
        if (g.dual) {
            ad.n_chunks = g.n_chunks_d; ad.t0 = g.t0_d; ad.t0_delta = 0;
            a.dual = 1; a.n_chunks_d = ad.n_chunks; a.window_d = ad.window; a.t0_d = ad.t0; a.t0_delta_d = ad.t0_delta;
            a.dirty_groups = h->dirty_groups.p; a.n_dirty_groups = h->n_dirty_groups;
            ad.dirty_groups = h->dirty_groups.p; ad.n_dirty_groups = h->n_dirty_groups; ad.use_group_list = 1;
            // the final sums run over the longer of the two plans: the slots the shorter one does not write must be zero
            HIPCHK(h, hipMemsetAsync(h->partials.p, 0, (size_t)std::max(a.n_chunks, ad.n_chunks) * (4 + h->d) * h->n_groups * 8, s));
        }
        IsoArgs b = a;
        b.group_mode = 2;
        if (h->knobs.wave_clock) {
            const int items = ((h->n_groups + 7) / 8 * 8) * (cut_wg ? WG_WAVES : a.n_chunks) + 8;
            if ((int)h->wave_clock.n < 4 * items) { h->wave_clock.release(); HIPCHK(h, h->wave_clock.alloc((size_t)4 * items)); }
            HIPCHK(h, hipMemsetAsync(h->wave_clock.p, 0, (size_t)4 * items * 8, s));
            b.wave_clock = h->wave_clock.p; h->wave_clock_items = items;
        }
        if (any_dirty) {
            HIPCHK(h, hipEventRecord(h->ev_fork, s));
            HIPCHK(h, hipStreamWaitEvent(h->aux[1], h->ev_fork, 0));
            HIPCHK(h, launch_iso(h->model, h->d, ad, true, h->aux[1]));
            HIPCHK(h, hipEventRecord(h->ev_join[1], h->aux[1]));
        }
        if (h->drift && h->hess_req) {
            // ssde_hess on a drift handle: the same plan, the same gains, the Hessian kernels instead of the evaluation
            h->hess_req = false;
            DriftHessArgs hx = h->hess_args;
            HIPCHK(h, launch_iso_drift_hess(h->model, b, hx, h->hess_tiles, s));
            return SSDE_OK;
        }
        if (h->drift) HIPCHK(h, launch_iso_drift(h->model, h->d, b, s, h->stamps ? h->ev_k0 : nullptr, h->stamps ? h->ev_k1 : nullptr));
        else {
            if (fused) {
                fill_reduce_args(h, a, order, add, ra);
                ra.kfast = 1;
                b.fused = 1;
                b.fuse_arrive = h->fuse_words.p + 4; b.fuse_done = h->fuse_words.p;
                b.chk_out = (double*)(h->fuse_words.p + 2);         // (its own word, zero between launches: the last wave moves it to out[n_out])
            }
            // the bulk's forms, on the host: the single launch of the fused form needs them; the two-launch form computes them
            // while the head runs (below), for its finalize launch
            if (lag_K > 0 && fused) { const int st = lag_forms_into(h, a, order, lag_K, a.n_chunks, ra, lag_cut); if (st) return st; }
            // The head from its Gram statistics (ssde_headforms.hpp): the synchronous single-engine call whose head would be the cut's
            // workgroups finished on the host forms the same 4 + d accumulators here instead and launches nothing.  They stand in
            // group 0's place of the reduction's order, the other groups' entries are zero.  (A table row that is not scored keeps
            // the kernel; so does every other caller: ssde_eval_device, stamps, shards, a communicator, the wave clock.)
            if (cut_wg && host_finish && h->head_ready && h->head_host && gain_deferred && lag_cut <= HEAD_C && !h->knobs.wave_clock && h->d == 2) {
                const double th0 = h->knobs.trace ? tick() : 0.0;
                HeadFormArgs hf;
                hf.G = h->head_G_host.data(); hf.s = h->head_s_host.data(); hf.n = h->head_n; hf.cut = lag_cut; hf.d = h->d;
                hf.mask = order >= 1 ? a.part_mask[0] : 0;
                hf.gain = h->gain_scratch.data(); hf.gain_last = a.gain_last; hf.tr = a.ctr;
                hf.mu[0] = a.mu[0]; hf.mu[1] = a.mu[1]; hf.full_probes = false;
                HeadFormOut ho;
                if (head_forms_host(hf, *h->head_work, ho)) {
                    for (int k = 0; k < NACC_MAX; k++) h->head_rec[k] = k < 4 + h->d ? ho.acc[k] : 0.0;
                    head_form = true;
                }
                if (h->knobs.trace) { const double t = tick(); h->trace_us[5] += t - th0; tk0 += t - th0; }
            }
            if (!head_form)
            HIPCHK(h, launch_iso_shared(h->model, h->d, b, ra, s, h->stamps ? h->ev_k0 : nullptr, h->stamps ? h->ev_k1 : nullptr,
                                        gv.rows > 0 ? &gv : nullptr, cut_wg ? &lead : nullptr));
        }
        h->last_kernel_id = h->drift ? SSDE_KERNEL_ISO_DRIFT : any_dirty ? SSDE_KERNEL_ISO_MIXED : SSDE_KERNEL_ISO_SHARED;
        h->ev_k_valid = h->stamps;
        h->last_s_stat = h->drift ? -1 : g.s_stat;
        if (any_dirty) HIPCHK(h, hipStreamWaitEvent(s, h->ev_join[1], 0));
    } else {
        if (h->stamps) HIPCHK(h, hipEventRecord(h->ev_k0, s));
        if (h->drift == 3) {
            a.t0 = 0; a.t0_delta = 0;
            if (h->knobs.wave_clock) {                  // (a build with -DSSDE_CV_CLOCK fills it: cycles per row and phase of every wave)
                const int items = h->n_groups * a.n_chunks * CV_WAVES;
                if ((int)h->wave_clock.n < 4 * items) { h->wave_clock.release(); HIPCHK(h, h->wave_clock.alloc((size_t)4 * items)); }
                HIPCHK(h, hipMemsetAsync(h->wave_clock.p, 0, (size_t)4 * items * 8, s));
                a.wave_clock = h->wave_clock.p; h->wave_clock_items = items;
            }
            h->last_kernel_id = h->cv_adj ? SSDE_KERNEL_ISO_ADJ : h->cv_single ? SSDE_KERNEL_ISO_FULL : h->cv_few ? SSDE_KERNEL_ISO_FEW : SSDE_KERNEL_ISO_COLVAR;
            if (h->cv_adj) {
                // checkpoints: the state entering every CB-th row from a window's first scored row to where its backward recursion starts
                const int items = adj_items(h->n_groups, a.n_chunks), cb = adj_ckpt_rows(h->model, h->d, h->cv_full), nst = adj_nstate(h->model, h->d, h->cv_full) / 2;
                const int units = (h->glen_max + WIN_ALIGN - 1) / WIN_ALIGN;
                a.adj_tail = a.window;
                a.adj_diag = h->knobs.adj_diag;
                if (h->knobs.adj_tail) a.adj_tail = (int)std::min<int64_t>((int64_t)*h->knobs.adj_tail * policy.boost(), h->glen_max);      // (testing)
                const int len = (units / a.n_chunks + 1) * WIN_ALIGN + (a.n_chunks > 1 ? a.adj_tail : 0);
                a.adj_ckpt_stride = (int64_t)((len + cb - 1) / cb + 1) * nst * WAVE;
                const size_t need = order >= 1 ? (size_t)items * (size_t)a.adj_ckpt_stride : (size_t)WAVE;
                if (h->adj_ckpt.n < need) { h->adj_ckpt.release(); HIPCHK(h, h->adj_ckpt.alloc(need)); }
                a.adj_ckpt = h->adj_ckpt.p;
                if ((int)h->cv_ranges.n < 4 * items) { h->cv_ranges.release(); HIPCHK(h, h->cv_ranges.alloc((size_t)4 * items)); }
                a.cv_ranges = h->cv_ranges.p;
                HIPCHK(h, launch_iso_adj(h->model, h->d, a, s));
                HIPCHK(h, launch_colvar_range_reduce(h->cv_ranges.p, items, h->cv_ranges_pinned, s));
            } else
            if (h->cv_single) HIPCHK(h, launch_iso_full(h->model, a, h->cv_parts.p, s));
            else if (h->cv_few) HIPCHK(h, launch_iso_few(h->model, h->d, a, h->cv_parts.p, h->cv_kc, s));
            else {
            const int n_wg = h->n_groups * a.n_chunks;
            if ((int)h->cv_ranges.n < 4 * n_wg) { h->cv_ranges.release(); HIPCHK(h, h->cv_ranges.alloc((size_t)4 * n_wg)); }
            a.cv_ranges = h->cv_ranges.p;
            HIPCHK(h, launch_iso_colvar(h->model, h->d, a, h->cv_parts.p, h->cv_kc, s));
            HIPCHK(h, launch_colvar_range_reduce(h->cv_ranges.p, n_wg, h->cv_ranges_pinned, s));
            }
        }
        else if (h->drift) { a.t0 = 0; a.t0_delta = 0; HIPCHK(h, launch_iso_drift_general(h->model, h->d, a, s)); h->last_kernel_id = SSDE_KERNEL_ISO_DRIFT_GEN; }
        else {
            HIPCHK(h, launch_iso(h->model, h->d, a, false, s));
            h->last_kernel_id = a.n_parts > 1 ? SSDE_KERNEL_ISO_SPLIT : a.quiet_w > 0 ? SSDE_KERNEL_ISO_QUIET
                              : a.uniform_dt ? SSDE_KERNEL_ISO_MASK_UNI : SSDE_KERNEL_ISO_MASK;
        }
        if (h->stamps) HIPCHK(h, hipEventRecord(h->ev_k1, s));
        h->ev_k_valid = h->stamps;
        h->last_s_stat = -1;
    }
    if (h->knobs.trace) { const double t = tick(); h->trace_us[2] += t - tk0; tk0 = t; }
    if (!fused) fill_reduce_args(h, a, order, add, ra);
    if (wg) ra.n_chk = h->n_groups;                     // (one check per group, from the main launch)
    if (!fused && lag_K > 0) { const int st = lag_forms_into(h, a, order, lag_K, a.n_chunks, ra, lag_cut); if (st) return st; }     // (the head is running: this overlaps it)
    // the hand-over checks and the final sums in one launch (unless the main launch has done them)
    if (host_finish) { h->host_ra = ra; h->host_armed = !head_form; h->head_armed = head_form; }      // (run_once: the spin on the mailbox -- none where the head came from its statistics -- and reduce_host)
    else if (!fused) HIPCHK(h, launch_iso_finalize(h->model, h->d, a, ra, s));
    h->last_finish_form = host_finish ? 2 : fused ? 1 : 0;
    h->last_head_form = head_form ? 1 : 0;
    if (h->knobs.trace) {
        const double t = tick(); h->trace_us[3] += t - tk0; h->trace_n++;
        if (h->trace_skip < 8) {                        // the first calls load code objects: not what is being measured
            h->trace_skip++;
            for (double& v : h->trace_us) v = 0.0;
            h->trace_n = 0;
        }
    }
    return SSDE_OK;
}

}  // namespace ssde_engine

extern "C" int ssde_reduce_host(const double* sums, const double* group_chk, int32_t n_groups, int32_t n_windows, int32_t nacc,
                                const double* lag_acc, double lag_chk, const double* add, const int16_t* add_slot, const int16_t* map,
                                int32_t n_out, double* out) {
    if (!sums || !group_chk || !add || !add_slot || !map || !out || n_groups < 1 || n_windows < 1 || nacc < 1 || n_out < 1) return SSDE_ERR_ARG;
    for (int k = 0; k + 1 < nacc; k++) if (map[k] >= n_out) return SSDE_ERR_ARG;
    for (int i = 0; i < 4; i++) if (add_slot[i] >= n_out) return SSDE_ERR_ARG;
    const ReduceHostArgs a = {sums, (int64_t)n_windows * nacc, group_chk, 1, n_groups, n_windows, nacc, lag_acc, lag_chk, add, add_slot, map, n_out};
    std::vector<double> scratch;
    reduce_host(a, out, scratch);
    return SSDE_OK;
}

extern "C" int ssde_reduce_host_head(const double* sums0, double chk0, int32_t n_groups, int32_t n_windows, int32_t nacc,
                                     const double* lag_acc, double lag_chk, const double* add, const int16_t* add_slot,
                                     const int16_t* map, int32_t n_out, double* out) {
    if (!sums0 || !add || !add_slot || !map || !out || n_groups < 1 || n_windows < 1 || n_windows > REDUCE_HEAD_MAX_WINDOWS || nacc < 1 || n_out < 1) return SSDE_ERR_ARG;
    for (int k = 0; k + 1 < nacc; k++) if (map[k] >= n_out) return SSDE_ERR_ARG;
    for (int i = 0; i < 4; i++) if (add_slot[i] >= n_out) return SSDE_ERR_ARG;
    const ReduceHostArgs a = {sums0, (int64_t)n_windows * nacc, &chk0, 1, n_groups, n_windows, nacc, lag_acc, lag_chk, add, add_slot, map, n_out};
    return reduce_host_head(a, out) ? SSDE_OK : SSDE_ERR_ARG;
}

extern "C" int ssde_last_finish_form(const ssde_handle* h) {
    if (!h) return -1;
    return h->shards.empty() ? h->last_finish_form : h->shards[0]->last_finish_form;
}

extern "C" int ssde_last_head_form(const ssde_handle* h) {
    if (!h) return -1;
    return h->shards.empty() ? h->last_head_form : h->shards[0]->last_head_form;
}

extern "C" int ssde_headforms_host(const double* G, const double* s, double n_tracks, int32_t d, const double* theta, double dt,
                                   const double* p0, int32_t cut, int32_t mask, int32_t full_probes, double* acc, double* gain_out,
                                   double* trans_out, int32_t* n_probe) {
    if (!G || !s || !theta || !acc || d != 2 || cut < 1 || cut > HEAD_C || !(dt > 0.0) || !std::isfinite(dt)) return SSDE_ERR_ARG;
    const double sig = exp(theta[0]);
    const double h_obs = sig * sig, tau = exp(theta[1 + d]), nu = exp(theta[2 + d]);
    CtcrwTrans tr;
    ctcrw_trans(dt, tau, 1.0 / tau, 2.0 * nu / sqrt(M_PI * tau), tr);
    // the gain table: the covariance half of the filter until it has stopped moving (as build_gain_table), at most the head's rows
    std::vector<double> gain;
    CtcrwCov<15> C;
    if (p0) C.init(p0[0], p0[1], p0[2]); else C.init(1.0, 0.0, 1.0);
    int last = 0, stable = 0;
    for (int t = 0; t < HEAD_C && stable < GAIN_SETTLED_ROWS; t++) {
        const CtcrwCov<15> prev = C;
        CtcrwGain g;
        ctcrw_cov_step<2, 15>(C, tr, h_obs, false, g);
        double r[HEAD_GROW] = {g.iF, g.k1, g.k2, g.bm};
        for (int j = 0; j < NDIRP; j++) { r[4 + j] = g.diF[j]; r[7 + j] = g.dk1[j]; r[10 + j] = g.dk2[j]; }
        gain.insert(gain.end(), r, r + HEAD_GROW);
        last = t;
        stable = ctcrw_cov_settled(C, prev) ? stable + 1 : 0;
    }
    std::vector<double> Gp((size_t)HEAD_LDW * HEAD_LDW), sp(2 * HEAD_LDW);
    head_pad_stats(G, s, Gp.data(), sp.data());
    HeadFormArgs hf;
    hf.G = Gp.data(); hf.s = sp.data(); hf.n = n_tracks; hf.cut = cut; hf.d = d;
    hf.mask = mask < 0 ? (DIR_SIG | DIR_MU | DIR_P1 | DIR_P2) : mask;
    hf.gain = gain.data(); hf.gain_last = last; hf.tr = tr; hf.mu[0] = theta[1]; hf.mu[1] = theta[2]; hf.full_probes = full_probes != 0;
    std::vector<HeadFormWork> work(1);
    HeadFormOut ho;
    if (!head_forms_host(hf, work[0], ho)) return SSDE_ERR_ARG;      // (a row that is not scored: such an evaluation keeps the kernel)
    for (int k = 0; k < 4 + d; k++) acc[k] = ho.acc[k];
    if (gain_out)
        for (int t = 0; t < cut; t++)
            for (int k = 0; k < HEAD_GROW; k++) gain_out[(size_t)t * HEAD_GROW + k] = gain[(size_t)(t < last ? t : last) * HEAD_GROW + k];
    if (trans_out) { trans_out[0] = tr.e; trans_out[1] = tr.t12; trans_out[2] = tr.b1; trans_out[3] = tr.b2; trans_out[4] = tr.de; trans_out[5] = tr.dt12; }
    if (n_probe) *n_probe = ho.n_full;
    return SSDE_OK;
}

extern "C" int ssde_last_gain_feed(const ssde_handle* h) {
    if (!h) return -1;
    return h->shards.empty() ? h->last_gain_feed : h->shards[0]->last_gain_feed;
}

extern "C" int ssde_last_gain_rows(const ssde_handle* h) {
    if (!h) return -1;
    return h->shards.empty() ? h->last_gain_rows : h->shards[0]->last_gain_rows;
}

// (isa: lag_forms_host_isa -- < 0 the process's choice, which is what the engine calls)
static int lagforms_host_entry(int isa, const double* M, const double* s, double n_bulk, int32_t d, const double* theta, double dt,
                               const double* p0, int32_t K, int32_t mask, int32_t taps_given, double* taps, double* raw,
                               double* acc, double* chk) {
    if (!M || !s || !theta || !taps || !raw || !acc || !chk || d < 1 || d > 2) return SSDE_ERR_ARG;
    if (K < LAG_CHECK || K > LAG_KMAX || !(dt > 0.0) || !std::isfinite(dt)) return SSDE_ERR_ARG;
    IsoArgs a;
    memset(&a, 0, sizeof(a));
    const double sig = exp(theta[0]);
    a.h = sig * sig;
    for (int i = 0; i < d; i++) a.mu[i] = theta[1 + i];
    a.tau = exp(theta[1 + d]);
    const double nu = exp(theta[2 + d]);
    a.beta = 1.0 / a.tau;
    a.sigma = 2.0 * nu / sqrt(M_PI * a.tau);
    ctcrw_trans(dt, a.tau, a.beta, a.sigma, a.ctr);
    // the stationary gains: the covariance half of the filter until it has stopped moving (as build_gain_table)
    CtcrwCov<15> C;
    if (p0) C.init(p0[0], p0[1], p0[2]); else C.init(1.0, 0.0, 1.0);
    CtcrwGain G;
    int stable = 0;
    for (int t = 0; t < 100000 && stable < GAIN_SETTLED_ROWS; t++) {
        const CtcrwCov<15> prev = C;
        if (d == 1) ctcrw_cov_step<1, 15>(C, a.ctr, a.h, false, G); else ctcrw_cov_step<2, 15>(C, a.ctr, a.h, false, G);
        stable = ctcrw_cov_settled(C, prev) ? stable + 1 : 0;
    }
    if (stable < GAIN_SETTLED_ROWS || G.iF == 0.0) return SSDE_ERR_ARG;      // (no stationary regime: such an evaluation streams every row)
    a.gain_stat[0] = G.iF; a.gain_stat[1] = G.k1; a.gain_stat[2] = G.k2; a.gain_stat[3] = G.bm;
    for (int j = 0; j < NDIRP; j++) { a.gain_stat[4 + j] = G.diF[j]; a.gain_stat[7 + j] = G.dk1[j]; a.gain_stat[10 + j] = G.dk2[j]; }
    fill_stat_consts(SSDE_MODEL_CTCRW, d, a);
    LagFormArgs f;
    LagFormOut o;
    lag_form_taps(a, d, mask < 0 ? (DIR_SIG | DIR_MU | DIR_P1 | DIR_P2) : mask, K, f);
    if (taps_given) {                                       // the caller's taps, as they are (nothing beyond the cut is read)
        for (int i = 0; i < LAG_N; i++) { f.lam[i] = taps[i]; f.rr[i] = taps[LAG_N + i]; }
        lag_tap_sums(f);
    } else {
        for (int i = 0; i < LAG_N; i++) { taps[i] = f.lam[i]; taps[LAG_N + i] = f.rr[i]; }
    }
    f.M = M; f.s = s; f.n = n_bulk;
    if (isa < 0) lag_forms_host(f, o); else lag_forms_host_isa(f, o, isa);
    for (int c = 0; c < 2; c++)
        for (int j = 0; j < LAG_NRAW; j++) raw[c * LAG_NRAW + j] = o.raw[c][j];
    for (int k = 0; k < 4 + d; k++) acc[k] = o.acc[k];
    *chk = o.chk;
    return SSDE_OK;
}

extern "C" int ssde_lagforms_host(const double* M, const double* s, double n_bulk, int32_t d, const double* theta, double dt,
                                  const double* p0, int32_t K, int32_t mask, int32_t taps_given, double* taps, double* raw,
                                  double* acc, double* chk) {
    return lagforms_host_entry(-1, M, s, n_bulk, d, theta, dt, p0, K, mask, taps_given, taps, raw, acc, chk);
}

extern "C" int ssde_lagforms_host_isa(int32_t isa, const double* M, const double* s, double n_bulk, int32_t d, const double* theta,
                                      double dt, const double* p0, int32_t K, int32_t mask, int32_t taps_given, double* taps,
                                      double* raw, double* acc, double* chk) {
    if (isa < 0 || isa > 1 || (isa == 1 && !lag_forms_wide())) return SSDE_ERR_ARG;
    return lagforms_host_entry(isa, M, s, n_bulk, d, theta, dt, p0, K, mask, taps_given, taps, raw, acc, chk);
}

extern "C" int ssde_lagforms_host_m(int32_t model, const double* M, const double* s, double n_bulk, const double* ref, int32_t d,
                                    const double* theta, double dt, const double* p0, int32_t K, int32_t mask, int32_t taps_given,
                                    double* taps, double* raw, double* acc, double* chk) {
    if (model == SSDE_MODEL_CTCRW) return ssde_lagforms_host(M, s, n_bulk, d, theta, dt, p0, K, mask, taps_given, taps, raw, acc, chk);
    if (model != SSDE_MODEL_OU_SSM && model != SSDE_MODEL_BM_SSM) return SSDE_ERR_ARG;
    const bool ou = model == SSDE_MODEL_OU_SSM;
    if (!M || !s || !theta || !taps || !raw || !acc || !chk || d < 1 || d > 2 || (ou && !ref)) return SSDE_ERR_ARG;
    if (K < LAG_CHECK || K > LAG_KMAX || !(dt > 0.0) || !std::isfinite(dt)) return SSDE_ERR_ARG;
    IsoArgs a;
    memset(&a, 0, sizeof(a));
    const double sig = exp(theta[0]);
    a.h = sig * sig;
    for (int i = 0; i < d; i++) a.mu[i] = theta[1 + i];
    if (ou) {
        a.tau = exp(theta[1 + d]);
        a.sigma = exp(theta[2 + d]);
        ou_trans(dt, a.tau, a.sigma, a.str);
    } else {
        a.sigma = exp(theta[1 + d]);
        bm_trans(dt, a.sigma, a.str);
    }
    // the stationary gains: the covariance half of the filter until it has stopped moving (as build_gain_table)
    ScalCov<15> C;
    C.init(p0 ? p0[0] : 1.0);
    ScalGain G;
    int stable = 0;
    for (int t = 0; t < 100000 && stable < GAIN_SETTLED_ROWS; t++) {
        const ScalCov<15> prev = C;
        if (ou) { if (d == 1) scal_cov_step<1, 15, true>(C, a.str, a.h, false, G); else scal_cov_step<2, 15, true>(C, a.str, a.h, false, G); }
        else { if (d == 1) scal_cov_step<1, 15, false>(C, a.str, a.h, false, G); else scal_cov_step<2, 15, false>(C, a.str, a.h, false, G); }
        bool same = gain_close(C.p, prev.p);
        for (int j = 0; j < NDIRP && same; j++) same = gain_close(C.dp[j], prev.dp[j]);
        stable = same ? stable + 1 : 0;
    }
    if (stable < GAIN_SETTLED_ROWS || G.iF == 0.0) return SSDE_ERR_ARG;      // (no stationary regime: such an evaluation streams every row)
    a.gain_stat[0] = G.iF; a.gain_stat[1] = G.k; a.gain_stat[2] = G.c;
    for (int j = 0; j < NDIRP; j++) { a.gain_stat[4 + j] = G.diF[j]; a.gain_stat[7 + j] = G.dk[j]; }
    fill_stat_consts(model, d, a);
    LagScalArgs f;
    LagFormOut o;
    lag_form_taps_scal(model, a, d, mask < 0 ? (DIR_SIG | DIR_MU | DIR_P1 | DIR_P2) : mask, K, ref, f);
    if (taps_given) {                                       // the caller's taps, as they are (nothing beyond the cut is read)
        for (int i = 0; i < LAG_N; i++) { f.lam[i] = taps[i]; f.t1[i] = taps[LAG_N + i]; f.t3[i] = taps[2 * LAG_N + i]; }
    } else {
        for (int i = 0; i < LAG_N; i++) { taps[i] = f.lam[i]; taps[LAG_N + i] = f.t1[i]; taps[2 * LAG_N + i] = f.t3[i]; }
    }
    f.M = M; f.s = s; f.n = n_bulk;
    lag_forms_scal_host(f, o);
    for (int c = 0; c < 2; c++)
        for (int j = 0; j < LAG_NRAW_SCAL; j++) raw[c * LAG_NRAW_SCAL + j] = o.raw[c][j];
    for (int k = 0; k < 4 + d; k++) acc[k] = o.acc[k];
    *chk = o.chk;
    return SSDE_OK;
}
