// ssde_engine.hpp -- internals shared by the engine's translation units (ssde_engine.hip: C ABI, constant-coefficient
// and direct paths; ssde_engine_tv.hip: the lane = gradient direction path).  Not part of the C ABI.
#ifndef SSDE_ENGINE_HPP
#define SSDE_ENGINE_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/ssde.h"
#include "ssde_device.hpp"
#include "ssde_host.hpp"
#include "ssde_knobs.hpp"
#include "ssde_lagstats.hpp"
#include "ssde_reduce_host.hpp"
#include "ssde_tv.hpp"
#include "ssde_windows.hpp"

namespace ssde { struct HeadFormWork; }     // ssde_headforms.hpp

namespace ssde_engine {

extern thread_local std::string g_create_error;   // message of the last failed ssde_create on this thread

enum { PATH_DIRECT = 0, PATH_ISO = 1, PATH_DENSE = 2, PATH_TV = 3 };
constexpr int PAR_RING = 8;
constexpr WindowConsts WINDOW_CONSTS = {ssde::WIN_ALIGN, ssde::SHARED_U, ssde::LAG_A, ssde::LAG_KMAX};   // (ssde_windows.hpp)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t alloc(size_t count) {
        n = count;
        if (count == 0) { p = nullptr; return hipSuccess; }
        return hipMalloc((void**)&p, count * sizeof(T));
    }
    hipError_t upload(const std::vector<T>& v) {
        hipError_t e = alloc(v.size());
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

}  // namespace ssde_engine

using ssde_engine::DevBuf;
using ssde_engine::PAR_RING;
using namespace ssde;
using namespace ssde_host;

struct ssde_handle {
    std::string err;
    int model = 0, d = 0, q = 0, sdim = 0, na_any = 0, device = 0, path = 0;
    int64_t n = 0, n_seg = 0, n_steps = 0;
    bool has_h = false, const_coeff = false, uniform_dt = false;
    double dt_uniform = 0.0;
    double tdf = 0.0, tconst = 0.0;     // BM_t: degrees of freedom, normalising constant of dt(., df)
    double p0_iso[3] = {0, 0, 0};
    double p0_full[256] = {0};     // sdim x sdim column-major (sdim <= 16)
    bool wide_ok = false;          // set by ssde_create for a response of 3 to 8 columns that has to run as ONE filter (coupling H_array / P0)
    ParLayout L;
    Penalty pen;
    std::vector<Slot> slots;
    int n_stream_cols = 0;
    std::vector<uint8_t> fixed;
    int n_free = 0;

    // Kalman tiles
    DevBuf<double> tiles, a0;
    DevBuf<int64_t> group_off, lane_row0;
    DevBuf<int32_t> group_len, lane_nsteps;
    int n_groups = 0, C = 0;
    int c_obs = 1;                 // tile channel of the first obs column (0: no dt channel, globally regular grid)
    double dt_all = 0.0;
    int64_t tile_doubles = 0;

    // direct families (long format, engine-owned copies)
    DevBuf<double> times, obs, colbuf, tdecay;
    DevBuf<uint32_t> scored;
    DevBuf<const double*> colptr;
    int direct_blocks = 0;

    // random-effect blocks given as piecewise-cubic functions of a covariate (ssde_ppbasis): tables in HBM; either
    // evaluated on the fly by the fast direct kernel (pp_fast) or materialised once into dense columns (pp_mat)
    PPRef pp[MAX_Q] = {};
    bool pp_fast[MAX_Q] = {false, false, false, false};
    DevBuf<double> pp_x[MAX_Q], pp_knots[MAX_Q], pp_tab[MAX_Q], pp_mat[MAX_Q];
    PpDrift pp_drift = {};                     // nb > 0: a smooth drift whose blocks the lanes evaluate from the tables (k_iso_drift_pp.hip); the tiles hold the covariates
    int pp_drift_j[2] = {-1, -1};              // ... the SDE parameter of each block
    bool no_drift_pp = false;                  // (a second build after SSDE_RETRY_WITHOUT_PP)
    bool force_tv = false;                     // the lane = direction path whatever the batch's size (the companion of SSDE_FLAG_EXACT_HESS)
    ssde_handle* hess_companion = nullptr;     // SSDE_FLAG_EXACT_HESS: the same problem on the lane = direction path, for k_tv_hess.hip
    int n_stream_cols_algo = 0;                    // streamed columns of the reference's data contract (algorithmic bytes)

    // fast direct kernel (<= 2 parameters with streamed columns)
    bool direct_fast = false;
    int64_t col_stride = 0;                        // doubles between consecutive streamed columns
    int df_ja = -1, df_jb = -1;
    std::vector<int> df_pidxA, df_pidxB;          // full-par indices of the streamed coefficients
    int df_icpt[MAX_Q] = {-1, -1, -1, -1};         // full-par index of each parameter's intercept, or -1
    const double *df_colA = nullptr, *df_colB = nullptr;
    bool direct_uniform_dt = false;
    double direct_dt = 0.0;

    // dense / direct parameter plumbing
    DevBuf<SlotTable> slot_table;
    DevBuf<DenseDir> dirs;
    std::vector<DenseDir> dirs_host;
    int n_dirblocks = 0;
    DevBuf<double> par_ring;
    double* par_pinned = nullptr;
    hipEvent_t par_ev[PAR_RING];
    bool par_ev_ok = false;
    int par_next = 0;

    DevBuf<double> partials, out;
    size_t partial_doubles = 0;

    // iso time windows
    DevBuf<double> bnd, chk;
    int max_chunks = 1;            // allocation bound
    int want_chunks = 1;           // planned number of equal windows (the transient window comes on top)
    int want_chunks_d = 0;         // mixed batch: windows of the general launch's own plan (0 = one plan for everything)
    int glen_max = 0;              // steps of the longest track group
    double dt_min = 0.0;           // smallest interval used inside a track
    double dt_max = 0.0;           // ... and the largest
    bool chunks_forced = false;    // SSDE_CHUNKS given: the window count is the tester's (1 = plain sequential filter)
    bool stream_nt = true;         // the tile stream is read with non-temporal loads (a batch far larger than the Infinity Cache)
    // quiet rows of the general kernel (k_iso.hip): blocks that hold a missing observation, per group; 0 words = not in use
    DevBuf<unsigned long long> nan_bits;
    DevBuf<double> quiet_flag;
    int nan_words = 0;
    bool quiet_ok = false;
    double quiet_share = 0.0;      // share of the dirty groups' blocks that qualify (nominal 128-row memory)
    int last_quiet_window = 0;     // rows of memory the last launch used (0: no quiet rows)
    bool gain_stationary = false;  // the last gain recursion reached its stationary row
    double stat_p[12] = {0}, stat_ld = 0.0, stat_gld[3] = {0, 0, 0};   // ... the covariance, log F and dF / F there
    double plan_rho = 1.0;         // spectral radius of the closed-loop matrix the last plan found
    int plan_warmup = 0;           // warm-up rows the last plan found sufficient (0: no usable forgetting)
    int last_chunks = 1, last_window = 0;
    ssde_engine::Knobs knobs;      // testing / tuning knobs, read once, by build(): nothing reads the environment per evaluation
    // The retry / probation policy around ssde_eval (ssde_windows.hpp).  A top-level handle decides with its own; the shards of a
    // multi-device parent plan with the parent's (create_sharded sets the pointer), so every engine of a handle sees one boost.
    ssde_engine::WindowPolicy own_policy;
    ssde_engine::WindowPolicy* parent_policy = nullptr;
    ssde_engine::WindowPolicy& policy() { return parent_policy ? *parent_policy : own_policy; }
    const ssde_engine::WindowPolicy& policy() const { return parent_policy ? *parent_policy : own_policy; }
    int saved_max_chunks = 0, saved_want_chunks = 0;   // this engine's limits from before the policy gave up on windows (apply_chunks)

    // shared-covariance path
    DevBuf<int32_t> group_flags;
    DevBuf<int32_t> dirty_groups;   // the groups that hold a track with a missing row (mixed batch: the general launch's)
    int n_dirty_groups = 0;
    int n_clean_groups = 0;
    bool use_shared = false;
    int drift = 0;                 // row-varying drift on the register path (k_iso_drift.hip): 1 = shared-covariance lanes (regular grid, complete
                                   // tracks), 2 = lanes with their own covariance (missing rows / irregular grid)
    int drift_nstate = 0;          // components of its hand-over dumps
    DevBuf<ssde::CvPart> cv_parts;  // drift == 3 (row-varying tau / nu on lane = track lanes, k_iso_colvar.hip): the columns of the four parts
    std::vector<int> cv_pidx;      // [CV_WAVES][CV_KC] full-parameter index of a part's column, -1 = unused slot
    int cv_mu_part = -1, cv_sig_part = -1;   // the parts that carry the drift-intercept / log sigma_obs direction
    int cv_kc = 0;                 // the widest part's column count
    bool cv_full = false;          // 4 x 4 covariance lanes (CTCRW, d = 2, per-row H_array)
    bool cv_single = false;        // ... with constant tau / nu: one wave per (group, window) runs filter and tangents (iso_full_kernel)
    bool cv_few = false;           // few design columns, H = sigma_obs^2 I: one wave per (group, window) too (iso_few_kernel)
    DevBuf<unsigned> fuse_words;   // the fused finalising work of iso_shared_kernel: [0] finished work items, [2..3] the check word, [4..] arrivals per (boundary, group)
    int last_finish_form = 0;      // what finished the last evaluation: 0 a finalize launch, 1 fused in the main launch, 2 the host (ssde_last_finish_form)
    // The head finished on the host (iso_shared_wg_kernel with IsoArgs.mbx, ssde_reduce_host.hpp): the workgroups store their group's
    // record into this pinned mailbox, the synchronous call spins on the groups' sequence words and forms the result itself.  One per
    // handle: a synchronous call has consumed it before the next one starts.
    double* mbx_pinned = nullptr;             // [n_groups][MBX_STRIDE]
    unsigned long long mbx_seq = 0;
    bool host_finish_ok = false;              // eval_device: this evaluation is a synchronous single-engine ssde_eval into h->out
    bool host_armed = false;                  // the evaluation just enqueued ends in the mailbox (set by eval_iso, consumed by run_once)
    ReduceArgs host_ra;                       // ... and these are its reduction's arguments (add, map, the bulk's forms)
    std::vector<double> reduce_scratch;
    bool cv_adj = false;           // gradient by a reverse sweep: one wave per (group, window), two passes (iso_adj_kernel)
    DevBuf<double> adj_ckpt;       // ... the state entering every adj_ckpt_rows-th row of every window (grown on demand)
    bool cv_one_wave() const { return cv_single || cv_few || cv_adj; }
    double cv_hmax = 0.0;          // ... the largest diagonal entry of H_array over the batch (the window planner's observation variance)
    std::vector<double> cv_col_lo, cv_col_hi;   // range of every streamed column over the batch (found at create)
    DevBuf<double> cv_ranges;      // [workgroup][4] ranges of the linear predictors seen by the last launch
    double* cv_ranges_pinned = nullptr;   // ... reduced over the launch: min / max of p1, min / max of p2 (host-visible; +inf / -inf before the first launch)
    double cv_eta_lo[2] = {0, 0}, cv_eta_hi[2] = {0, 0};   // range the linear predictors of par[d], par[d + 1] can reach at the last parameters
    // exact Hessian over the drift coefficients (ssde_hess.hip): eval_device launches the Hessian kernels instead of an evaluation
    DevBuf<double> hs_partials, hs_hess;      // scratch of the Hessian passes, kept between calls (allocation costs more than the pass)
    DevBuf<int16_t> hs_i16;
    bool hess_req = false;
    DriftHessArgs hess_args;
    int hess_tiles = 0;
    // one-row tracks never reach a kernel; REPORT(aest_all) still shows their a0 (nllk_ctcrw.hpp:196-200, 246)
    std::vector<int64_t> single_rows;
    std::vector<double> single_a0;       // [single_rows.size()][sdim]
    std::vector<std::pair<int, int64_t>> clean_ns_hist;  // (scored rows, number of tracks) over NaN-free groups
    DevBuf<double> gain_ring;
    double* gain_pinned = nullptr;
    size_t gain_rows_cap = 0;
    int last_gain_rows = 0;
    int last_occ_form = 0;         // the forms of the last ssde_path_occupancy: bit 0 the LDS-tile form, bit 1 the global form (ssde_last_occupancy_form)
    int64_t last_occ_points = 0, last_occ_capped = 0;   // of the last ssde_path_occupancy_fine (ssde_last_occupancy_points)
    int64_t last_prox_tiles = 0, last_prox_tiles_max = 0;   // of the last ssde_path_proximity (ssde_last_proximity_plan) ...
    int last_prox_batches = 0, last_prox_route = 0;     // ... its batches of draws, and 1: positions stayed on the device, 2: gathered from shards
    ssde_engine::HessPlanInfo hess_plan;                            // of the last ssde_hess (ssde_last_hess_plan; ssde_windows.hpp)
    int last_gain_feed = 0;        // how the last evaluation's launch got its gain table: 0 the ring and a copy, 1 by value (ssde_last_gain_feed)
    std::vector<double> gain_scratch;        // a deferred table's rows (build_gain_table / feed_gain_table)
    bool par_ev_pending[PAR_RING] = {false, false, false, false, false, false, false, false};   // slot last used by an asynchronous call
    bool sync_call = false;        // set around the evaluation of a synchronous ssde_eval (single engine, null stream)
    bool device_current = false;   // run_once has just made h->device the thread's current device: eval_device need not (set and cleared by run_once alone)

    // side streams: the kernels of one evaluation that do not depend on each other run concurrently
    hipStream_t aux[2] = {nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    hipEvent_t ev_async = nullptr;            // end of the last ssde_eval_device on the caller's stream: a synchronous call waits for it
    bool async_pending = false;

    // timing of the dominant kernel (recorded on the stream it is launched on)
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;   // the CURRENT evaluation's pair: ev_ring[ev_idx % EV_RING]
    bool ev_k_valid = false;
    bool stamps = true;                            // SSDE_OPT_KERNEL_STAMPS: 0 = plain launches, no event pair per evaluation
    // Every evaluation stamps its dominant kernel with a pair of its own, so that a caller can time K evaluations and read
    // the K kernel durations AFTERWARDS (ssde_kernel_ms_history) instead of paying an event query between them.
    static constexpr int EV_RING = 64;
    hipEvent_t ev_ring[EV_RING][2] = {};
    bool ev_ring_valid[EV_RING] = {};
    int64_t ev_idx = -1;
    std::vector<int32_t> glen_host, lane_ns_host;
    int last_s_stat = 0, last_t0 = 0, last_t0_delta = 0;
    mutable int rows_key[3] = {-1, -1, -1};
    mutable int64_t rows_cached = 0;

    // iso direction split
    int iso_parts = 1;
    int iso_masks[MAX_PARTS] = {0, 0, 0, 0};
    int iso_free_mask = 0;

    // row-varying isotropic path (k_tv.hip)
    DevBuf<double> tv_rec, tv_wdir, tv_a0, tv_bnd, tv_chk, tv_gval, tv_gdir, tv_stats, tv_harr, tv_eh, tv_eR;
    bool tv_dense = false;         // full-covariance lanes: per-row H_array and / or a P0 that is not block-identical
    DevBuf<TvDir> tv_dirs;
    DevBuf<int64_t> tv_row0;
    // [lanes] the ID segment (in the handle's data) of every lane's track, tiled routes and PATH_TV alike: a0 at create, and the
    // deviates' track counter of ssde_smooth_draws
    DevBuf<int64_t> lane_seg;
    // [lanes] the interval the data hold for the first row of every lane's track, tiled routes (the tiles start at the second row;
    // PATH_TV keeps the times): the lead time of a forecast from that row (ssde_forecast_scores)
    DevBuf<double> lane_dt0;
    DevBuf<int32_t> tv_ns;
    DevBuf<TvItem> tv_items_g, tv_items_v;     // work items of a gradient / a value-only evaluation
    std::vector<int32_t> tv_ns_host;
    int tv_nd = 0, tv_ndp = 0, tv_lpt_shift = 0, tv_nb = 1;
    int tv_n_items_g = 0, tv_n_items_v = 0, tv_window = -1, tv_max_nc = 1;
    size_t tv_items_cap = 0;
    double* tv_stats_pinned = nullptr;
    hipEvent_t tv_stats_ev = nullptr;
    bool tv_stats_valid = false;
    int tv_stats_blocks = 0;
    int16_t tv_dir_of_par[MAX_PAR];
    // hipGraph replay of a synchronous tv evaluation (ssde_eval): upload, pre-pass, statistics read-back, filter,
    // finalize and result read-back are captured once per plan and replayed with ONE launch call
    hipStream_t tv_stream = nullptr;
    hipGraphExec_t tv_gexec[2] = {nullptr, nullptr};    // [order]
    int tv_graph_plan[2] = {-1, -1};                    // plan generation the executable was captured for
    int tv_plan_gen = 0;
    DevBuf<double> tv_par_dev;
    double* tv_par_pinned = nullptr;
    double* tv_out_pinned = nullptr;
    double* tv_chk_pinned = nullptr;          // [TV_LEAN_ITEMS] the items' hand-over checks of a lean replay (eval_tv_graph)
    bool tv_graph_lean[2] = {false, false};
    DevBuf<double> lap_out;                   // ssde_laplace_eval: result vectors of a batch of asynchronous evaluations
    // publication of a synchronous evaluation's result by its reducing launch (ReduceArgs.pub, ssde_device.hpp): the host spins
    // on a sequence word in pinned memory instead of issuing a read-back copy
    double* pub_pinned = nullptr;             // [2 + n_full] result, then (128-byte aligned) the sequence word
    unsigned long long* pub_flag = nullptr;
    unsigned long long pub_seq = 0;
    DevBuf<unsigned int> pub_count;
    DevBuf<double> wave_clock;                // SSDE_WAVE_CLOCK=file: per-wave stamps of the last shared-covariance launch, written at destroy
    int wave_clock_items = 0;
    bool pub_request = false;                 // run_once asks the next eval_device to publish
    std::vector<double> gain_cum[4];          // build_gain_table's running sums
    bool pub_armed = false;                   // the evaluation just enqueued will publish (set by eval_device, consumed by run_once)
    std::vector<double> eval_out;             // ssde_eval's result vector (no allocation per call)

    int64_t hbm_bytes = 0;
    // dtimes(n-1) of the reference is 1 (nllk_ctcrw.hpp:126-129); a shard of a multi-device handle that is not the last
    // one carries the real interval to the next shard's first row there (only REPORT(aest_all) ever shows it)
    double last_dt = 1.0;
    // lattice padding (ssde_engine.hip: lattice_pad): the tiles hold n_pad > n rows; pad_pos[i] = the lattice row whose
    // reported state is caller row i's (ssde_report)
    int64_t n_pad = 0;
    DevBuf<int64_t> pad_pos;
    DevBuf<int64_t> pad_row;       // the lattice row of caller row i itself (ssde_smooth: the state AT the row, not predicted past it)
    double pad_step = 0.0;
    double snap_dt = 0.0;          // > 0: a grid that is regular to SSDE_GRID_RTOL (last-bit jitter of decimal steps): this step is hoisted

    // ---- distributed evaluation (ssde_engine_dist.hip) -------------------------------------------------------------
    // single-process multi-GPU parent (ssde_desc.n_devices > 1): one engine per device, this handle owns no device data
    std::vector<ssde_handle*> shards;
    std::vector<int64_t> shard_row0;          // first global row of each engine
    std::vector<int64_t> shard_nrows;         // its rows
    std::vector<int> shard_col0;              // first column of aest_all it reports (dimension parts: 2 or 4 columns each)
    std::vector<int> shard_leader;            // index of the first engine on the same device (its stream and out buffer
                                              // collect that device's engines before the collective)
    int n_track_shards = 1, n_dim_parts = 1;
    std::vector<double> poison_vec;           // the NaN result vector of a poisoned handle (ssde_eval_device)
    bool poison = false;                      // SSDE_NA_ANY_NAN, n_dim > 2: an observed row with a NaN outside column 0
    std::vector<void*> comms;                 // ncclComm_t: one per shard (parent), or one (ssde_comm_init_rank)
    bool shards_share_device = false;         // rehearsal on a one-GPU machine: shards summed by a kernel, not RCCL
    int comm_ranks = 1;                       // ranks of a multi-process communicator (the caller's argument)
    int comm_ranks_reported = 0;              // ... what ncclCommCount says about it (0: no communicator)
    int64_t smooth_budget_mb = 0;             // SSDE_OPT_SMOOTH_BUDGET_MB: cap on ssde_smooth's record buffer (0: a quarter of the free memory)
    bool comm_defer = false;                  // SSDE_OPT_COMM_DEFER: ssde_eval_device leaves the rank's partial result to the caller's own collective
    // the bulk of a stationary batch from lag statistics (ssde_lagstats.hpp): built at create when the rule engages it
    bool lag_ready = false;
    DevBuf<double> lag_M, lag_s;           // [LAG_N][LAG_N], [2][LAG_N]
    DevBuf<int32_t> lag_glen, lag_ns;      // group_len / lane_nsteps capped at LAG_A: what the streamed head launch walks
    std::vector<double> lag_M_host, lag_s_host;   // the same on the host: what an evaluation's forms read (ssde_lagforms.hpp)
    double lag_n = 0.0;                    // bulk rows (past LAG_A) of the batch
    double lag_ref[2] = {0.0, 0.0};        // OU_SSM: what the statistics' levels are centred on (ssde_lagstats.hpp); 0 otherwise
    int64_t lag_rows = 0, last_lag_rows = 0;   // ... and those the last evaluation took from the statistics (0: streamed)
    double lag_create_ms = 0.0;            // what building them cost at create
    // ... at the early cuts (CTCRW; ssde_lagstats.hpp: LAG_CUT_MIN .. LAG_CUT_MAX), index c = lag_cut_index(cut): built with the late ones
    // when the dispatch rule builds those, or at ssde_set_option(SSDE_OPT_LAG_EARLY, 1); lag_cut_mask == 0: none
    unsigned lag_cut_mask = 0;             // bit c: the statistics of cut c exist
    bool lag_early = false;                // SSDE_OPT_LAG_EARLY: an evaluation may cut the bulk at its transient's end
    std::vector<double> lag_cut_M_host[ssde::LAG_NCUT], lag_cut_s_host[ssde::LAG_NCUT];
    double lag_cut_n[ssde::LAG_NCUT] = {};
    int64_t lag_cut_rows[ssde::LAG_NCUT] = {};
    DevBuf<double> lag_cut_M[ssde::LAG_NCUT], lag_cut_s[ssde::LAG_NCUT];          // the device copies (ssde_lagstats_read_cut)
    DevBuf<int32_t> lag_cut_glen[ssde::LAG_NCUT], lag_cut_ns[ssde::LAG_NCUT];     // group_len / lane_nsteps capped at the cut
    DevBuf<int32_t> lag_cut_nsmin[ssde::LAG_NCUT];   // [n_groups] the smallest lag_cut_ns of a group over its lanes with a track (head_ns_min)
    int lag_lead_n = 0;                    // groups g < lag_lead_n lie at g * lag_lead_stride doubles of the tiles (head_lead_groups)
    int64_t lag_lead_stride = 0;
    std::vector<int32_t> lag_host_glen, lag_host_ns;   // the uncapped lengths, kept for a later build of the early cuts
    // The head's rows as Gram statistics (ssde_headforms.hpp; CTCRW, d = 2, every track >= HEAD_C rows): built with the early cuts where
    // the dispatch rule builds those, or at ssde_set_option(SSDE_OPT_LAG_HEAD_HOST, 1).  A synchronous single-engine evaluation whose
    // cut is <= HEAD_C then forms the head's accumulators on the host and launches nothing.
    bool head_ready = false;               // the statistics exist
    bool head_host = false;                // SSDE_OPT_LAG_HEAD_HOST: such an evaluation may take the host form
    std::vector<double> head_G_host, head_s_host;   // [HEAD_LDW][HEAD_LDW], [2][HEAD_LDW]: zero-padded, as the forms read them
    double head_n = 0.0;                   // tracks
    DevBuf<double> head_G, head_s;         // the device copies ([HEAD_NW][HEAD_NW], [2][HEAD_NW]: ssde_headstats_read)
    ssde::HeadFormWork* head_work = nullptr;   // the forms' work arrays (no allocation per evaluation)
    std::vector<double> head_rec;          // [NACC_MAX] group 0's record, the head's accumulators: every other group's is zero and is not kept (reduce_host_head)
    std::vector<double> head_chk;          // [1] zero: one window has no hand-over
    bool head_armed = false;               // the evaluation just planned ends in head_rec (set by eval_iso, consumed by run_once)
    int last_head_form = 0;                // the head of the last evaluation: 0 the kernel, 1 the statistics (ssde_last_head_form)
    int last_lag_cut = 0;                  // first bulk row of the last evaluation (0: streamed)
    int last_cut_parts = 0;                // > 0: its head ran as this many direction parts per group, one workgroup per padded group (iso_shared_cut_kernel)
    int last_kernel_id = 0;                   // SSDE_KERNEL_*: the family that ran the last evaluation's rows
    // where a stamped synchronous evaluation spent its time (ssde_last_phase_ms): events on the evaluation's stream
    hipEvent_t ev_ph[3] = {nullptr, nullptr, nullptr};   // first operation | end of the finalising launch | end of the all-reduce
    bool ph_valid = false, ph_has_comm = false;
    double ph_host_total_ms = 0.0, ph_host_enq_ms = 0.0;
    // Decisions that shape the SEQUENCE of collectives must be the same on every rank, whatever each rank's own data look
    // like (one rank's shard on a regular grid, another's with missing rows): agreed on once, at ssde_comm_init_rank
    // (min over ranks), and used instead of the local facts while a communicator is joined.  -1 = no communicator.
    int comm_rides = -1;                      // an order-0 ssde_eval evaluates order 1 (grad_rides_along) on every rank, or on none
    int comm_async_ok = -1;                   // ssde_laplace_eval batches its evaluations through ssde_eval_device on every rank, or on none
    hipStream_t own_stream = nullptr;         // stream of the synchronous evaluation when a collective follows it
    // ---- memo of the last ssde_eval (include/ssde.h) ---------------------------------------------------------------
    std::vector<double> memo_par, memo_grad;
    double memo_value = 0.0;
    int memo_order = -1;                      // -1 = nothing memoised
    int64_t n_evals = 0, n_memo_hits = 0;
    // host-side phase clock of the isotropic path (SSDE_TRACE=1 at create; printed at destroy): plan, gain table,
    // main launch(es), finalize launch, read-back
    double trace_us[6] = {0, 0, 0, 0, 0, 0};
    int64_t trace_n = 0;
    int trace_skip = 0;
};


namespace ssde_engine {

#define HIPCHK(h, call)                                                                  \
    do {                                                                                 \
        hipError_t e__ = (call);                                                         \
        if (e__ != hipSuccess) {                                                         \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e__);               \
            return SSDE_ERR_HIP;                                                         \
        }                                                                                \
    } while (0)


int fail(ssde_handle* h, int code, const std::string& msg);

// ssde_engine_build.hip
int build(const ssde_desc* d, ssde_handle* h, const ParLayout* part_layout = nullptr);
void destroy(ssde_handle* h);
int build_lagstats_early(ssde_handle* h);     // the lag statistics at the early cuts (create, ssde_set_option(SSDE_OPT_LAG_EARLY, 1))
int build_headstats(ssde_handle* h);          // the Gram statistics of the head's rows (create, ssde_set_option(SSDE_OPT_LAG_HEAD_HOST, 1))
void attach_hess_companion(const ssde_desc* desc, ssde_handle* h);     // SSDE_FLAG_EXACT_HESS (ssde_engine.hip)
void release_device(ssde_handle* h);          // everything the handle holds on the device / in pinned memory (the handle stays)
int eval_iso(ssde_handle* h, const double* par, int order, double* out_dev, hipStream_t s, ReduceArgs& ra);   // ssde_engine_iso.hip
int eval_device(ssde_handle* h, const double* par, int order, double* out_dev, hipStream_t s);

// ---- distributed evaluation (ssde_engine_dist.hip) --------------------------------------------------------------------
int create_sharded(const ssde_desc* d, ssde_handle* parent);
// sum the shards' [nllk, grad..., check] buffers (RCCL all-reduce, or the rehearsal kernel) -- enqueue only
int reduce_shards(ssde_handle* parent);
// all-reduce one handle's out buffer over its multi-process communicator -- enqueue only
int reduce_ranks(ssde_handle* h, double* buf, hipStream_t s);
int report_sharded(ssde_handle* parent, const double* par, double* aest_all);
int smooth_sharded(ssde_handle* parent, const double* par, double* a_smooth, double* P_smooth, double* resid);
void destroy_dist(ssde_handle* h);
hipError_t launch_sum_into(double* dst, const double* src, int n, hipStream_t s);   // k_reduce.hip

// ---- exact second derivatives, direct families BM / OU (ssde_hess.hip) -------------------------------------------------
// 0: no exact second derivatives; 1: over the drift coefficients of a shared-covariance drift handle (and log_lambda);
// 2: over every coefficient and log_lambda (direct families BM / OU)
int hess_exact_scope(const ssde_handle* h);
inline bool hess_exact_available(const ssde_handle* h) { return hess_exact_scope(h) == 2; }
int hess_exact(ssde_handle* h, const double* par, const int32_t* idx, int n_idx, double* H);

// copy a caller array (host or device) into a fresh device buffer
template <class T>
inline hipError_t stage(const T* src, size_t count, bool on_device, DevBuf<T>& dst) {
    hipError_t e = dst.alloc(count);
    if (e != hipSuccess || count == 0) return e;
    return hipMemcpy(dst.p, src, count * sizeof(T), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
}


// upload the parameter vector for the dense / direct / tv kernels; returns the device pointer (ssde_engine.hip)
int push_par(ssde_handle* h, const double* par, hipStream_t s, const double** dev);

// ---- lane = gradient direction path (ssde_engine_tv.hip) ------------------------------------------------------------
void tv_base_args(const ssde_handle* h, TvArgs& a);
// the general kernel's arguments a handle fixes (tiles, model, P0, rows: everything but slots, parameters, directions and outputs),
// and the handle's slots as a value-only table (ssde_engine.hip)
void dense_base_args(const ssde_handle* h, DenseArgs& a);
SlotTable value_slot_table(const ssde_handle* h);
int build_tv(const ssde_desc* d, ssde_handle* h, const std::vector<int64_t>& starts, bool on_dev);
int tv_plan(ssde_handle* h, double hobs, hipStream_t s);
int eval_tv(ssde_handle* h, const double* par, int order, double* out_dev, hipStream_t s);
int eval_tv_graph(ssde_handle* h, const double* par, int order, double* o_host);

}  // namespace ssde_engine
#endif
