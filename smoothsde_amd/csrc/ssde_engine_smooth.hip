// ssde_engine_smooth.hip -- the host side of the eleven calls that consume the smoother's records:
//     ssde_smooth               the fixed-interval smoother of the Kalman families                        DESIGN.md §3.9
//     ssde_smooth_loo           leave-one-out residuals and predictive densities of every fix             §3.20
//     ssde_forecast_scores      k-step-ahead forecast errors and scores of every fix                      §3.21
//     ssde_smooth_draws         joint posterior draws of the state path                                   §3.10
//     ssde_path_stats           the drawn paths reduced per track and draw                                §3.12
//     ssde_path_speed           the speed along them (CTCRW), per track and draw and counted per row      §3.17
//     ssde_path_occupancy       their occupancy grids                                                     §3.13
//     ssde_path_occupancy_fine  ... refined between the fixes                                             §3.15
//     ssde_predict              the smoothed state between and after the rows                             §3.11
//     ssde_predict_draws        the drawn paths there                                                     §3.14
//     ssde_path_proximity       those states of two tracks, paired and reduced per pair and draw          §3.16
//
// Every call has three layers.  The entry point (extern "C", at the end) checks the arguments before the device is touched; the
// check_* functions hold what several entries check alike.  A parent of several engines goes through *_sharded: for_each_shard, and
// the deal and placement functions of ssde_smooth_plan.hpp.  One engine's work is *_single: a RecordRun produces the records (a
// forward pass in record mode: dense_kernel MODE 2 on the tiled routes, smooth_tv_record_kernel on PATH_TV) chunk by chunk under
// SSDE_OPT_SMOOTH_BUDGET_MB -- groups of 64 tracks are independent, so no result depends on the chunking -- and the call's kernel
// consumes each chunk; the calls that draw also go batch by batch through walk_batches.
// The steps the calls share exist once, ahead of the calls.  Where the calls DIFFER, the difference is behaviour and is written out
// at the call: which budget sizes the batches (batch_budget asks the free memory again, run.budget does not), the unit of a batch,
// which empty handle returns before anything is allocated.  Every buffer is the call's own: the handle's record / stats buffers,
// memo and window state are not touched.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>
#include <tuple>

#include "ssde_engine.hpp"
#include "ssde_occ.hpp"
#include "ssde_predict.hpp"
#include "ssde_prox.hpp"
#include "ssde_smooth_plan.hpp"

using namespace ssde_engine;
using namespace ssde_plan;

namespace {

// releases a call's buffers on every way out
template <class... B>
struct Release {
    std::tuple<B&...> bufs;
    explicit Release(B&... b) : bufs(b...) {}
    ~Release() { std::apply([](auto&... b) { (b.release(), ...); }, bufs); }
};

// what the entry points check alike (the strings are part of the interface)
int refuse(ssde_handle* h, int code, const std::string& msg) { h->err = msg; return code; }      // (the handle's message only)
int check_par_len(ssde_handle* h, int32_t n_par_full) {
    return n_par_full == h->L.n_full ? SSDE_OK : refuse(h, SSDE_ERR_ARG, "parameter vector has the wrong length");
}
int check_kalman(ssde_handle* h) {
    return is_kalman(h->model) ? SSDE_OK : refuse(h, SSDE_ERR_MODEL, "the smoother serves the Kalman families only (the direct families have no state; ESEAL_SSM no REPORT)");
}
int check_not_coupled_wide(ssde_handle* h, const char* who) {
    return h->d <= 2 ? SSDE_OK : refuse(h, SSDE_ERR_MODEL, std::string(who) + ": a response of three or more columns that runs as ONE coupled filter is not served (uncoupled wide responses run as column pairs and are)");
}
// a call that needs `which` columns in one lane for a `what` serves no response of three or more columns
int check_position_columns(ssde_handle* h, const std::string& who, const char* what, const char* which) {
    return h->d <= 2 ? SSDE_OK : refuse(h, SSDE_ERR_MODEL, who + ": a response of three or more columns is not served, as column pairs or as one coupled filter (a " + what + " needs the " + which + " columns in one lane)");
}
int check_draw_range(ssde_handle* h, const std::string& who, int64_t draw0, int32_t n_draws) {
    return (n_draws < 1 || draw0 < 0 || draw0 + (int64_t)n_draws >= ((int64_t)1 << 28))
        ? refuse(h, SSDE_ERR_ARG, who + ": n_draws >= 1, draw0 >= 0 and draw0 + n_draws < 2^28 are required") : SSDE_OK;
}
// query by query, the row before the offset
int check_queries(ssde_handle* h, const std::string& who, const int64_t* q_row, const double* q_off, int64_t nq) {
    for (int64_t k = 0; k < nq; k++) {
        if (q_row[k] < 0 || q_row[k] >= h->n) return refuse(h, SSDE_ERR_ARG, who + ": a query row outside [0, n)");
        if (!std::isfinite(q_off[k]) || q_off[k] < 0.0) return refuse(h, SSDE_ERR_ARG, who + ": a query offset that is negative or not finite");
    }
    return SSDE_OK;
}
// the bridge deviates' counter holds the rank of an offset in its interval in 32 bits (sorted only where the queries could pass that)
int check_distinct_offsets(ssde_handle* h, const std::string& who, const int64_t* q_row, const double* q_off, int64_t nq) {
    const int64_t limit = (int64_t)1 << 32;
    return (nq >= limit && max_distinct_offsets(q_row, q_off, nq) + 1 >= limit)
        ? refuse(h, SSDE_ERR_ARG, who + ": an interval with 2^32 or more distinct offsets") : SSDE_OK;
}
// n weights (NULL: none), each finite and >= 0; wmax: the largest (1 without weights)
int check_weights(ssde_handle* h, const std::string& who, const double* weight, int64_t n, double& wmax) {
    wmax = weight ? 0.0 : 1.0;
    for (int64_t i = 0; weight && i < n; i++) {
        if (!(weight[i] >= 0.0 && weight[i] <= std::numeric_limits<double>::max()))         // negative, NaN or inf
            return refuse(h, SSDE_ERR_ARG, who + ": a weight that is negative or not finite");
        wmax = std::max(wmax, weight[i]);
    }
    return SSDE_OK;
}

// the thresholds of a call that counts them in its statistics (ssde_smooth_loo, ssde_forecast_scores): at most max_thr, each finite
// and >= 0, and none without the statistics
int check_thresholds(ssde_handle* h, const std::string& who, const double* thr, int32_t n_thr, int max_thr, const char* max_name, bool have_stats) {
    if (n_thr < 0 || n_thr > max_thr || (n_thr > 0 && !thr))
        return refuse(h, SSDE_ERR_ARG, who + ": 0 <= n_thr <= " + max_name + ", with a table of thresholds when there are any");
    for (int k = 0; k < n_thr; k++)
        if (!std::isfinite(thr[k]) || thr[k] < 0.0) return refuse(h, SSDE_ERR_ARG, who + ": a threshold that is not finite or negative");
    if (n_thr > 0 && !have_stats) return refuse(h, SSDE_ERR_ARG, who + ": thresholds are counted in the statistics, which were not asked for");
    return SSDE_OK;
}

// a quarter of the free memory, in doubles: the budget where SSDE_OPT_SMOOTH_BUDGET_MB sets none
int free_budget(ssde_handle* h, int64_t& budget) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
    budget = (int64_t)(free_b / 4 / 8);
    return SSDE_OK;
}

// how every *_single opens: on the handle's device, with stream 0 drained of what the caller left there
int open_call(ssde_handle* h) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(0));
    return SSDE_OK;
}

// a call that places by track needs the ordinal of every lane's track
int check_track_ordinals(ssde_handle* h, int64_t n_lanes, const char* who) {
    return (int64_t)h->lane_seg.n >= n_lanes ? SSDE_OK : refuse(h, SSDE_ERR_ARG, std::string(who) + ": the handle holds no track ordinals for its lanes");
}

// The record-producing half of every call of this file: the parameter vector, the groups' record offsets, the chunk plan under
// the budget, the record buffer and the forward launch's arguments.  produce(c) fills the buffer with chunk c's records and leaves
// `s` addressing them.
struct RecordRun {
    ssde_handle* h = nullptr;
    bool tv = false, have_records = false;
    int R = 0;
    int64_t nt = 0, n_lanes = 0, budget = 0;
    int SW = 0;                        // > 0 (set before setup): the record pass also writes side rows of SW doubles (ssde_predict) ...
    int side_kind = 0;                 // ... of this kind (ssde_records.hpp: 0 ssde_predict's, REC_SIDE_AHEAD ssde_forecast_scores')
    // set before setup: the doubles the call keeps per group beside its records and side rows, from the group's state rows; the
    // chunks are then cut on the groups' whole cost
    std::function<int64_t(int64_t)> extra;
    std::vector<int64_t> gsteps;       // the groups' state rows (their longest track's)
    DevBuf<double> rec, pbuf, side;
    DevBuf<int64_t> offb;
    DevBuf<SlotTable> stb;
    std::vector<int64_t> goff;
    std::vector<int> cut;
    SmoothArgs s;
    TvArgs ta;
    DenseArgs da;
    ~RecordRun() { rec.release(); pbuf.release(); side.release(); offb.release(); stb.release(); }
    size_t n_chunks() const { return cut.size() - 1; }
    // rows of the layout the kernels write
    static int64_t rows(const ssde_handle* h) { return (h->path != PATH_TV && h->n_pad > 0) ? h->n_pad : h->n; }

    int setup(ssde_handle* h_, const double* par, const char* who) {
        h = h_;
        const int d = h->d;
        R = smooth_rec_doubles(h->model, d);
        if (R <= 0) { h->err = std::string(who) + ": no smoother for this response width"; return SSDE_ERR_MODEL; }
        tv = h->path == PATH_TV;
        nt = rows(h);
        HIPCHK(h, pbuf.upload(std::vector<double>(par, par + h->L.n_full)));

        // the groups' record offsets (doubles; 64-bit throughout)
        std::vector<int32_t> glen;
        if (tv) {
            std::vector<int32_t> ns((size_t)h->n_seg);
            if (h->n_seg) HIPCHK(h, hipMemcpy(ns.data(), h->tv_ns.p, (size_t)h->n_seg * 4, hipMemcpyDeviceToHost));
            n_lanes = h->n_seg;
            for (int64_t t = 0; t < h->n_seg; t += WAVE) {
                int32_t m = 0;
                for (int64_t k = t; k < std::min<int64_t>(t + WAVE, h->n_seg); k++) m = std::max(m, ns[k]);
                glen.push_back(m);
            }
        } else {
            glen.resize((size_t)h->n_groups);
            if (h->n_groups) HIPCHK(h, hipMemcpy(glen.data(), h->group_len.p, (size_t)h->n_groups * 4, hipMemcpyDeviceToHost));
            n_lanes = (int64_t)h->n_groups * WAVE;
        }
        const int G = (int)glen.size();
        goff.assign((size_t)G + 1, 0);
        for (int g = 0; g < G; g++) goff[g + 1] = goff[g] + (int64_t)glen[g] * R * WAVE;
        gsteps.assign(glen.begin(), glen.end());
        HIPCHK(h, offb.upload(goff));
        if (h->smooth_budget_mb > 0) budget = h->smooth_budget_mb * (int64_t)(1 << 20) / 8;
        else if (int st = free_budget(h, budget)) return st;
        if (extra) {
            std::vector<int64_t> cost((size_t)G + 1, 0);
            for (int g = 0; g < G; g++) cost[g + 1] = cost[g] + (int64_t)glen[g] * (R + SW) * WAVE + extra(glen[g]);
            cut = chunk_groups(cost, budget);
        } else {
            if (SW > 0) budget = budget / (R + SW) * R;            // the side rows share the budget
            cut = chunk_groups(goff, budget);
        }
        int64_t biggest = 0;
        for (size_t c = 0; c + 1 < cut.size(); c++) biggest = std::max(biggest, goff[cut[c + 1]] - goff[cut[c]]);
        HIPCHK(h, rec.alloc((size_t)std::max<int64_t>(biggest, 1)));
        if (SW > 0) HIPCHK(h, side.alloc((size_t)std::max<int64_t>(biggest / R * SW, 1)));

        memset(&s, 0, sizeof(s));
        s.model = h->model; s.d = d; s.rc.rec = rec.p; s.rc.side = side.p; s.rc.side_kind = side_kind; s.rc.rec_off = offb.p;
        s.n_out = nt; s.n_lanes = n_lanes;
        if (tv) {
            tv_base_args(h, ta);
            ta.par = pbuf.p;
            const double sig = exp(par[0]);
            ta.h = sig * sig;
            s.lane_row0 = h->tv_row0.p; s.lane_ns = h->tv_ns.p;
        } else {
            const SlotTable stab = value_slot_table(h);
            HIPCHK(h, stb.upload(std::vector<SlotTable>(1, stab)));
            dense_base_args(h, da);
            da.slots = stb.p; da.par = pbuf.p; da.n_slots = stab.n_slots;
            da.n_dirblocks = 1; da.pp = h->pp_drift; da.n = nt;
            s.lane_row0 = h->lane_row0.p; s.lane_ns = h->lane_nsteps.p;
        }
        return SSDE_OK;
    }

    int produce(size_t c) {
        s.rc.g0 = cut[c]; s.rc.n_groups = cut[c + 1] - cut[c]; s.rc.rec_base = goff[cut[c]];
        if (tv) {
            HIPCHK(h, launch_smooth_tv_record(ta, s, 0));
        } else {
            da.rc = s.rc;
            HIPCHK(h, launch_dense(da, false, 0));
        }
        return SSDE_OK;
    }

    // chunk c's records for one batch of a call that draws: produced once when there is one chunk, per batch otherwise
    int produce_for_batch(size_t c) {
        if (have_records && n_chunks() == 1) return SSDE_OK;
        have_records = true;
        return produce(c);
    }
};

// The budget for the batches of a call that draws, asked again: what is free now, beside the records and the call's tables (a set
// SSDE_OPT_SMOOTH_BUDGET_MB stands as the run has it).  The calls that size their batches by run.budget instead say so.
int batch_budget(ssde_handle* h, const RecordRun& run, int64_t& budget) {
    budget = run.budget;
    return h->smooth_budget_mb <= 0 ? free_budget(h, budget) : SSDE_OK;
}

// The batches of a call that draws, over the chunks of its run.  Per batch of at most nb_cap draws: begin(k0, nb) (the preset of the
// batch's output), d's draw range, then per chunk chunk(c, ready) -- which may return before it calls ready() to skip a chunk that
// has nothing to do; ready() produces the chunk's records (once per call where there is one chunk) and points d.s at them, after
// which the callable launches -- and end(k0, nb) (the copy home, or the consumer).  k0: the batch's first draw within the call.
template <class Begin, class Chunk, class End>
int walk_batches(RecordRun& run, DrawArgs& d, int64_t draw0, int n_draws, int nb_cap, Begin begin, Chunk chunk, End end) {
    for (int k0 = 0; k0 < n_draws; k0 += nb_cap) {
        const int nb = std::min(nb_cap, n_draws - k0);
        if (int st = begin(k0, nb)) return st;
        d.draw0 = (uint32_t)(draw0 + k0); d.n_draws = nb;
        for (size_t c = 0; c < run.n_chunks(); c++) {
            auto ready = [&]() -> int { const int st = run.produce_for_batch(c); d.s = run.s; return st; };
            if (int st = chunk(c, ready)) return st;
        }
        if (int st = end(k0, nb)) return st;
    }
    return SSDE_OK;
}
int no_step(int, int) { return SSDE_OK; }

// the caller's row OF each lattice row, on the device (a lattice-padded handle); p stays NULL where the rows ARE the caller's
struct RowMap {
    DevBuf<int64_t> buf;
    const int64_t* p = nullptr;
    ~RowMap() { buf.release(); }
    int make(ssde_handle* h, int64_t nt) {
        if (nt == h->n) return SSDE_OK;
        HIPCHK(h, buf.alloc((size_t)nt));
        HIPCHK(h, launch_path_row_map(h->pad_row.p, h->n, nt, buf.p, 0));
        p = buf.p;
        return SSDE_OK;
    }
};

// A per-row output [nt x ncol] of a call that walks the records back once (ssde_smooth, ssde_smooth_loo), where the caller wants
// it: preset to NaN (all bits set) where no row writes, and at the end fetched to the caller's rows (a lattice-padded handle: the
// lattice row OF each caller row) on the host.  preset() comes BEFORE the run's set-up, whose default budget is what the outputs
// leave free.  (No handle is without rows -- ssde_create refuses n < 2 -- so the guards for nt == 0 and n == 0 are for form.)
struct RowOut {
    DevBuf<double> b;
    ~RowOut() { b.release(); }
    int preset(ssde_handle* h, const double* want, int64_t nt, size_t ncol) {
        if (!want) return SSDE_OK;
        HIPCHK(h, b.alloc(std::max<size_t>((size_t)nt * ncol, 1)));
        if (nt > 0) HIPCHK(h, hipMemset(b.p, 0xff, (size_t)nt * ncol * 8));
        return SSDE_OK;
    }
    int fetch(ssde_handle* h, int64_t nt, int ncol, double* dst) {
        const int64_t n = h->n;
        if (!dst || n == 0) return SSDE_OK;
        DevBuf<double> rows;
        Release g2(rows);
        if (nt != n) {
            HIPCHK(h, rows.alloc((size_t)n * ncol));
            HIPCHK(h, launch_lattice_gather(h->pad_row.p, b.p, n, nt, ncol, rows.p, 0));
        }
        HIPCHK(h, hipMemcpy(dst, nt != n ? rows.p : b.p, (size_t)n * ncol * 8, hipMemcpyDeviceToHost));
        return SSDE_OK;
    }
};

// ---- the plans of the calls that answer queries -------------------------------------------------------------------------------
// The plan of a set of queries on one engine: the lanes' tracks in the resident layout and, on a lattice-padded handle, the lattice
// row of every caller row are read to the host; plan_queries (ssde_smooth_plan.hpp) places the queries.
int plan_engine_queries(ssde_handle* h, const RecordRun& run, const int64_t* q_row, const double* q_off, int64_t nq, QueryPlan& P) {
    const int64_t nl = run.n_lanes, n = h->n;
    std::vector<int64_t> row0((size_t)nl), prow;
    std::vector<int32_t> lns((size_t)nl);
    if (nl) {
        HIPCHK(h, hipMemcpy(row0.data(), run.s.lane_row0, (size_t)nl * 8, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(lns.data(), run.s.lane_ns, (size_t)nl * 4, hipMemcpyDeviceToHost));
    }
    if (run.nt != n) {
        prow.resize((size_t)n);
        HIPCHK(h, hipMemcpy(prow.data(), h->pad_row.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    P = plan_queries(row0, lns, run.nt != n ? prow.data() : nullptr, h->pad_step, q_row, q_off, nq);
    return SSDE_OK;
}
// the slots of chunk c of the run, and its queries
QueryRange chunk_range(const RecordRun& run, const QueryPlan& P, size_t c) { return chunk_queries(P, run.cut[c], run.cut[c + 1], WAVE); }
// the most slots of any chunk: what the per-chunk buffers are sized by
int64_t most_slots(const RecordRun& run, const QueryPlan& P) {
    int64_t most = 0;
    for (size_t c = 0; c < run.n_chunks(); c++) { const QueryRange r = chunk_range(run, P, c); most = std::max(most, r.s1 - r.s0); }
    return most;
}
// every slot's lane
std::vector<int64_t> slot_lanes(const QueryPlan& P) {
    std::vector<int64_t> slot_lane(P.want_step.size());
    for (size_t l = 0; l + 1 < P.want_off.size(); l++)
        for (int64_t i = P.want_off[l]; i < P.want_off[l + 1]; i++) slot_lane[(size_t)i] = (int64_t)l;
    return slot_lane;
}

int smooth_single(ssde_handle* h, const double* par, double* a_smooth, double* P_smooth, double* resid) {
    if (int st = open_call(h)) return st;
    const int sd = h->sdim, d = h->d;
    const int64_t nt = RecordRun::rows(h);
    RowOut am, Vm, em;
    if (int st = am.preset(h, a_smooth, nt, (size_t)sd)) return st;
    if (int st = Vm.preset(h, P_smooth, nt, (size_t)sd * sd)) return st;
    if (int st = em.preset(h, resid, nt, (size_t)d)) return st;
    RecordRun run;
    if (int st = run.setup(h, par, "ssde_smooth")) return st;
    run.s.am = am.b.p; run.s.Vm = Vm.b.p; run.s.em = em.b.p;
    for (size_t c = 0; c < run.n_chunks(); c++) {
        if (int st = run.produce(c)) return st;
        HIPCHK(h, launch_smooth_back(run.s, 0));
    }
    if (int st = am.fetch(h, nt, sd, a_smooth)) return st;
    if (int st = Vm.fetch(h, nt, sd * sd, P_smooth)) return st;
    if (int st = em.fetch(h, nt, d, resid)) return st;
    HIPCHK(h, hipStreamSynchronize(0));
    return SSDE_OK;
}

// draws [n x sdim x n_draws] of one engine, into host memory or (dev_out) HBM on the handle's device.  Draw k's matrix starts at
// draws + k * stride doubles (stride = n * sdim for a handle of its own; a column pair writes its columns into the parent's wider
// matrices).  track0: the ID segments of the shards before this one; col0: the handle's first state column in the whole state.
int draws_single(ssde_handle* h, const double* par, uint64_t seed, int64_t draw0, int n_draws, double* draws, bool dev_out,
                 int64_t stride, int64_t track0, int col0) {
    if (int st = open_call(h)) return st;
    const int sd = h->sdim;
    if (int st = check_not_coupled_wide(h, "ssde_smooth_draws")) return st;
    RecordRun run;
    if (int st = run.setup(h, par, "ssde_smooth_draws")) return st;
    const int64_t nt = run.nt, n = h->n;
    if (int st = check_track_ordinals(h, run.n_lanes, "ssde_smooth_draws")) return st;
    DevBuf<double> batch, rows;
    Release guard(batch, rows);
    // Draws per batch: what fits beside the records (batch_budget; a draw always goes).  A device output on the caller's own rows is
    // written in place; otherwise a batch is staged (and, on a lattice-padded handle, gathered to the caller's rows) before it
    // leaves.
    const bool in_place = dev_out && nt == n;
    int64_t budget = 0;
    if (int st = batch_budget(h, run, budget)) return st;
    const int nb_cap = batch_cap(budget, nt * sd, 1, DRAW_CH, n_draws);
    if (!in_place) HIPCHK(h, batch.alloc((size_t)nt * sd * nb_cap));
    if (nt != n) HIPCHK(h, rows.alloc((size_t)n * sd * nb_cap));
    DrawArgs a;
    memset(&a, 0, sizeof(a));
    a.lane_trk = h->lane_seg.p; a.track0 = track0; a.seed = seed; a.col0 = col0;
    a.draw_stride = in_place ? stride : nt * sd;
    auto begin = [&](int k0, int nb) -> int {                               // NaN (all bits set) where no state row writes
        a.out = in_place ? draws + (size_t)k0 * stride : batch.p;
        if (nt * sd > 0) HIPCHK(h, hipMemset2D(a.out, (size_t)a.draw_stride * 8, 0xff, (size_t)nt * sd * 8, (size_t)nb));
        return SSDE_OK;
    };
    auto chunk = [&](size_t, auto&& ready) -> int {
        if (int st = ready()) return st;
        HIPCHK(h, launch_smooth_draws(a, 0));
        return SSDE_OK;
    };
    auto end = [&](int k0, int nb) -> int {
        if (in_place || n * sd == 0) return SSDE_OK;
        const double* src = batch.p;
        if (nt != n) {                                                      // the lattice row OF each caller row, every draw's columns
            HIPCHK(h, launch_lattice_gather(h->pad_row.p, batch.p, n, nt, sd * nb, rows.p, 0));
            src = rows.p;
        }
        HIPCHK(h, hipMemcpy2D(draws + (size_t)k0 * stride, (size_t)stride * 8, src, (size_t)n * sd * 8, (size_t)n * sd * 8, (size_t)nb,
                              dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
        return SSDE_OK;
    };
    if (int st = walk_batches(run, a, draw0, n_draws, nb_cap, begin, chunk, end)) return st;
    HIPCHK(h, hipStreamSynchronize(0));
    return SSDE_OK;
}

// ---- ssde_path_stats ----------------------------------------------------------------------------------------------------------
// One engine's statistics [n_seg x n_stat x n_draws] into host memory: the draws' walk with the stores replaced by the reduction
// (k_path_stats.hip), batch by batch (walk_batches).  weight: the engine's own rows (host) or NULL; track0: the ID segments of the
// shards before this one (the deviates' counter only: the statistics are placed by the engine's own ordinals).
int path_single(ssde_handle* h, const double* par, uint64_t seed, int64_t draw0, int n_draws, const double* regions, int n_regions,
                const double* weight, double* stats, int64_t track0) {
    if (int st = open_call(h)) return st;
    RecordRun run;
    if (int st = run.setup(h, par, "ssde_path_stats")) return st;
    const int64_t n = h->n, n_trk = h->n_seg;
    const int n_stat = 2 + n_regions;
    if (int st = check_track_ordinals(h, run.n_lanes, "ssde_path_stats")) return st;
    if (n_trk == 0) return SSDE_OK;
    DevBuf<double> sb, wb;
    RowMap map;
    Release guard(sb, wb);
    // draws per batch: what fits the RUN's budget beside the records, in whole waves of DRAW_CH draws (one wave's draws always go)
    const size_t per_draw = (size_t)n_trk * n_stat;
    const int nb_cap = batch_cap(run.budget, (int64_t)per_draw, DRAW_CH, DRAW_CH, n_draws);
    HIPCHK(h, sb.alloc(per_draw * nb_cap));
    if (weight && n > 0) HIPCHK(h, wb.upload(std::vector<double>(weight, weight + n)));
    if (int st = map.make(h, run.nt)) return st;
    PathArgs a;
    memset(&a, 0, sizeof(a));
    a.row_map = map.p;
    a.d.lane_trk = h->lane_seg.p; a.d.track0 = track0; a.d.seed = seed; a.d.col0 = 0;
    a.weight = (weight && n > 0) ? wb.p : nullptr;
    a.stats = sb.p; a.n_trk = n_trk; a.n_regions = n_regions;
    for (int k = 0; k < 4 * n_regions; k++) a.regions[k] = regions[k];
    auto begin = [&](int, int nb) -> int {                                  // NaN (all bits set) where no lane writes
        HIPCHK(h, hipMemset(sb.p, 0xff, per_draw * nb * 8));
        return SSDE_OK;
    };
    auto chunk = [&](size_t, auto&& ready) -> int {
        if (int st = ready()) return st;
        HIPCHK(h, launch_path_stats(a, 0));
        return SSDE_OK;
    };
    auto end = [&](int k0, int nb) -> int {
        HIPCHK(h, hipMemcpy(stats + per_draw * k0, sb.p, per_draw * nb * 8, hipMemcpyDeviceToHost));
        return SSDE_OK;
    };
    if (int st = walk_batches(run, a.d, draw0, n_draws, nb_cap, begin, chunk, end)) return st;
    HIPCHK(h, hipStreamSynchronize(0));
    return SSDE_OK;
}

// The engines of a parent in turn: fn(sh, k, lo, m, track0) with the shard's first row and rows in the parent's data and the ID
// segments of the track shards before it (the column pairs of one track shard follow each other and share them).  A shard's
// failure is the parent's, with the shard's message.
template <class F>
int for_each_shard(ssde_handle* parent, F fn) {
    const size_t P = (size_t)std::max(parent->n_dim_parts, 1);
    int64_t track0 = 0;
    for (size_t k = 0; k < parent->shards.size(); k++) {
        ssde_handle* sh = parent->shards[k];
        if (int st = fn(sh, k, (int64_t)parent->shard_row0[k], (int64_t)parent->shard_nrows[k], track0)) { parent->err = sh->err; return st; }
        if ((k + 1) % P == 0) track0 += sh->n_seg;                          // the next track shard's first ordinal
    }
    return SSDE_OK;
}

// the track shards' statistics: each shard reads its own slice of the weights, counts its deviates by the GLOBAL track ordinal and
// lands at its tracks' places in the parent's array
int path_sharded(ssde_handle* parent, const double* par, uint64_t seed, int64_t draw0, int n_draws, const double* regions,
                 int n_regions, const double* weight, double* stats) {
    const int64_t N = parent->n_seg;
    const int n_stat = 2 + n_regions;
    std::fill(stats, stats + (size_t)N * n_stat * n_draws, std::numeric_limits<double>::quiet_NaN());
    return for_each_shard(parent, [&](ssde_handle* sh, size_t, int64_t lo, int64_t, int64_t track0) -> int {
        std::vector<double> t((size_t)sh->n_seg * n_stat * n_draws);
        if (int st = path_single(sh, par, seed, draw0, n_draws, regions, n_regions, weight ? weight + lo : nullptr, t.data(), track0)) return st;
        place_track_stats(stats, N, track0, t.data(), sh->n_seg, n_stat, n_draws, -1, lo);
        return SSDE_OK;
    });
}

// ---- ssde_path_speed ----------------------------------------------------------------------------------------------------------
// One engine's speed statistics [n_seg x n_stat x n_draws] and per-row counts [n x n_thr] into host memory (either may be NULL):
// ssde_path_stats' flow (batches under the RUN's budget, weights, RowMap) with k_path_speed.hip's kernel.  The counts are one device
// table of the engine's own caller rows, zeroed once per call, added to by every chunk and batch and copied home once; its bytes are
// taken off the budget before the batches are sized.
int speed_single(ssde_handle* h, const double* par, uint64_t seed, int64_t draw0, int n_draws, const double* thr, int n_thr,
                 const double* weight, double* stats, uint32_t* row_below, int64_t track0) {
    if (int st = open_call(h)) return st;
    RecordRun run;
    if (int st = run.setup(h, par, "ssde_path_speed")) return st;
    const int64_t n = h->n, n_trk = h->n_seg;
    const int n_stat = 5 + n_thr;
    if (int st = check_track_ordinals(h, run.n_lanes, "ssde_path_speed")) return st;
    if (n_trk == 0 || n == 0) return SSDE_OK;
    DevBuf<double> sb, wb;
    DevBuf<uint32_t> cb;
    RowMap map;
    Release guard(sb, wb, cb);
    const size_t n_cnt = row_below ? (size_t)n * n_thr : 0;
    // draws per batch: what fits the run's budget beside the records and the counts, in whole waves of DRAW_CH draws (one wave's
    // draws always go); a call without statistics keeps nothing per draw
    const size_t per_draw = stats ? (size_t)n_trk * n_stat : 0;
    const int64_t left = std::max<int64_t>(run.budget - (int64_t)((n_cnt * 4 + 7) / 8), 0);
    const int nb_cap = batch_cap(left, (int64_t)per_draw, DRAW_CH, DRAW_CH, n_draws);
    if (stats) HIPCHK(h, sb.alloc(per_draw * nb_cap));
    if (n_cnt) { HIPCHK(h, cb.alloc(n_cnt)); HIPCHK(h, hipMemset(cb.p, 0, n_cnt * 4)); }
    if (weight) HIPCHK(h, wb.upload(std::vector<double>(weight, weight + n)));
    if (int st = map.make(h, run.nt)) return st;
    SpeedArgs a;
    memset(&a, 0, sizeof(a));
    a.row_map = map.p;
    a.d.lane_trk = h->lane_seg.p; a.d.track0 = track0; a.d.seed = seed; a.d.col0 = 0;
    a.weight = weight ? wb.p : nullptr;
    a.stats = stats ? sb.p : nullptr; a.row_below = n_cnt ? cb.p : nullptr;
    a.n_trk = n_trk; a.n_rows = n; a.n_thr = n_thr;
    for (int k = 0; k < n_thr; k++) a.thr[k] = thr[k];
    auto begin = [&](int, int nb) -> int {                                  // NaN (all bits set) where no lane writes
        if (stats) HIPCHK(h, hipMemset(sb.p, 0xff, per_draw * nb * 8));
        return SSDE_OK;
    };
    auto chunk = [&](size_t, auto&& ready) -> int {
        if (int st = ready()) return st;
        HIPCHK(h, launch_path_speed(a, 0));
        return SSDE_OK;
    };
    auto end = [&](int k0, int nb) -> int {
        if (stats) HIPCHK(h, hipMemcpy(stats + per_draw * k0, sb.p, per_draw * nb * 8, hipMemcpyDeviceToHost));
        return SSDE_OK;
    };
    if (int st = walk_batches(run, a.d, draw0, n_draws, nb_cap, begin, chunk, end)) return st;
    if (n_cnt) HIPCHK(h, hipMemcpy(row_below, cb.p, n_cnt * 4, hipMemcpyDeviceToHost));
    HIPCHK(h, hipStreamSynchronize(0));
    return SSDE_OK;
}

// the track shards' speeds: each shard reads its own slice of the weights, counts its deviates by the GLOBAL track ordinal and lands
// at its tracks' places in the parent's statistics and at its rows' places in the parent's counts; the row of a maximum, which a
// shard counts in its own rows, is moved to the parent's rows
int speed_sharded(ssde_handle* parent, const double* par, uint64_t seed, int64_t draw0, int n_draws, const double* thr, int n_thr,
                  const double* weight, double* stats, uint32_t* row_below) {
    const int64_t N = parent->n_seg, n = parent->n;
    const int n_stat = 5 + n_thr;
    if (stats) std::fill(stats, stats + (size_t)N * n_stat * n_draws, std::numeric_limits<double>::quiet_NaN());
    if (row_below) std::fill(row_below, row_below + (size_t)n * n_thr, 0u);
    return for_each_shard(parent, [&](ssde_handle* sh, size_t, int64_t lo, int64_t, int64_t track0) -> int {
        const int64_t m = sh->n_seg, mr = sh->n;
        std::vector<double> t(stats ? (size_t)m * n_stat * n_draws : 0);
        std::vector<uint32_t> tc(row_below ? (size_t)mr * n_thr : 0, 0u);
        if (int st = speed_single(sh, par, seed, draw0, n_draws, thr, n_thr, weight ? weight + lo : nullptr, stats ? t.data() : nullptr,
                                  row_below ? tc.data() : nullptr, track0)) return st;
        if (stats) place_track_stats(stats, N, track0, t.data(), m, n_stat, n_draws, 2, lo);     // statistic 2: the row of the maximum
        for (int r = 0; row_below && r < n_thr; r++) memcpy(row_below + (size_t)n * r + lo, tc.data() + (size_t)mr * r, (size_t)mr * 4);
        return SSDE_OK;
    });
}

// ---- ssde_smooth_loo ----------------------------------------------------------------------------------------------------------
// One engine's leave-one-out outputs into host memory (each may be NULL): RowOut outputs and chunks of whole groups, as ssde_smooth,
// with k_smooth_loo.hip's kernel walking the records back.  The statistics [n_seg x n_stat] are preset to what a track without a
// served row gives (0, 0, NaN, NaN, zero counts) and written once per track by the lane that owns it; on a lattice-padded handle the
// row of a maximum is the caller's through the RowMap.
int loo_single(ssde_handle* h, const double* par, double* loo_mean, double* loo_cov, double* loo_resid, double* lpd, const double* thr,
               int n_thr, double* stats) {
    if (int st = open_call(h)) return st;
    const int d = h->d;
    const int64_t nt = RecordRun::rows(h), n_trk = h->n_seg;
    const int n_stat = 4 + n_thr;
    RowOut mb, cb, eb, lb;
    DevBuf<double> sb;
    RowMap map;
    Release guard(sb);
    if (int st = mb.preset(h, loo_mean, nt, (size_t)d)) return st;
    if (int st = cb.preset(h, loo_cov, nt, (size_t)d * d)) return st;
    if (int st = eb.preset(h, loo_resid, nt, (size_t)d)) return st;
    if (int st = lb.preset(h, lpd, nt, 1)) return st;
    if (stats && n_trk > 0) {
        HIPCHK(h, sb.alloc((size_t)n_trk * n_stat));
        HIPCHK(h, hipMemset(sb.p, 0, (size_t)n_trk * n_stat * 8));
        HIPCHK(h, hipMemset(sb.p + (size_t)n_trk * 2, 0xff, (size_t)n_trk * 2 * 8));
    }
    RecordRun run;
    if (int st = run.setup(h, par, "ssde_smooth_loo")) return st;
    if (stats) if (int st = check_track_ordinals(h, run.n_lanes, "ssde_smooth_loo")) return st;
    if (int st = map.make(h, nt)) return st;
    LooArgs a;
    memset(&a, 0, sizeof(a));
    a.row_map = map.p;
    a.lane_trk = h->lane_seg.p;
    a.mean = mb.b.p; a.cov = cb.b.p; a.resid = eb.b.p; a.lpd = lb.b.p;
    a.stats = (stats && n_trk > 0) ? sb.p : nullptr; a.n_trk = n_trk; a.n_thr = n_thr;
    for (int k = 0; k < n_thr; k++) a.thr[k] = thr[k];
    for (size_t c = 0; c < run.n_chunks(); c++) {
        if (int st = run.produce(c)) return st;
        a.s = run.s;
        HIPCHK(h, launch_smooth_loo(a, 0));
    }
    if (int st = mb.fetch(h, nt, d, loo_mean)) return st;
    if (int st = cb.fetch(h, nt, d * d, loo_cov)) return st;
    if (int st = eb.fetch(h, nt, d, loo_resid)) return st;
    if (int st = lb.fetch(h, nt, 1, lpd)) return st;
    if (stats && n_trk > 0) HIPCHK(h, hipMemcpy(stats, sb.p, (size_t)n_trk * n_stat * 8, hipMemcpyDeviceToHost));
    HIPCHK(h, hipStreamSynchronize(0));
    return SSDE_OK;
}

// ---- ssde_forecast_scores -----------------------------------------------------------------------------------------------------
// One engine's forecast scores into host memory (each output may be NULL): chunks of whole groups as ssde_smooth, over a run whose
// record pass writes ssde_ahead.hpp's side rows; per chunk k_smooth_ahead.hip's launch, one wave per (group, block of AHEAD_BLOCK
// start rows).  The per-row outputs live on the caller's rows on the device (preset to NaN; the kernel stores through the RowMap) and
// come home in one copy each.  The statistics [n_seg x n_stat x n_h] are preset to 0 (a track without a state row reaches no lane);
// each chunk's partial records are folded by the launch's second kernel.  The partial records are counted against the budget with the
// records and side rows (RecordRun::extra).
int ahead_single(ssde_handle* h, const double* par, const int32_t* hz, int n_h, double* z_ahead, double* lpd_ahead, const double* thr,
                 int n_thr, double* stats) {
    if (int st = open_call(h)) return st;
    const int d = h->d;
    const int64_t n = h->n, n_trk = h->n_seg;
    const int n_stat = 5 + n_thr, n_slot = n_h * n_stat;
    const bool sums = stats && n_trk > 0;
    DevBuf<double> zb, lb, sb, part, dt0;
    DevBuf<int64_t> bo;
    RowMap map;
    Release guard(zb, lb, sb, part, dt0, bo);
    RecordRun run;
    run.SW = ahead_side_doubles(h->model, d);
    if (run.SW <= 0) { h->err = "ssde_forecast_scores: no kernels for this model and width"; return SSDE_ERR_MODEL; }
    run.side_kind = REC_SIDE_AHEAD;
    if (sums) run.extra = [=](int64_t steps) { return ahead_partial_doubles(steps, n_h, n_stat, WAVE); };
    // (the outputs BEFORE the run's set-up, whose default budget is what they leave free)
    if (z_ahead) { HIPCHK(h, zb.alloc((size_t)n * d * n_h)); HIPCHK(h, hipMemset(zb.p, 0xff, (size_t)n * d * n_h * 8)); }
    if (lpd_ahead) { HIPCHK(h, lb.alloc((size_t)n * n_h)); HIPCHK(h, hipMemset(lb.p, 0xff, (size_t)n * n_h * 8)); }
    if (sums) { HIPCHK(h, sb.alloc((size_t)n_trk * n_slot)); HIPCHK(h, hipMemset(sb.p, 0, (size_t)n_trk * n_slot * 8)); }
    if (int st = run.setup(h, par, "ssde_forecast_scores")) return st;
    if (sums) if (int st = check_track_ordinals(h, run.n_lanes, "ssde_forecast_scores")) return st;
    if (int st = map.make(h, run.nt)) return st;
    const double* dt0p = h->lane_dt0.p;
    if (run.tv) {                                                           // PATH_TV keeps the times
        HIPCHK(h, dt0.alloc((size_t)std::max<int64_t>(run.n_lanes, 1)));
        HIPCHK(h, launch_ahead_dt0(h->times.p, run.s.lane_row0, run.n_lanes, h->n, h->last_dt, dt0.p, 0));
        dt0p = dt0.p;
    } else if ((int64_t)h->lane_dt0.n < run.n_lanes) {
        return refuse(h, SSDE_ERR_ARG, "ssde_forecast_scores: the handle holds no first intervals for its lanes");
    }
    const std::vector<int64_t> blk_off = ahead_block_offsets(run.gsteps);
    HIPCHK(h, bo.upload(blk_off));
    if (sums) {
        int64_t most = 0;
        for (size_t c = 0; c < run.n_chunks(); c++) most = std::max(most, blk_off[run.cut[c + 1]] - blk_off[run.cut[c]]);
        HIPCHK(h, part.alloc((size_t)std::max<int64_t>(most * n_slot * WAVE, 1)));
    }
    AheadArgs a;
    memset(&a, 0, sizeof(a));
    a.lane_trk = h->lane_seg.p; a.row_map = map.p; a.lane_dt0 = dt0p; a.blk_off = bo.p;
    a.z = zb.p; a.lpd = lb.p; a.part = sums ? part.p : nullptr; a.stats = sums ? sb.p : nullptr;
    a.n_rows = n; a.n_trk = n_trk; a.n_h = n_h; a.n_thr = n_thr; a.hmax = hz[n_h - 1];
    for (int j = 0; j < n_h; j++) a.hz[j] = hz[j];
    for (int k = 0; k < n_thr; k++) a.thr[k] = thr[k];
    for (size_t c = 0; c < run.n_chunks(); c++) {
        if (int st = run.produce(c)) return st;
        a.s = run.s;
        a.blk_base = blk_off[run.cut[c]];
        int64_t mb = 0;
        for (int g = run.cut[c]; g < run.cut[c + 1]; g++) mb = std::max(mb, blk_off[g + 1] - blk_off[g]);
        a.max_blocks = (int)std::min<int64_t>(mb, std::numeric_limits<int>::max());
        HIPCHK(h, launch_forecast_scores(a, 0));
    }
    if (z_ahead) HIPCHK(h, hipMemcpy(z_ahead, zb.p, (size_t)n * d * n_h * 8, hipMemcpyDeviceToHost));
    if (lpd_ahead) HIPCHK(h, hipMemcpy(lpd_ahead, lb.p, (size_t)n * n_h * 8, hipMemcpyDeviceToHost));
    if (sums) HIPCHK(h, hipMemcpy(stats, sb.p, (size_t)n_trk * n_slot * 8, hipMemcpyDeviceToHost));
    HIPCHK(h, hipStreamSynchronize(0));
    return SSDE_OK;
}

// ---- ssde_path_occupancy ------------------------------------------------------------------------------------------------------
// What the two occupancy calls share on one engine: every lane's output grid and from them every wavefront group's form, on the
// host and on the device; the accumulator [nx * ny * n_groups, then n_groups for the weight outside], zeroed once per call; the
// grid.  (The weights stay with the calls: ssde_path_occupancy quantises and uploads them piece by piece, the refined call quantises
// them on the host, where its plan reads the quanta.)
struct OccTables {
    std::vector<int32_t> lns, lgrp, grp_of;
    DevBuf<unsigned long long> acc;
    DevBuf<int32_t> lg, go;
    OccGrid grid;
    size_t n_cells = 0, n_acc = 0;
    int forms = 0;                                // the forms that ran: 1 the tile form, 2 the global form
    ~OccTables() { acc.release(); lg.release(); go.release(); }
    // on the host (the lanes' tracks and state rows are read from the device)
    int plan(ssde_handle* h, const RecordRun& run, const int32_t* group, const ssde_occ_grid& g, int n_groups, bool force_global) {
        const int64_t nl = run.n_lanes, ncell = (int64_t)g.nx * g.ny;
        std::vector<int64_t> lseg((size_t)nl);
        lns.assign((size_t)nl, 0); lgrp.assign((size_t)nl, -1);
        HIPCHK(h, hipMemcpy(lseg.data(), h->lane_seg.p, (size_t)nl * 8, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(lns.data(), run.s.lane_ns, (size_t)nl * 4, hipMemcpyDeviceToHost));
        for (int64_t l = 0; l < nl; l++)
            if (lns[l] > 0 && lseg[l] >= 0 && lseg[l] < h->n_seg) lgrp[l] = group ? group[lseg[l]] : 0;
        grp_of = plan_occ_groups(lgrp, WAVE, ncell, OCC_TILE_CELLS, force_global, OCC_GROUP_MIXED);
        grid.x0 = g.x0; grid.dx = g.dx; grid.y0 = g.y0; grid.dy = g.dy; grid.nx = g.nx; grid.ny = g.ny;
        n_cells = (size_t)ncell * n_groups; n_acc = n_cells + (size_t)n_groups;
        return SSDE_OK;
    }
    int upload(ssde_handle* h) {
        HIPCHK(h, lg.upload(lgrp)); HIPCHK(h, go.upload(grp_of));
        HIPCHK(h, acc.alloc(n_acc));
        HIPCHK(h, hipMemset(acc.p, 0, n_acc * 8));
        return SSDE_OK;
    }
    template <class Args>
    void bind(Args& a) const { a.grid = grid; a.lane_grp = lg.p; a.grp_of = go.p; a.acc = acc.p; a.acc_out = acc.p + n_cells; }
    // the forms chunk c runs (a group none of whose lanes takes part runs neither), noted in `forms`
    int forms_of(const RecordRun& run, size_t c) {
        int f = 0;
        for (int g = run.cut[c]; g < run.cut[c + 1]; g++) {
            if (grp_of[g] == OCC_GROUP_MIXED) f |= 2;
            else if (grp_of[g] >= 0) f |= 1;
        }
        forms |= f;
        return f;
    }
    // home, and ADDED to the call's counts: integers, so engines, chunks and batches add up exactly
    int add_into(ssde_handle* h, std::vector<uint64_t>& counts) {
        std::vector<uint64_t> got(n_acc);
        HIPCHK(h, hipMemcpy(got.data(), acc.p, n_acc * 8, hipMemcpyDeviceToHost));
        HIPCHK(h, hipStreamSynchronize(0));
        for (size_t i = 0; i < n_acc; i++) counts[i] += got[i];
        return SSDE_OK;
    }
};

// One engine's occupancy counts, ADDED to `counts` [nx * ny * n_groups, then n_groups for the weight outside] in host memory, in
// quanta of 2^e: the draws' walk with the stores replaced by integer adds (k_path_occ.hip).  weight / group: the engine's own rows /
// tracks (host) or NULL; track0 as ssde_path_stats'.  The counts are integers, so chunks, batches and shards add up exactly.
int occ_single(ssde_handle* h, const double* par, uint64_t seed, int64_t draw0, int n_draws, const ssde_occ_grid& grid,
               const double* weight, const int32_t* group, int n_groups, int e, bool force_global, std::vector<uint64_t>& counts,
               int64_t track0) {
    if (int st = open_call(h)) return st;
    RecordRun run;
    if (int st = run.setup(h, par, "ssde_path_occupancy")) return st;
    const int64_t n = h->n, nl = run.n_lanes;
    if (int st = check_track_ordinals(h, nl, "ssde_path_occupancy")) return st;
    h->last_occ_form = 0;
    if (h->n_seg == 0 || nl == 0) return SSDE_OK;
    OccTables T;
    if (int st = T.plan(h, run, group, grid, n_groups, force_global)) return st;
    DevBuf<uint64_t> wb;
    RowMap map;
    Release guard(wb);
    OccArgs a;
    memset(&a, 0, sizeof(a));
    if (weight && n > 0) {                                              // quantised and uploaded piece by piece: no second [n] array on the host
        const int64_t piece = (int64_t)1 << 20;
        std::vector<uint64_t> wq((size_t)std::min(n, piece));
        HIPCHK(h, wb.alloc((size_t)n));
        for (int64_t i0 = 0; i0 < n; i0 += piece) {
            const int64_t m = std::min(piece, n - i0);
            occ_quantise_all(weight + i0, m, e, wq.data());
            HIPCHK(h, hipMemcpy(wb.p + i0, wq.data(), (size_t)m * 8, hipMemcpyHostToDevice));
        }
        a.wq = wb.p;
    }
    a.unit = occ_quantise(1.0, e);
    if (int st = T.upload(h)) return st;
    if (int st = map.make(h, run.nt)) return st;
    a.row_map = map.p;
    a.d.lane_trk = h->lane_seg.p; a.d.track0 = track0; a.d.seed = seed; a.d.col0 = 0;
    T.bind(a);
    // draws per batch: the call keeps nothing per draw, so no budget enters
    const int nb_cap = occ_batch_cap(OCC_NW, DRAW_CH, n_draws);
    auto chunk = [&](size_t c, auto&& ready) -> int {
        if (int st = ready()) return st;
        const int forms = T.forms_of(run, c);
        if (forms & 1) HIPCHK(h, launch_path_occ(a, true, 0));
        if (forms & 2) HIPCHK(h, launch_path_occ(a, false, 0));
        return SSDE_OK;
    };
    if (int st = walk_batches(run, a.d, draw0, n_draws, nb_cap, no_step, chunk, no_step)) return st;
    if (int st = T.add_into(h, counts)) return st;
    h->last_occ_form = T.forms;
    return SSDE_OK;
}

// the track shards' counts: each shard reads its own slice of the weights and of the groups, counts its deviates by the GLOBAL track
// ordinal and adds into the same integers; the quantum is the parent's
int occ_sharded(ssde_handle* parent, const double* par, uint64_t seed, int64_t draw0, int n_draws, const ssde_occ_grid& grid,
                const double* weight, const int32_t* group, int n_groups, int e, bool force_global, std::vector<uint64_t>& counts) {
    return for_each_shard(parent, [&](ssde_handle* sh, size_t, int64_t lo, int64_t, int64_t track0) -> int {
        return occ_single(sh, par, seed, draw0, n_draws, grid, weight ? weight + lo : nullptr, group ? group + track0 : nullptr, n_groups, e,
                          force_global, counts, track0);
    });
}

// ---- ssde_path_occupancy_fine -------------------------------------------------------------------------------------------------
// The interval the handle holds for every slot of plan_all_slots' lists (lane-major, steps ascending), read once on the host: the one
// interval of a globally regular grid (on a lattice-padded handle: of the lattice), else the tiles' dt channel; on PATH_TV the
// differences of the times.  A lane's last step has no interval to the next row; its entry is not read.
int slot_intervals(ssde_handle* h, const RecordRun& run, const QueryPlan& P, const std::vector<int64_t>& row0, std::vector<double>& dt) {
    const int64_t nl = run.n_lanes, n_slots = (int64_t)P.want_step.size();
    dt.assign((size_t)n_slots, 0.0);
    if (n_slots == 0) return SSDE_OK;
    if (run.tv) {
        std::vector<double> tm((size_t)h->n);
        HIPCHK(h, hipMemcpy(tm.data(), h->times.p, (size_t)h->n * 8, hipMemcpyDeviceToHost));
        for (int64_t l = 0; l < nl; l++)
            for (int64_t i = P.want_off[l]; i < P.want_off[l + 1]; i++) {
                const int64_t row = row0[l] + 1 + (i - P.want_off[l]);
                dt[(size_t)i] = row + 1 < h->n ? tm[(size_t)row + 1] - tm[(size_t)row] : h->last_dt;
            }
        return SSDE_OK;
    }
    if (h->c_obs == 0) { std::fill(dt.begin(), dt.end(), h->dt_all); return SSDE_OK; }
    // channel 0 of every tile row: group g's rows start at the sum of the group lengths before it
    std::vector<int32_t> glen((size_t)h->n_groups);
    HIPCHK(h, hipMemcpy(glen.data(), h->group_len.p, (size_t)h->n_groups * 4, hipMemcpyDeviceToHost));
    std::vector<int64_t> grow((size_t)h->n_groups + 1, 0);
    for (int g = 0; g < h->n_groups; g++) grow[g + 1] = grow[g] + glen[g];
    std::vector<double> ch((size_t)grow[h->n_groups] * WAVE);
    if (!ch.empty())
        HIPCHK(h, hipMemcpy2D(ch.data(), (size_t)WAVE * 8, h->tiles.p, (size_t)h->C * WAVE * 8, (size_t)WAVE * 8, (size_t)grow[h->n_groups],
                              hipMemcpyDeviceToHost));
    // (in the tiles' order, step by step over a group's 64 lanes: the 80 MB of a large handle are read once, front to back)
    for (int g = 0; g < h->n_groups; g++)
        for (int64_t s = 0; s < glen[g]; s++) {
            const double* row = ch.data() + (size_t)(grow[g] + s) * WAVE;
            for (int64_t l = (int64_t)g * WAVE; l < std::min<int64_t>((int64_t)(g + 1) * WAVE, nl); l++)
                if (s < P.want_off[l + 1] - P.want_off[l]) dt[(size_t)(P.want_off[l] + s)] = row[l - (int64_t)g * WAVE];
        }
    return SSDE_OK;
}

// One engine's refined occupancy counts, ADDED to `counts`, and its two counts of ssde_last_occupancy_points added to n_points /
// n_capped.  OccTables over a run with side rows: chunks without a slot are skipped, the batches come from occ_fine_batch_cap; per
// batch and chunk the draws' walk that leaves the ends of every slot, then path_occ_fine_kernel.
int occ_fine_single(ssde_handle* h, const double* par, uint64_t seed, int64_t draw0, int n_draws, const ssde_occ_grid& grid,
                    double max_step, const double* weight, const int32_t* group, int n_groups, int e, bool force_global,
                    std::vector<uint64_t>& counts, int64_t& n_points, int64_t& n_capped, int64_t track0) {
    if (int st = open_call(h)) return st;
    RecordRun run;
    run.SW = predict_side_doubles(h->model, h->d);
    if (run.SW <= 0) { h->err = "ssde_path_occupancy_fine: no kernels for this model and width"; return SSDE_ERR_MODEL; }
    if (int st = run.setup(h, par, "ssde_path_occupancy_fine")) return st;
    const int64_t nt = run.nt, n = h->n, nl = run.n_lanes;
    const int ez = 2 * h->sdim;
    if (int st = check_track_ordinals(h, nl, "ssde_path_occupancy_fine")) return st;
    h->last_occ_form = 0; h->last_occ_points = 0; h->last_occ_capped = 0;
    if (h->n_seg == 0 || nl == 0) return SSDE_OK;
    // every lane's output grid, every wavefront group's form, every slot
    OccTables T;
    if (int st = T.plan(h, run, group, grid, n_groups, force_global)) return st;
    std::vector<int64_t> row0((size_t)nl), rmap;
    HIPCHK(h, hipMemcpy(row0.data(), run.s.lane_row0, (size_t)nl * 8, hipMemcpyDeviceToHost));
    const QueryPlan P = plan_all_slots(T.lns, T.lgrp);
    if (P.want_step.empty()) return SSDE_OK;
    std::vector<double> sdt;
    if (int st = slot_intervals(h, run, P, row0, sdt)) return st;
    RowMap map;
    DevBuf<uint64_t> ob, sb;
    DevBuf<int32_t> mb, ws;
    DevBuf<int64_t> wo, sl;
    DevBuf<double> ends, sidepk;
    Release guard(ob, sb, mb, ws, wo, sl, ends, sidepk);
    if (int st = map.make(h, nt)) return st;
    if (map.p) {                                                        // ... for the host plan
        rmap.resize((size_t)nt);
        HIPCHK(h, hipMemcpy(rmap.data(), map.p, (size_t)nt * 8, hipMemcpyDeviceToHost));
    }
    std::vector<uint64_t> wq;
    if (weight && n > 0) { wq.resize((size_t)n); occ_quantise_all(weight, n, e, wq.data()); }
    const FineWeights F = plan_fine_weights(P, row0, sdt, max_step, SSDE_OCC_MAX_SUB, map.p ? rmap.data() : nullptr,
                                            wq.empty() ? nullptr : wq.data(), occ_quantise(1.0, e));
    std::vector<uint64_t>().swap(wq);
    sdt = std::vector<double>();
    const int64_t most = most_slots(run, P);
    HIPCHK(h, wo.upload(P.want_off)); HIPCHK(h, ws.upload(P.want_step)); HIPCHK(h, sl.upload(slot_lanes(P)));
    HIPCHK(h, mb.upload(F.m)); HIPCHK(h, ob.upload(F.own)); HIPCHK(h, sb.upload(F.share));
    if (int st = T.upload(h)) return st;
    // draws per batch: what fits beside the records, side rows and tables (batch_budget)
    int64_t budget = 0;
    if (int st = batch_budget(h, run, budget)) return st;
    const int nb_cap = occ_fine_batch_cap(budget, most, ez, DRAW_CH, n_draws);
    HIPCHK(h, ends.alloc((size_t)most * ez * nb_cap));
    HIPCHK(h, sidepk.alloc((size_t)most * run.SW));
    OccFineArgs a;
    memset(&a, 0, sizeof(a));
    a.p.d.lane_trk = h->lane_seg.p; a.p.d.track0 = track0; a.p.d.seed = seed; a.p.d.col0 = 0;
    a.p.want_off = wo.p; a.p.want_step = ws.p; a.p.ends = ends.p; a.p.sidepk = sidepk.p; a.p.slot_lane = sl.p;
    a.m = mb.p; a.own = ob.p; a.share = sb.p;
    T.bind(a);
    auto chunk = [&](size_t c, auto&& ready) -> int {
        const QueryRange r = chunk_range(run, P, c);
        if (r.s1 == r.s0) return SSDE_OK;                                 // no slot on this chunk's tracks
        if (int st = ready()) return st;
        a.p.slot0 = r.s0; a.p.pk_stride = r.s1 - r.s0;
        const int forms = T.forms_of(run, c);
        HIPCHK(h, launch_predict_draws_walk(a.p, 0));
        if (forms & 1) HIPCHK(h, launch_path_occ_fine(a, true, 0));
        if (forms & 2) HIPCHK(h, launch_path_occ_fine(a, false, 0));
        return SSDE_OK;
    };
    if (int st = walk_batches(run, a.p.d, draw0, n_draws, nb_cap, no_step, chunk, no_step)) return st;
    if (int st = T.add_into(h, counts)) return st;
    h->last_occ_form = T.forms; h->last_occ_points = F.n_points; h->last_occ_capped = F.n_capped;
    n_points += F.n_points; n_capped += F.n_capped;
    return SSDE_OK;
}

// the track shards' refined counts, as occ_sharded: slices of the weights and groups, the GLOBAL track ordinal in the deviates, the
// parent's quantum; integer grids and the two counts add up
int occ_fine_sharded(ssde_handle* parent, const double* par, uint64_t seed, int64_t draw0, int n_draws, const ssde_occ_grid& grid,
                     double max_step, const double* weight, const int32_t* group, int n_groups, int e, bool force_global,
                     std::vector<uint64_t>& counts, int64_t& n_points, int64_t& n_capped) {
    return for_each_shard(parent, [&](ssde_handle* sh, size_t, int64_t lo, int64_t, int64_t track0) -> int {
        return occ_fine_single(sh, par, seed, draw0, n_draws, grid, max_step, weight ? weight + lo : nullptr, group ? group + track0 : nullptr,
                               n_groups, e, force_global, counts, n_points, n_capped, track0);
    });
}

// ---- ssde_predict -------------------------------------------------------------------------------------------------------------
// One engine's queries.  plan_queries (ssde_smooth_plan.hpp) places them on the host; then, chunk by chunk: the record pass with side
// rows, the walk that fills the chunk's packets, the query kernel.
int predict_single(ssde_handle* h, const double* par, const int64_t* q_row, const double* q_off, int64_t nq, double* a_pred,
                   double* P_pred) {
    if (int st = open_call(h)) return st;
    const int sd = h->sdim;
    if (int st = check_not_coupled_wide(h, "ssde_predict")) return st;
    RecordRun run;
    run.SW = predict_side_doubles(h->model, h->d);
    const int PKD = predict_packet_doubles(h->model, h->d);
    if (run.SW <= 0 || PKD <= 0) { h->err = "ssde_predict: no kernels for this model and width"; return SSDE_ERR_MODEL; }
    if (int st = run.setup(h, par, "ssde_predict")) return st;
    QueryPlan P;
    if (int st = plan_engine_queries(h, run, q_row, q_off, nq, P)) return st;

    // the outputs, NaN (all bits set) where no query writes
    DevBuf<double> am, Vm, pk, offd;
    DevBuf<int64_t> wo, ord, qs;
    DevBuf<int32_t> ws;
    Release guard(am, Vm, pk, offd, wo, ord, qs, ws);
    HIPCHK(h, am.alloc((size_t)nq * sd)); HIPCHK(h, hipMemset(am.p, 0xff, (size_t)nq * sd * 8));
    if (P_pred) { HIPCHK(h, Vm.alloc((size_t)nq * sd * sd)); HIPCHK(h, hipMemset(Vm.p, 0xff, (size_t)nq * sd * sd * 8)); }
    if (!P.order.empty()) {
        HIPCHK(h, wo.upload(P.want_off)); HIPCHK(h, ws.upload(P.want_step));
        HIPCHK(h, ord.upload(P.order)); HIPCHK(h, qs.upload(P.q_slot)); HIPCHK(h, offd.upload(P.off));
        HIPCHK(h, pk.alloc((size_t)most_slots(run, P) * PKD));
        PredictArgs a;
        memset(&a, 0, sizeof(a));
        a.want_off = wo.p; a.want_step = ws.p; a.pk = pk.p; a.order = ord.p; a.q_slot = qs.p; a.q_off = offd.p;
        a.n_query = nq; a.a_pred = am.p; a.P_pred = Vm.p;
        for (size_t c = 0; c < run.n_chunks(); c++) {
            const QueryRange r = chunk_range(run, P, c);
            if (r.s1 == r.s0) continue;                             // no query on this chunk's tracks
            if (int st = run.produce(c)) return st;
            a.s = run.s;
            a.slot0 = r.s0; a.pk_stride = r.s1 - r.s0; a.q0 = r.q0; a.q1 = r.q1;
            HIPCHK(h, launch_predict_walk(a, 0));
            HIPCHK(h, launch_predict_query(a, 0));
        }
    }
    HIPCHK(h, hipMemcpy(a_pred, am.p, (size_t)nq * sd * 8, hipMemcpyDeviceToHost));
    if (P_pred) HIPCHK(h, hipMemcpy(P_pred, Vm.p, (size_t)nq * sd * sd * 8, hipMemcpyDeviceToHost));
    HIPCHK(h, hipStreamSynchronize(0));
    return SSDE_OK;
}

// the shards' and column pairs' queries: each engine gets the queries on its rows, its columns land in the parent's layout
int predict_sharded(ssde_handle* parent, const double* par, const int64_t* q_row, const double* q_off, int64_t nq, double* a_pred,
                    double* P_pred) {
    const int SD = parent->sdim;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::fill(a_pred, a_pred + (size_t)nq * SD, nan);
    if (P_pred) std::fill(P_pred, P_pred + (size_t)nq * SD * SD, 0.0);           // cross-pair blocks: zero
    return for_each_shard(parent, [&](ssde_handle* sh, size_t k, int64_t lo, int64_t m, int64_t) -> int {
        const int sd = sh->sdim, c0 = parent->shard_col0[k];
        const QueryDeal D = deal_queries(lo, m, q_row, q_off, nq);
        const int64_t mq = (int64_t)D.idx.size();
        if (mq == 0) return SSDE_OK;
        std::vector<double> ta((size_t)mq * sd), tP(P_pred ? (size_t)mq * sd * sd : 0);
        if (int st = ssde_predict(sh, par, parent->L.n_full, D.rows.data(), D.offs.data(), mq, ta.data(), P_pred ? tP.data() : nullptr)) return st;
        place_columns(a_pred, nq, c0, ta.data(), mq, sd, 0, D.idx.data());
        if (P_pred) place_cov_block(P_pred, nq, SD, c0, tP.data(), mq, sd, 0, D.idx.data());   // (a query without a state: no covariance at all)
        return SSDE_OK;
    });
}

// ---- ssde_predict_draws -------------------------------------------------------------------------------------------------------
// One engine's queries for n_draws draws into host memory [nq x sdim x n_draws].  plan_engine_queries over a run with side rows,
// chunks without a query skipped, batch by batch (walk_batches): per batch and chunk the walk that stores the ends of the wanted
// intervals, then the query kernel.  track0 / col0 as ssde_smooth_draws'.
// A call that reduces the states on the device (ssde_path_proximity) passes a consumer: after the chunk loop of a batch `out` holds
// every query of that batch of draws, and instead of the copy home the consumer gets (out [nq x sdim x nb], the batch's first draw
// within the call, nb, the most draws a batch of this call holds); out == NULL: no query of the call has a state, every element of all
// n_draws draws is NaN.  extra_per_draw: the doubles per draw the consumer keeps on this device, accounted for in the batch cap.
typedef std::function<int(const double* out, int k0, int nb, int nb_cap)> BatchConsumer;
int predict_draws_single(ssde_handle* h, const double* par, const int64_t* q_row, const double* q_off, int64_t nq, uint64_t seed,
                         int64_t draw0, int n_draws, double* draws_at, int64_t track0, int col0,
                         const BatchConsumer* consume = nullptr, int64_t extra_per_draw = 0) {
    if (int st = open_call(h)) return st;
    const int sd = h->sdim;
    if (int st = check_not_coupled_wide(h, "ssde_predict_draws")) return st;
    RecordRun run;
    run.SW = predict_side_doubles(h->model, h->d);
    if (run.SW <= 0) { h->err = "ssde_predict_draws: no kernels for this model and width"; return SSDE_ERR_MODEL; }
    if (int st = run.setup(h, par, "ssde_predict_draws")) return st;
    if (int st = check_track_ordinals(h, run.n_lanes, "ssde_predict_draws")) return st;
    QueryPlan P;
    if (int st = plan_engine_queries(h, run, q_row, q_off, nq, P)) return st;
    const SlotOffsets S = plan_slot_offsets(P);
    if (S.most >= ((int64_t)1 << 32)) { h->err = "ssde_predict_draws: an interval with 2^32 or more distinct offsets"; return SSDE_ERR_ARG; }
    const size_t per_draw = (size_t)nq * sd;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (P.order.empty()) {
        if (consume) return (*consume)(nullptr, 0, n_draws, n_draws);
        std::fill(draws_at, draws_at + per_draw * n_draws, nan);
        return SSDE_OK;
    }

    const int64_t most = most_slots(run, P);
    DevBuf<double> out, ends, sidepk, offv;
    DevBuf<int64_t> wo, sl, op, qp, qd;
    DevBuf<int32_t> ws;
    Release guard(out, ends, sidepk, offv, wo, sl, op, qp, qd, ws);
    HIPCHK(h, wo.upload(P.want_off)); HIPCHK(h, ws.upload(P.want_step)); HIPCHK(h, sl.upload(slot_lanes(P)));
    HIPCHK(h, op.upload(S.off_ptr)); HIPCHK(h, offv.upload(S.off_val)); HIPCHK(h, qp.upload(S.q_ptr)); HIPCHK(h, qd.upload(S.q_dest));
    // draws per batch: what fits beside the records, side rows and tables (batch_budget)
    int64_t budget = 0;
    if (int st = batch_budget(h, run, budget)) return st;
    const int nb_cap = consume ? batch_cap(budget, most * 2 * sd + nq * sd + extra_per_draw, 1, DRAW_CH, n_draws)
                               : predict_draws_batch_cap(budget, most, sd, nq, DRAW_CH, n_draws);
    HIPCHK(h, out.alloc(per_draw * nb_cap));
    HIPCHK(h, ends.alloc((size_t)most * 2 * sd * nb_cap));
    HIPCHK(h, sidepk.alloc((size_t)most * run.SW));
    PredictDrawArgs a;
    memset(&a, 0, sizeof(a));
    a.d.lane_trk = h->lane_seg.p; a.d.track0 = track0; a.d.seed = seed; a.d.col0 = col0;
    a.want_off = wo.p; a.want_step = ws.p; a.ends = ends.p; a.sidepk = sidepk.p; a.slot_lane = sl.p;
    a.off_ptr = op.p; a.off_val = offv.p; a.q_ptr = qp.p; a.q_dest = qd.p; a.n_query = nq; a.out = out.p;
    auto begin = [&](int, int nb) -> int {                                  // NaN (all bits set) where no query writes
        HIPCHK(h, hipMemset(out.p, 0xff, per_draw * nb * 8));
        return SSDE_OK;
    };
    auto chunk = [&](size_t c, auto&& ready) -> int {
        const QueryRange r = chunk_range(run, P, c);
        if (r.s1 == r.s0) return SSDE_OK;                                 // no query on this chunk's tracks
        if (int st = ready()) return st;
        a.slot0 = r.s0; a.pk_stride = r.s1 - r.s0;
        HIPCHK(h, launch_predict_draws_walk(a, 0));
        HIPCHK(h, launch_predict_draws_query(a, 0));
        return SSDE_OK;
    };
    auto end = [&](int k0, int nb) -> int {
        if (consume) return (*consume)(out.p, k0, nb, nb_cap);
        HIPCHK(h, hipMemcpy(draws_at + per_draw * k0, out.p, per_draw * nb * 8, hipMemcpyDeviceToHost));
        return SSDE_OK;
    };
    if (int st = walk_batches(run, a.d, draw0, n_draws, nb_cap, begin, chunk, end)) return st;
    HIPCHK(h, hipStreamSynchronize(0));
    return SSDE_OK;
}

// the shards' and column pairs' queries: each engine gets the queries on its rows (deal_queries), counts its deviates by the GLOBAL
// track ordinal and state column and its columns land in the parent's layout (place_columns)
int predict_draws_sharded(ssde_handle* parent, const double* par, const int64_t* q_row, const double* q_off, int64_t nq, uint64_t seed,
                          int64_t draw0, int n_draws, double* draws_at) {
    const int SD = parent->sdim;
    std::fill(draws_at, draws_at + (size_t)nq * SD * n_draws, std::numeric_limits<double>::quiet_NaN());
    return for_each_shard(parent, [&](ssde_handle* sh, size_t k, int64_t lo, int64_t m, int64_t track0) -> int {
        const int sd = sh->sdim, c0 = parent->shard_col0[k];
        const QueryDeal D = deal_queries(lo, m, q_row, q_off, nq);
        const int64_t mq = (int64_t)D.idx.size();
        if (mq == 0) return SSDE_OK;
        std::vector<double> t((size_t)mq * sd * n_draws);
        if (int st = check_kalman(sh)) return st;
        if (int st = predict_draws_single(sh, par, D.rows.data(), D.offs.data(), mq, seed, draw0, n_draws, t.data(), track0, c0)) return st;
        for (int q = 0; q < n_draws; q++)
            place_columns(draws_at + (size_t)nq * SD * q, nq, c0, t.data() + (size_t)mq * sd * q, mq, sd, 0, D.idx.data());
        return SSDE_OK;
    });
}

// ---- ssde_path_proximity ------------------------------------------------------------------------------------------------------
// What both routes share: the call as the host sees it, and the two kernels' tables, partial records and statistics on one device.
struct ProxCall {
    int64_t n_point = 0;
    int n_pairs = 0, n_radii = 0, n_stat = 2, e = 0;
    const double* radii = nullptr;
    std::vector<uint64_t> wq;                  // the weights in quanta, quantised once on the host; empty: every point weighs `unit`
    uint64_t unit = 0;
    ProxPlan plan;
    // the doubles (64-bit words) per draw that the two kernels keep
    int64_t per_draw() const { return plan.n_tiles * PROX_REC + (int64_t)n_pairs * n_stat; }
};

struct ProxDev {
    DevBuf<int64_t> tf, ti, pt;
    DevBuf<int32_t> tc;
    DevBuf<uint64_t> wq, part;
    DevBuf<double> sb;
    ProxArgs a;
    bool ready = false;
    ~ProxDev() { tf.release(); ti.release(); pt.release(); tc.release(); wq.release(); part.release(); sb.release(); }
    // on the CURRENT device: the tables, and room for nb_cap draws
    int prepare(ssde_handle* h, const ProxCall& c, int nb_cap) {
        if (ready) return SSDE_OK;
        HIPCHK(h, tf.upload(c.plan.tile_first)); HIPCHK(h, ti.upload(c.plan.tile_idx0)); HIPCHK(h, tc.upload(c.plan.tile_count));
        HIPCHK(h, pt.upload(c.plan.pair_tile)); HIPCHK(h, wq.upload(c.wq));
        HIPCHK(h, part.alloc((size_t)c.plan.n_tiles * PROX_REC * nb_cap));
        HIPCHK(h, sb.alloc((size_t)c.n_pairs * c.n_stat * nb_cap));
        memset(&a, 0, sizeof(a));
        a.model = h->model; a.d = h->d;
        a.n_point = c.n_point; a.n_query = 2 * c.n_point;
        a.tile_first = tf.p; a.tile_idx0 = ti.p; a.tile_count = tc.p; a.pair_tile = pt.p;
        a.n_tiles = c.plan.n_tiles; a.n_pairs = c.n_pairs;
        a.wq = c.wq.empty() ? nullptr : wq.p; a.unit = c.unit;
        a.part = part.p; a.stats = sb.p; a.n_radii = c.n_radii; a.e = c.e;
        for (int r = 0; r < c.n_radii; r++) a.radii[r] = c.radii[r];
        ready = true;
        return SSDE_OK;
    }
    // nb draws of positions in `pos` (n_col columns per draw; packed: the position columns alone) -> stats_host [n_pairs x n_stat x nb]
    int reduce(ssde_handle* h, const ProxCall& c, const double* pos, int n_col, bool packed, int nb, double* stats_host) {
        a.pos = pos; a.draw_stride = a.n_query * n_col; a.packed = packed ? 1 : 0; a.n_draws = nb;
        HIPCHK(h, launch_prox_tile(a, 0));
        HIPCHK(h, launch_prox_fold(a, 0));
        HIPCHK(h, hipMemcpy(stats_host, sb.p, (size_t)c.n_pairs * c.n_stat * nb * 8, hipMemcpyDeviceToHost));
        return SSDE_OK;
    }
};

// route 1: one engine; the positions of a batch never leave its device
int prox_single(ssde_handle* h, const double* par, const int64_t* q_row, const double* q_off, const ProxCall& c, uint64_t seed,
                int64_t draw0, int n_draws, double* stats, int& n_batches) {
    ProxDev dev;
    const size_t per = (size_t)c.n_pairs * c.n_stat;
    const BatchConsumer consume = [&](const double* out, int k0, int nb, int nb_cap) -> int {
        if (!out) { std::fill(stats, stats + per * n_draws, std::numeric_limits<double>::quiet_NaN()); n_batches = 1; return SSDE_OK; }
        if (int st = dev.prepare(h, c, nb_cap)) return st;
        n_batches++;
        return dev.reduce(h, c, out, h->sdim, false, nb, stats + per * k0);
    };
    return predict_draws_single(h, par, q_row, q_off, 2 * c.n_point, seed, draw0, n_draws, nullptr, 0, 0, &consume, c.per_draw());
}

// route 2: a multi-device parent.  Per batch of draws every track shard answers the queries on its rows (deal_queries;
// as for ssde_predict_draws the GLOBAL track ordinal in the deviates) and its position columns are gathered, on the first shard's device, into one buffer
// [2 n_point x d x nb] at the parent's query indices; the same two kernels run there.  The positions are the single engine's bit for
// bit and the reduction does not depend on where it runs, so the result is bitwise route 1's.
int prox_sharded(ssde_handle* parent, const double* par, const int64_t* q_row, const double* q_off, const ProxCall& c, uint64_t seed,
                 int64_t draw0, int n_draws, double* stats, int& n_batches) {
    const int64_t nq = 2 * c.n_point;
    const int D = parent->d, col_step = parent->model == SSDE_MODEL_CTCRW ? 2 : 1;
    ssde_handle* first = parent->shards[0];
    const int dev0 = first->device;
    const size_t per = (size_t)c.n_pairs * c.n_stat;
    // the deal, once: the queries on every shard's rows
    const size_t ns = parent->shards.size();
    std::vector<QueryDeal> deal(ns);
    for (size_t k = 0; k < ns; k++) {
        if (parent->shards[k]->sdim != parent->sdim) { parent->err = "ssde_path_proximity: column pairs are not served"; return SSDE_ERR_MODEL; }
        deal[k] = deal_queries(parent->shard_row0[k], parent->shard_nrows[k], q_row, q_off, nq);
    }
    HIPCHK(parent, hipSetDevice(dev0));
    HIPCHK(parent, hipStreamSynchronize(0));
    int64_t budget = 0;
    if (parent->smooth_budget_mb > 0) budget = parent->smooth_budget_mb * (int64_t)(1 << 20) / 8;
    else if (int st = free_budget(parent, budget)) return st;
    const int nbp = batch_cap(budget, nq * D + c.per_draw(), 1, DRAW_CH, n_draws);
    ProxDev dev;
    DevBuf<double> pos, stage;
    std::vector<DevBuf<int64_t>> idxd(ns);
    struct Free {
        DevBuf<double>&a, &b; std::vector<DevBuf<int64_t>>& v;
        ~Free() { a.release(); b.release(); for (auto& x : v) x.release(); }
    } guard{pos, stage, idxd};
    HIPCHK(parent, pos.alloc((size_t)nq * D * nbp));
    if (int st = dev.prepare(first, c, nbp)) { parent->err = first->err; return st; }
    for (size_t k = 0; k < ns; k++) HIPCHK(parent, idxd[k].upload(deal[k].idx));
    // (the parent's own batches: each shard's call walks them again inside, so this loop is not walk_batches')
    for (int k0 = 0; k0 < n_draws; k0 += nbp) {
        const int nb = std::min(nbp, n_draws - k0);
        HIPCHK(parent, hipSetDevice(dev0));
        HIPCHK(parent, hipMemset(pos.p, 0xff, (size_t)nq * D * nb * 8));     // NaN (all bits set) where no shard answers
        HIPCHK(parent, hipStreamSynchronize(0));
        const int st = for_each_shard(parent, [&](ssde_handle* sh, size_t k, int64_t, int64_t, int64_t track0) -> int {
            const int64_t mq = (int64_t)deal[k].idx.size();
            const int sd = sh->sdim;
            if (mq == 0) return SSDE_OK;
            const BatchConsumer consume = [&](const double* out, int j0, int mb, int) -> int {
                if (!out) return SSDE_OK;
                const double* src = out;
                HIPCHK(sh, hipStreamSynchronize(0));                     // the shard's batch is complete
                if (sh->device != dev0) {
                    HIPCHK(sh, hipSetDevice(dev0));
                    if (stage.n < (size_t)mq * sd * mb) { stage.release(); HIPCHK(sh, stage.alloc((size_t)mq * sd * mb)); }
                    HIPCHK(sh, hipMemcpyPeer(stage.p, dev0, out, sh->device, (size_t)mq * sd * mb * 8));
                    src = stage.p;
                }
                HIPCHK(sh, launch_prox_gather(src, mq, sd, col_step, D, mb, idxd[k].p, pos.p + (size_t)nq * D * j0, nq, 0));
                HIPCHK(sh, hipStreamSynchronize(0));
                if (sh->device != dev0) HIPCHK(sh, hipSetDevice(sh->device));
                return SSDE_OK;
            };
            if (int st = check_kalman(sh)) return st;
            return predict_draws_single(sh, par, deal[k].rows.data(), deal[k].offs.data(), mq, seed, draw0 + k0, nb, nullptr, track0, 0,
                                        &consume, 0);
        });
        if (st) return st;
        HIPCHK(parent, hipSetDevice(dev0));
        if (int st = dev.reduce(first, c, pos.p, D, true, nb, stats + per * k0)) { parent->err = first->err; return st; }
        n_batches++;
    }
    HIPCHK(parent, hipStreamSynchronize(0));
    return SSDE_OK;
}

}  // namespace

namespace ssde_engine {

int smooth_sharded(ssde_handle* parent, const double* par, double* a_smooth, double* P_smooth, double* resid) {
    const int64_t n = parent->n;
    const int SD = parent->sdim, D = parent->d, per = parent->model == SSDE_MODEL_CTCRW ? 2 : 1;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (a_smooth) std::fill(a_smooth, a_smooth + (size_t)n * SD, nan);
    if (P_smooth) std::fill(P_smooth, P_smooth + (size_t)n * SD * SD, 0.0);      // cross-pair blocks: zero
    if (resid) std::fill(resid, resid + (size_t)n * D, nan);
    return for_each_shard(parent, [&](ssde_handle* sh, size_t k, int64_t lo, int64_t m, int64_t) -> int {
        const int sd = sh->sdim, d = sh->d, c0 = parent->shard_col0[k], r0 = c0 / per;
        std::vector<double> ta(a_smooth ? (size_t)m * sd : 0), tP(P_smooth ? (size_t)m * sd * sd : 0), te(resid ? (size_t)m * d : 0);
        if (int st = ssde_smooth(sh, par, parent->L.n_full, a_smooth ? ta.data() : nullptr, P_smooth ? tP.data() : nullptr,
                                 resid ? te.data() : nullptr)) return st;
        if (a_smooth) place_columns(a_smooth, n, c0, ta.data(), m, sd, lo);
        if (resid) place_columns(resid, n, r0, te.data(), m, d, lo);
        if (P_smooth) place_cov_block(P_smooth, n, SD, c0, tP.data(), m, sd, lo);      // (a row without a state: no covariance at all)
        return SSDE_OK;
    });
}

// the shards' and column pairs' leave-one-out outputs, placed as smooth_sharded places the smoother's: a pair's columns (and its
// diagonal block of the covariance; the cross-pair blocks are exactly zero) in the parent's wider layout, a track shard's rows and
// tracks at their places.  lpd and stats are asked of track shards only (the entry refuses them on column pairs); the row of a
// maximum, which a shard counts in its own rows, is moved to the parent's rows.
int loo_sharded(ssde_handle* parent, const double* par, double* loo_mean, double* loo_cov, double* loo_resid, double* lpd,
                const double* thr, int n_thr, double* stats) {
    const int64_t n = parent->n, NT = parent->n_seg;
    const int D = parent->d, per = parent->model == SSDE_MODEL_CTCRW ? 2 : 1, n_stat = 4 + n_thr;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (loo_mean) std::fill(loo_mean, loo_mean + (size_t)n * D, nan);
    if (loo_cov) std::fill(loo_cov, loo_cov + (size_t)n * D * D, 0.0);           // cross-pair blocks: zero
    if (loo_resid) std::fill(loo_resid, loo_resid + (size_t)n * D, nan);
    if (lpd) std::fill(lpd, lpd + (size_t)n, nan);
    std::vector<char> any(loo_cov ? (size_t)n : 0, 0);                           // rows some engine served
    const int st = for_each_shard(parent, [&](ssde_handle* sh, size_t k, int64_t lo, int64_t m, int64_t track0) -> int {
        const int64_t mt = sh->n_seg;
        const int d = sh->d, r0 = parent->shard_col0[k] / per;
        std::vector<double> tm(loo_mean ? (size_t)m * d : 0), tc(loo_cov ? (size_t)m * d * d : 0), te(loo_resid ? (size_t)m * d : 0),
            tl(lpd ? (size_t)m : 0), ts(stats ? (size_t)mt * n_stat : 0);
        if (int st = ssde_smooth_loo(sh, par, parent->L.n_full, loo_mean ? tm.data() : nullptr, loo_cov ? tc.data() : nullptr,
                                     loo_resid ? te.data() : nullptr, lpd ? tl.data() : nullptr, thr, n_thr, stats ? ts.data() : nullptr, 0))
            return st;
        if (loo_mean) place_columns(loo_mean, n, r0, tm.data(), m, d, lo);
        if (loo_resid) place_columns(loo_resid, n, r0, te.data(), m, d, lo);
        if (lpd) place_columns(lpd, n, 0, tl.data(), m, 1, lo);
        if (loo_cov) {
            // (place_block, not place_cov_block: the served rows of the pairs may differ here, so the rule for a row without a
            //  covariance is this call's own, below)
            place_block(loo_cov, n, D, r0, tc.data(), m, d, lo);
            for (int64_t i = 0; i < m; i++)
                if (!std::isnan(tc[i])) any[(size_t)(lo + i)] = 1;
        }
        if (stats) place_track_stats(stats, NT, track0, ts.data(), mt, n_stat, 1, 3, lo);      // statistic 3: the row of the maximum
        return SSDE_OK;
    });
    if (st) return st;
    // a row no engine served has no covariance at all; where the pairs disagree, the blocks of those that did not serve it are NaN
    // already (their own preset), the cross-pair zeros stand
    for (int64_t i = 0; loo_cov && i < n; i++)
        if (!any[(size_t)i])
            for (int q = 0; q < D * D; q++) loo_cov[(size_t)n * q + i] = nan;
    return SSDE_OK;
}

// the shards' and column pairs' forecast scores, placed as loo_sharded places the leave-one-out outputs: a pair's columns of z_ahead
// in the parent's wider layout horizon by horizon, a track shard's rows and tracks at their places.  lpd_ahead and stats are asked of
// track shards only (the entry refuses them on column pairs).
int ahead_sharded(ssde_handle* parent, const double* par, const int32_t* hz, int n_h, double* z_ahead, double* lpd_ahead,
                  const double* thr, int n_thr, double* stats) {
    const int64_t n = parent->n, NT = parent->n_seg;
    const int D = parent->d, per = parent->model == SSDE_MODEL_CTCRW ? 2 : 1, n_stat = 5 + n_thr;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (z_ahead) std::fill(z_ahead, z_ahead + (size_t)n * D * n_h, nan);
    if (lpd_ahead) std::fill(lpd_ahead, lpd_ahead + (size_t)n * n_h, nan);
    if (stats) std::fill(stats, stats + (size_t)NT * n_stat * n_h, 0.0);
    return for_each_shard(parent, [&](ssde_handle* sh, size_t k, int64_t lo, int64_t m, int64_t track0) -> int {
        const int64_t mt = sh->n_seg;
        const int d = sh->d, r0 = parent->shard_col0[k] / per;
        std::vector<double> tz(z_ahead ? (size_t)m * d * n_h : 0), tl(lpd_ahead ? (size_t)m * n_h : 0), ts(stats ? (size_t)mt * n_stat * n_h : 0);
        if (int st = ssde_forecast_scores(sh, par, parent->L.n_full, hz, n_h, z_ahead ? tz.data() : nullptr, lpd_ahead ? tl.data() : nullptr,
                                          thr, n_thr, stats ? ts.data() : nullptr, 0)) return st;
        for (int j = 0; z_ahead && j < n_h; j++) place_columns(z_ahead + (size_t)n * D * j, n, r0, tz.data() + (size_t)m * d * j, m, d, lo);
        if (lpd_ahead) place_columns(lpd_ahead, n, 0, tl.data(), m, n_h, lo);
        if (stats) place_track_stats(stats, NT, track0, ts.data(), mt, n_stat, n_h, -1, lo);
        return SSDE_OK;
    });
}

// the shards' and column pairs' draws, each counted by the GLOBAL track ordinal and state column, placed in the parent's layout
int draws_sharded(ssde_handle* parent, const double* par, uint64_t seed, int64_t draw0, int n_draws, double* draws, bool dev_out) {
    const int64_t n = parent->n;
    const int SD = parent->sdim;
    if (!dev_out) std::fill(draws, draws + (size_t)n * SD * n_draws, std::numeric_limits<double>::quiet_NaN());
    return for_each_shard(parent, [&](ssde_handle* sh, size_t k, int64_t lo, int64_t m, int64_t track0) -> int {
        const int sd = sh->sdim, c0 = parent->shard_col0[k];
        if (dev_out) {
            // the column pairs of ONE device: every pair holds all the rows and writes (or gathers) its columns straight into the
            // parent's matrices in HBM, batch by batch under the budget like any single handle
            if (lo != 0 || m != n) return refuse(sh, SSDE_ERR_ARG, "ssde_smooth_draws: SSDE_DRAWS_DEVICE_OUT needs a single-device handle");
            return draws_single(sh, par, seed, draw0, n_draws, draws + (size_t)n * c0, true, (int64_t)n * SD, track0, c0);
        }
        std::vector<double> t((size_t)m * sd * n_draws);
        if (int st = draws_single(sh, par, seed, draw0, n_draws, t.data(), false, (int64_t)m * sd, track0, c0)) return st;
        for (int q = 0; q < n_draws; q++) place_columns(draws + (size_t)n * SD * q, n, c0, t.data() + (size_t)m * sd * q, m, sd, lo);
        return SSDE_OK;
    });
}

}  // namespace ssde_engine

extern "C" {

int ssde_smooth_draws(ssde_handle* h, const double* par, int32_t n_par_full, uint64_t seed, int64_t draw0, int32_t n_draws,
                      double* draws, uint32_t flags) {
    if (!h || !par || !draws) { if (h) h->err = "ssde_smooth_draws: no parameter vector, or no output"; return SSDE_ERR_ARG; }
    if (int st = check_par_len(h, n_par_full)) return st;
    if (int st = check_draw_range(h, "ssde_smooth_draws", draw0, n_draws)) return st;
    if (flags & ~(uint32_t)SSDE_DRAWS_DEVICE_OUT) { h->err = "ssde_smooth_draws: unknown flag"; return SSDE_ERR_ARG; }
    if (int st = check_kalman(h)) return st;
    const bool dev_out = (flags & SSDE_DRAWS_DEVICE_OUT) != 0;
    if (!h->shards.empty()) {
        if (dev_out && h->n_track_shards > 1) { h->err = "ssde_smooth_draws: SSDE_DRAWS_DEVICE_OUT needs a single-device handle"; return SSDE_ERR_ARG; }
        return draws_sharded(h, par, seed, draw0, n_draws, draws, dev_out);
    }
    return draws_single(h, par, seed, draw0, n_draws, draws, dev_out, (int64_t)h->n * h->sdim, 0, 0);
}

int ssde_path_stats(ssde_handle* h, const double* par, int32_t n_par_full, uint64_t seed, int64_t draw0, int32_t n_draws,
                    const double* regions, int32_t n_regions, const double* weight, double* stats, uint32_t flags) {
    if (!h || !par || !stats) { if (h) h->err = "ssde_path_stats: no parameter vector, or no output"; return SSDE_ERR_ARG; }
    if (int st = check_par_len(h, n_par_full)) return st;
    if (int st = check_draw_range(h, "ssde_path_stats", draw0, n_draws)) return st;
    if (n_regions < 0 || n_regions > SSDE_PATH_MAX_REGIONS || (n_regions > 0 && !regions)) {
        h->err = "ssde_path_stats: 0 <= n_regions <= SSDE_PATH_MAX_REGIONS, with a table of bounds when there are regions";
        return SSDE_ERR_ARG;
    }
    for (int k = 0; k < 2 * n_regions; k++) {
        const double lo = regions[2 * k], hi = regions[2 * k + 1];
        if ((k & 1) && h->d == 1) continue;                         // the second pair is not read for one position column
        if (std::isnan(lo) || std::isnan(hi) || lo > hi) { h->err = "ssde_path_stats: a region bound that is NaN, or lo > hi"; return SSDE_ERR_ARG; }
    }
    if (flags != 0) { h->err = "ssde_path_stats: unknown flag"; return SSDE_ERR_ARG; }
    if (int st = check_kalman(h)) return st;
    if (int st = check_position_columns(h, "ssde_path_stats", "distance", "position")) return st;
    if (!h->shards.empty()) return path_sharded(h, par, seed, draw0, n_draws, regions, n_regions, weight, stats);
    return path_single(h, par, seed, draw0, n_draws, regions, n_regions, weight, stats, 0);
}

int ssde_path_speed(ssde_handle* h, const double* par, int32_t n_par_full, uint64_t seed, int64_t draw0, int32_t n_draws,
                    const double* thr, int32_t n_thr, const double* weight, double* stats, uint32_t* row_below, uint32_t flags) {
    if (!h || !par || (!stats && !row_below)) { if (h) h->err = "ssde_path_speed: no parameter vector, or no output"; return SSDE_ERR_ARG; }
    if (int st = check_par_len(h, n_par_full)) return st;
    if (int st = check_draw_range(h, "ssde_path_speed", draw0, n_draws)) return st;
    if (n_thr < 0 || n_thr > SSDE_SPEED_MAX_THR || (n_thr > 0 && !thr)) {
        h->err = "ssde_path_speed: 0 <= n_thr <= SSDE_SPEED_MAX_THR, with a table of thresholds when there are any";
        return SSDE_ERR_ARG;
    }
    for (int k = 0; k < n_thr; k++)
        if (std::isnan(thr[k]) || thr[k] < 0.0) { h->err = "ssde_path_speed: a threshold that is NaN or negative"; return SSDE_ERR_ARG; }
    if (row_below && n_thr == 0) { h->err = "ssde_path_speed: per-row counts need a threshold"; return SSDE_ERR_ARG; }
    if (flags != 0) { h->err = "ssde_path_speed: unknown flag"; return SSDE_ERR_ARG; }
    if (int st = check_kalman(h)) return st;
    if (h->model != SSDE_MODEL_CTCRW) { h->err = "ssde_path_speed: the state of OU_SSM and BM_SSM holds no velocity (a CTCRW's does)"; return SSDE_ERR_MODEL; }
    if (int st = check_position_columns(h, "ssde_path_speed", "speed", "velocity")) return st;
    if (!h->shards.empty()) return speed_sharded(h, par, seed, draw0, n_draws, thr, n_thr, weight, stats, row_below);
    return speed_single(h, par, seed, draw0, n_draws, thr, n_thr, weight, stats, row_below, 0);
}

// what ssde_path_occupancy and ssde_path_occupancy_fine check alike, before anything touches the device; wmax: the largest weight (1
// without weights)
static int occ_check(ssde_handle* h, const char* who, const double* par, int32_t n_par_full, int64_t draw0, int32_t n_draws,
                     const ssde_occ_grid* grid, const double* weight, const int32_t* group, int32_t n_groups, const double* occ,
                     uint32_t flags, double& wmax) {
    const std::string w(who);
    if (!h || !par || !grid || !occ) { if (h) h->err = w + ": no parameter vector, no grid, or no output"; return SSDE_ERR_ARG; }
    if (int st = check_par_len(h, n_par_full)) return st;
    if (int st = check_draw_range(h, w, draw0, n_draws)) return st;
    if (flags & ~(uint32_t)SSDE_OCC_FORCE_GLOBAL) { h->err = w + ": unknown flag"; return SSDE_ERR_ARG; }
    if (grid->nx < 1 || grid->nx > 4096 || grid->ny < 1 || grid->ny > 4096) { h->err = w + ": nx and ny must be 1 ... 4096"; return SSDE_ERR_ARG; }
    if (n_groups < 1 || (int64_t)grid->nx * grid->ny * (int64_t)n_groups > ((int64_t)1 << 28)) {
        h->err = w + ": n_groups >= 1 and nx * ny * n_groups <= 2^28 are required";
        return SSDE_ERR_ARG;
    }
    if (!group && n_groups != 1) { h->err = w + ": without a group table there is one group"; return SSDE_ERR_ARG; }
    if (int st = check_kalman(h)) return st;
    if (int st = check_position_columns(h, w, "cell", "position")) return st;
    if (h->d == 1 && grid->ny != 1) { h->err = w + ": one position column takes ny = 1"; return SSDE_ERR_ARG; }
    if (!std::isfinite(grid->x0) || !std::isfinite(grid->dx) || grid->dx <= 0.0 ||
        (h->d == 2 && (!std::isfinite(grid->y0) || !std::isfinite(grid->dy) || grid->dy <= 0.0))) {
        h->err = w + ": the grid's origin must be finite and its steps finite and positive";
        return SSDE_ERR_ARG;
    }
    for (int64_t t = 0; group && t < h->n_seg; t++)
        if (group[t] < -1 || group[t] >= n_groups) { h->err = w + ": a group outside -1 ... n_groups - 1"; return SSDE_ERR_ARG; }
    return check_weights(h, w, weight, h->n, wmax);
}

int ssde_path_occupancy(ssde_handle* h, const double* par, int32_t n_par_full, uint64_t seed, int64_t draw0, int32_t n_draws,
                        const ssde_occ_grid* grid, const double* weight, const int32_t* group, int32_t n_groups, double* occ,
                        double* outside, uint32_t flags) {
    double wmax = 1.0;
    if (int st = occ_check(h, "ssde_path_occupancy", par, n_par_full, draw0, n_draws, grid, weight, group, n_groups, occ, flags, wmax)) return st;
    // the quantum of the whole handle's call; the counts of every engine, chunk and batch add up as integers
    const int e = occ_quantum_exp(wmax, h->n, n_draws);
    const bool force_global = (flags & SSDE_OCC_FORCE_GLOBAL) != 0;
    const size_t n_cells = (size_t)grid->nx * grid->ny * n_groups;
    std::vector<uint64_t> counts(n_cells + (size_t)n_groups, 0);
    const int st = h->shards.empty() ? occ_single(h, par, seed, draw0, n_draws, *grid, weight, group, n_groups, e, force_global, counts, 0)
                                     : occ_sharded(h, par, seed, draw0, n_draws, *grid, weight, group, n_groups, e, force_global, counts);
    if (st) return st;
    for (size_t i = 0; i < n_cells; i++) occ[i] = ldexp((double)counts[i], e);
    for (int g = 0; outside && g < n_groups; g++) outside[g] = ldexp((double)counts[n_cells + g], e);
    return SSDE_OK;
}

int ssde_path_occupancy_fine(ssde_handle* h, const double* par, int32_t n_par_full, uint64_t seed, int64_t draw0, int32_t n_draws,
                             const ssde_occ_grid* grid, double max_step, const double* weight, const int32_t* group, int32_t n_groups,
                             double* occ, double* outside, uint32_t flags) {
    double wmax = 1.0;
    if (int st = occ_check(h, "ssde_path_occupancy_fine", par, n_par_full, draw0, n_draws, grid, weight, group, n_groups, occ, flags, wmax)) return st;
    if (!(max_step > 0.0)) { h->err = "ssde_path_occupancy_fine: max_step must be positive (+inf: no refinement)"; return SSDE_ERR_ARG; }
    // the bridge deviates' counter holds the track ordinal's low word (ssde_predict_draws)
    if (h->n_seg >= ((int64_t)1 << 32)) { h->err = "ssde_path_occupancy_fine: 2^32 or more tracks"; return SSDE_ERR_ARG; }
    const int e = occ_quantum_exp(wmax, h->n, n_draws);
    const bool force_global = (flags & SSDE_OCC_FORCE_GLOBAL) != 0;
    const size_t n_cells = (size_t)grid->nx * grid->ny * n_groups;
    std::vector<uint64_t> counts(n_cells + (size_t)n_groups, 0);
    int64_t n_points = 0, n_capped = 0;
    h->last_occ_points = 0; h->last_occ_capped = 0;
    const int st = h->shards.empty()
        ? occ_fine_single(h, par, seed, draw0, n_draws, *grid, max_step, weight, group, n_groups, e, force_global, counts, n_points, n_capped, 0)
        : occ_fine_sharded(h, par, seed, draw0, n_draws, *grid, max_step, weight, group, n_groups, e, force_global, counts, n_points, n_capped);
    if (st) return st;
    h->last_occ_points = n_points; h->last_occ_capped = n_capped;
    for (size_t i = 0; i < n_cells; i++) occ[i] = ldexp((double)counts[i], e);
    for (int g = 0; outside && g < n_groups; g++) outside[g] = ldexp((double)counts[n_cells + g], e);
    return SSDE_OK;
}

int ssde_last_occupancy_points(const ssde_handle* h, int64_t* n_points, int64_t* n_capped) {
    if (!h) return SSDE_ERR_ARG;
    if (n_points) *n_points = h->last_occ_points;
    if (n_capped) *n_capped = h->last_occ_capped;
    return SSDE_OK;
}

int ssde_last_occupancy_form(const ssde_handle* h) {
    if (!h) return -1;
    return h->shards.empty() ? h->last_occ_form : h->shards[0]->last_occ_form;
}

int ssde_predict(ssde_handle* h, const double* par, int32_t n_par_full, const int64_t* q_row, const double* q_off, int64_t n_query,
                 double* a_pred, double* P_pred) {
    if (!h || !par || !q_row || !q_off || !a_pred) { if (h) h->err = "ssde_predict: no parameter vector, no queries, or no output"; return SSDE_ERR_ARG; }
    if (int st = check_par_len(h, n_par_full)) return st;
    if (n_query < 1) { h->err = "ssde_predict: n_query >= 1 is required"; return SSDE_ERR_ARG; }
    if (int st = check_queries(h, "ssde_predict", q_row, q_off, n_query)) return st;
    if (int st = check_kalman(h)) return st;
    if (!h->shards.empty()) return predict_sharded(h, par, q_row, q_off, n_query, a_pred, P_pred);
    return predict_single(h, par, q_row, q_off, n_query, a_pred, P_pred);
}

int ssde_predict_draws(ssde_handle* h, const double* par, int32_t n_par_full, const int64_t* q_row, const double* q_off, int64_t n_query,
                       uint64_t seed, int64_t draw0, int32_t n_draws, double* draws_at, uint32_t flags) {
    if (!h || !par || !q_row || !q_off || !draws_at) { if (h) h->err = "ssde_predict_draws: no parameter vector, no queries, or no output"; return SSDE_ERR_ARG; }
    if (int st = check_par_len(h, n_par_full)) return st;
    if (n_query < 1) { h->err = "ssde_predict_draws: n_query >= 1 is required"; return SSDE_ERR_ARG; }
    if (int st = check_queries(h, "ssde_predict_draws", q_row, q_off, n_query)) return st;
    if (int st = check_draw_range(h, "ssde_predict_draws", draw0, n_draws)) return st;
    if (flags != 0) { h->err = "ssde_predict_draws: unknown flag"; return SSDE_ERR_ARG; }
    // the bridge deviates' counter holds the track ordinal's low word and the rank of an offset in its interval, 32 bits each
    if (h->n_seg >= ((int64_t)1 << 32)) { h->err = "ssde_predict_draws: 2^32 or more tracks"; return SSDE_ERR_ARG; }
    if (int st = check_distinct_offsets(h, "ssde_predict_draws", q_row, q_off, n_query)) return st;
    if (int st = check_kalman(h)) return st;
    if (!h->shards.empty()) return predict_draws_sharded(h, par, q_row, q_off, n_query, seed, draw0, n_draws, draws_at);
    if (int st = check_not_coupled_wide(h, "ssde_predict_draws")) return st;        // (every check before the device is touched)
    return predict_draws_single(h, par, q_row, q_off, n_query, seed, draw0, n_draws, draws_at, 0, 0);
}

int ssde_path_proximity(ssde_handle* h, const double* par, int32_t n_par_full, uint64_t seed, int64_t draw0, int32_t n_draws,
                        const int64_t* qa_row, const double* qa_off, const int64_t* qb_row, const double* qb_off,
                        const int64_t* pair_ptr, int32_t n_pairs, const double* weight, const double* radii, int32_t n_radii,
                        double* stats, uint32_t flags) {
    if (!h || !par || !qa_row || !qa_off || !qb_row || !qb_off || !pair_ptr || !stats) {
        if (h) h->err = "ssde_path_proximity: no parameter vector, no queries, no pair list, or no output";
        return SSDE_ERR_ARG;
    }
    if (int st = check_par_len(h, n_par_full)) return st;
    if (n_pairs < 1) { h->err = "ssde_path_proximity: n_pairs >= 1 is required"; return SSDE_ERR_ARG; }
    bool csr = pair_ptr[0] == 0;
    for (int32_t p = 0; csr && p < n_pairs; p++) csr = pair_ptr[p + 1] >= pair_ptr[p];
    if (!csr || pair_ptr[n_pairs] < 1) {
        h->err = "ssde_path_proximity: pair_ptr must start at 0, not decrease, and end at n_point >= 1";
        return SSDE_ERR_ARG;
    }
    const int64_t np = pair_ptr[n_pairs];
    if (int st = check_queries(h, "ssde_path_proximity", qa_row, qa_off, np)) return st;       // side A's queries, then side B's
    if (int st = check_queries(h, "ssde_path_proximity", qb_row, qb_off, np)) return st;
    if (int st = check_draw_range(h, "ssde_path_proximity", draw0, n_draws)) return st;
    if (n_radii < 0 || n_radii > SSDE_PROX_MAX_RADII || (n_radii > 0 && !radii)) {
        h->err = "ssde_path_proximity: 0 <= n_radii <= SSDE_PROX_MAX_RADII, with a table of radii when there are any";
        return SSDE_ERR_ARG;
    }
    for (int r = 0; r < n_radii; r++)
        if (!(radii[r] >= 0.0)) { h->err = "ssde_path_proximity: a radius that is NaN or negative"; return SSDE_ERR_ARG; }
    double wmax = 1.0;
    if (int st = check_weights(h, "ssde_path_proximity", weight, np, wmax)) return st;
    if (flags != 0) { h->err = "ssde_path_proximity: unknown flag"; return SSDE_ERR_ARG; }
    // the limits of ssde_predict_draws: the bridge deviates' counter holds the track ordinal's low word and the rank of an offset
    if (h->n_seg >= ((int64_t)1 << 32)) { h->err = "ssde_path_proximity: 2^32 or more tracks"; return SSDE_ERR_ARG; }
    std::vector<int64_t> q_row((size_t)2 * np);
    std::vector<double> q_off((size_t)2 * np);
    std::copy(qa_row, qa_row + np, q_row.begin()); std::copy(qb_row, qb_row + np, q_row.begin() + np);
    std::copy(qa_off, qa_off + np, q_off.begin()); std::copy(qb_off, qb_off + np, q_off.begin() + np);
    if (int st = check_distinct_offsets(h, "ssde_path_proximity", q_row.data(), q_off.data(), 2 * np)) return st;
    if (int st = check_kalman(h)) return st;
    if (int st = check_position_columns(h, "ssde_path_proximity", "distance", "position")) return st;
    // (every check before the device is touched)
    ProxCall c;
    c.n_point = np; c.n_pairs = n_pairs; c.n_radii = n_radii; c.n_stat = 2 + n_radii; c.radii = radii;
    c.e = occ_quantum_exp(wmax, np, 1);                              // no n_draws in the quantum: draw ranges cut over calls agree bitwise
    c.unit = occ_quantise(1.0, c.e);
    if (weight) { c.wq.resize((size_t)np); occ_quantise_all(weight, np, c.e, c.wq.data()); }
    c.plan = plan_prox_tiles(pair_ptr, n_pairs);
    int n_batches = 0;
    h->last_prox_tiles = 0; h->last_prox_tiles_max = 0; h->last_prox_batches = 0; h->last_prox_route = 0;
    const bool sharded = !h->shards.empty();
    const int st = sharded ? prox_sharded(h, par, q_row.data(), q_off.data(), c, seed, draw0, n_draws, stats, n_batches)
                           : prox_single(h, par, q_row.data(), q_off.data(), c, seed, draw0, n_draws, stats, n_batches);
    if (st) return st;
    h->last_prox_tiles = c.plan.n_tiles; h->last_prox_tiles_max = c.plan.tiles_max;
    h->last_prox_batches = n_batches; h->last_prox_route = sharded ? 2 : 1;
    return SSDE_OK;
}

int ssde_last_proximity_plan(const ssde_handle* h, int64_t* n_tiles, int64_t* tiles_max, int32_t* n_batches, int32_t* route) {
    if (!h) return SSDE_ERR_ARG;
    if (n_tiles) *n_tiles = h->last_prox_tiles;
    if (tiles_max) *tiles_max = h->last_prox_tiles_max;
    if (n_batches) *n_batches = h->last_prox_batches;
    if (route) *route = h->last_prox_route;
    return SSDE_OK;
}

int ssde_smooth(ssde_handle* h, const double* par, int32_t n_par_full, double* a_smooth, double* P_smooth, double* resid) {
    if (!h || !par || (!a_smooth && !P_smooth && !resid)) { if (h) h->err = "ssde_smooth: no parameter vector, or no output asked for"; return SSDE_ERR_ARG; }
    if (int st = check_par_len(h, n_par_full)) return st;
    if (int st = check_kalman(h)) return st;
    if (!h->shards.empty()) return smooth_sharded(h, par, a_smooth, P_smooth, resid);
    return smooth_single(h, par, a_smooth, P_smooth, resid);
}

int ssde_smooth_loo(ssde_handle* h, const double* par, int32_t n_par_full, double* loo_mean, double* loo_cov, double* loo_resid,
                    double* lpd, const double* thr, int32_t n_thr, double* stats, uint32_t flags) {
    if (!h || !par || (!loo_mean && !loo_cov && !loo_resid && !lpd && !stats)) {
        if (h) h->err = "ssde_smooth_loo: no parameter vector, or no output asked for";
        return SSDE_ERR_ARG;
    }
    if (int st = check_par_len(h, n_par_full)) return st;
    if (int st = check_thresholds(h, "ssde_smooth_loo", thr, n_thr, SSDE_LOO_MAX_THR, "SSDE_LOO_MAX_THR", stats != nullptr)) return st;
    if (flags != 0) { h->err = "ssde_smooth_loo: unknown flag"; return SSDE_ERR_ARG; }
    if (int st = check_kalman(h)) return st;
    if (!h->shards.empty()) {
        if ((lpd || stats) && std::max(h->n_dim_parts, 1) > 1) {
            h->err = "ssde_smooth_loo: lpd and stats are not served for an uncoupled wide response run as column pairs (they need a per-row sum across the pair handles); loo_mean, loo_cov and loo_resid are";
            return SSDE_ERR_MODEL;
        }
        return loo_sharded(h, par, loo_mean, loo_cov, loo_resid, lpd, thr, n_thr, stats);
    }
    return loo_single(h, par, loo_mean, loo_cov, loo_resid, lpd, thr, n_thr, stats);
}

int ssde_forecast_scores(ssde_handle* h, const double* par, int32_t n_par_full, const int32_t* horizon, int32_t n_h, double* z_ahead,
                         double* lpd_ahead, const double* thr, int32_t n_thr, double* stats, uint32_t flags) {
    if (!h || !par || !horizon || (!z_ahead && !lpd_ahead && !stats)) {
        if (h) h->err = "ssde_forecast_scores: no parameter vector, no horizons, or no output asked for";
        return SSDE_ERR_ARG;
    }
    if (int st = check_par_len(h, n_par_full)) return st;
    switch (check_horizons(horizon, n_h, SSDE_AHEAD_MAX_H, SSDE_AHEAD_MAX_STEP)) {
        case 0: break;
        case 1: return refuse(h, SSDE_ERR_ARG, "ssde_forecast_scores: 1 <= n_h <= SSDE_AHEAD_MAX_H is required");
        case 2: return refuse(h, SSDE_ERR_ARG, "ssde_forecast_scores: a horizon outside 1 .. SSDE_AHEAD_MAX_STEP");
        default: return refuse(h, SSDE_ERR_ARG, "ssde_forecast_scores: the horizons must be strictly increasing");
    }
    if (int st = check_thresholds(h, "ssde_forecast_scores", thr, n_thr, SSDE_AHEAD_MAX_THR, "SSDE_AHEAD_MAX_THR", stats != nullptr)) return st;
    if (flags != 0) { h->err = "ssde_forecast_scores: unknown flag"; return SSDE_ERR_ARG; }
    if (int st = check_kalman(h)) return st;
    if (!h->shards.empty()) {
        if ((lpd_ahead || stats) && std::max(h->n_dim_parts, 1) > 1) {
            h->err = "ssde_forecast_scores: lpd_ahead and stats are not served for an uncoupled wide response run as column pairs (they need a per-row sum across the pair handles); z_ahead is";
            return SSDE_ERR_MODEL;
        }
        return ahead_sharded(h, par, horizon, n_h, z_ahead, lpd_ahead, thr, n_thr, stats);
    }
    if (int st = check_not_coupled_wide(h, "ssde_forecast_scores")) return st;          // (every check before the device is touched)
    return ahead_single(h, par, horizon, n_h, z_ahead, lpd_ahead, thr, n_thr, stats);
}

}  // extern "C"
