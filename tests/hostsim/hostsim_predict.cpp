// hostsim_predict.cpp -- TEST INFRASTRUCTURE, not an engine.
//
// Compiles smoothsde_amd/csrc/ssde_predict.hpp (the lane math of k_predict.hip) over ssde_smooth.hpp / ssde_dense.hpp with g++ and
// walks each track the way one lane of the kernels does: smooth_record_row + predict_side_row -> dense_step per state row, then from
// the last record to the first predict_packet_row (before the row is processed) and smooth_back_row; predict_query_row answers the
// queries from the packets.  tests/test_predict_hostsim.py compares it with tests/predict_ref.py.  It also exports the host-side
// plans of smoothsde_amd/csrc/ssde_smooth_plan.hpp to tests/test_smooth_plan_host.py.
#include <cstring>

#include "../../smoothsde_amd/csrc/ssde_smooth_plan.hpp"
#include "hostsim_records.hpp"

using namespace ssde;

namespace {

// the problem as hostsim_records.hpp has it.  Queries (q_row, q_off); a_pred (nq x SD) and P_pred (nq x SD x SD), row-major, are
// written where a state exists.
template <int MODEL, int D>
void run_predict(const TwinProblem& pb, int64_t nq, const int64_t* q_row, const double* q_off, double* a_pred, double* P_pred) {
    typedef SmoothRec<MODEL, D> RC;
    typedef PredictPk<MODEL, D> PK;
    constexpr int SD = RC::SD, R = RC::R, SW = PK::SW, SZ = PK::SZ;
    std::vector<double> packets((size_t)pb.n * SZ, 0.0), recs, side;
    std::vector<char> has((size_t)pb.n, 0);
    for (int64_t m = 0; m < pb.n_tracks; m++) {
        const int64_t ns = twin_record_track<MODEL, D>(pb, m, recs, &side);
        if (ns <= 0) continue;
        double r[SD] = {}, N[SD][SD] = {};
        for (int64_t s = ns - 1; s >= 0; s--) {
            const int64_t i = pb.row0[m] + 1 + s;
            const double* rp = &recs[(size_t)s * R];
            const double* sp = &side[(size_t)s * SW];
            double* pp = &packets[(size_t)i * SZ];
            predict_packet_row<MODEL, D, SD>([&](int k) -> double { return rp[k]; }, [&](int k) -> double { return sp[k]; }, r, N,
                                             s == ns - 1, [&](int k) -> double& { return pp[k]; });
            has[(size_t)i] = 1;
            double am[SD], V[SD][SD];
            smooth_back_row<MODEL, D, SD>(r, N, s == ns - 1, [&](int k) -> double { return rp[k]; }, am, V);
        }
    }
    for (int64_t k = 0; k < nq; k++) {
        const int64_t i = q_row[k];
        if (!has[(size_t)i]) continue;
        const double* pp = &packets[(size_t)i * SZ];
        double am[SD], V[SD][SD];
        if (!predict_query_row<MODEL, D, SD>([&](int q) -> double { return pp[q]; }, q_off[k], am, V)) continue;
        for (int c = 0; c < SD; c++) {
            a_pred[k * SD + c] = am[c];
            for (int q = 0; q < SD; q++) P_pred[(k * SD + c) * SD + q] = V[c][q];
        }
    }
}

template <class T>
void copy_out(const std::vector<T>& v, T* dst) { if (!v.empty()) memcpy(dst, v.data(), v.size() * sizeof(T)); }

}  // namespace

extern "C" {

int hostsim_predict(int model, int d, TWIN_PARAMS, int64_t nq, const int64_t* q_row, const double* q_off, double* a_pred, double* P_pred) {
#define PR(MODEL, D) if (model == MODEL && d == D) { run_predict<MODEL, D>(TWIN_ARGS, nq, q_row, q_off, a_pred, P_pred); return 0; }
    TWIN_D12(PR)
#undef PR
    return 1;
}

int hostsim_predict_packet_doubles(int model, int d) {
#define PD(MODEL, D) if (model == MODEL && d == D) return PredictPk<MODEL, D>::SZ;
    TWIN_D12(PD)
#undef PD
    return 0;
}

// ---- the plans of ssde_smooth_plan.hpp ------------------------------------------------------------------------------------------
// plan_queries over nl lanes and nq queries (pad_row NULL: the rows are the caller's).  order, q_slot, off: room for nq; want_off:
// nl + 1; want_step: nq.  cuts: n_cuts group boundaries (ascending, wave lanes a group); ranges: (n_cuts - 1) x 4 = s0, s1, q0, q1 of
// every chunk.  counts = planned queries, slots.
void hostsim_plan_queries(int64_t nl, const int64_t* row0, const int32_t* ns, const int64_t* pad_row, double pad_step, int64_t nq,
                          const int64_t* q_row, const double* q_off, int n_cuts, const int32_t* cuts, int wave, int64_t* counts,
                          int64_t* order, int64_t* q_slot, double* off, int64_t* want_off, int32_t* want_step, int64_t* ranges) {
    const ssde_plan::QueryPlan P = ssde_plan::plan_queries(std::vector<int64_t>(row0, row0 + nl), std::vector<int32_t>(ns, ns + nl),
                                                           pad_row, pad_step, q_row, q_off, nq);
    counts[0] = (int64_t)P.order.size(); counts[1] = (int64_t)P.want_step.size();
    copy_out(P.order, order); copy_out(P.q_slot, q_slot); copy_out(P.off, off);
    copy_out(P.want_off, want_off); copy_out(P.want_step, want_step);
    for (int c = 0; c + 1 < n_cuts; c++) {
        const ssde_plan::QueryRange r = ssde_plan::chunk_queries(P, cuts[c], cuts[c + 1], wave);
        ranges[4 * c] = r.s0; ranges[4 * c + 1] = r.s1; ranges[4 * c + 2] = r.q0; ranges[4 * c + 3] = r.q1;
    }
}

// chunk_groups over goff (n_groups + 1 offsets): cuts gets at most n_groups + 1 entries, returns how many
int hostsim_chunk_groups(int n_groups, const int64_t* goff, int64_t budget, int32_t* cuts) {
    const std::vector<int> cut = ssde_plan::chunk_groups(std::vector<int64_t>(goff, goff + n_groups + 1), budget);
    for (size_t k = 0; k < cut.size(); k++) cuts[k] = cut[k];
    return (int)cut.size();
}

int hostsim_batch_cap(int64_t budget, int64_t per_draw, int unit, int ch, int n_draws) { return ssde_plan::batch_cap(budget, per_draw, unit, ch, n_draws); }

// ---- a parent of several engines: the deal of the queries, the placement of an engine's outputs ------------------------------------
// deal_queries: idx, rows, offs have room for nq; returns how many queries are on rows [lo, lo + m)
int64_t hostsim_deal_queries(int64_t lo, int64_t m, const int64_t* q_row, const double* q_off, int64_t nq, int64_t* idx, int64_t* rows, double* offs) {
    const ssde_plan::QueryDeal D = ssde_plan::deal_queries(lo, m, q_row, q_off, nq);
    copy_out(D.idx, idx); copy_out(D.rows, rows); copy_out(D.offs, offs);
    return (int64_t)D.idx.size();
}

// idx NULL: the engine's rows are the parent's lo ..
void hostsim_place_columns(double* dst, int64_t n, int c0, const double* src, int64_t m, int ncol, int64_t lo, const int64_t* idx) {
    ssde_plan::place_columns(dst, n, c0, src, m, ncol, lo, idx);
}

// nan_rule 1: place_cov_block (a row whose block is NaN has no covariance at all), 0: place_block
void hostsim_place_block(double* dst, int64_t n, int SD, int c0, const double* src, int64_t m, int sd, int64_t lo, const int64_t* idx, int nan_rule) {
    if (nan_rule) ssde_plan::place_cov_block(dst, n, SD, c0, src, m, sd, lo, idx);
    else ssde_plan::place_block(dst, n, SD, c0, src, m, sd, lo, idx);
}

void hostsim_place_track_stats(double* dst, int64_t NT, int64_t track0, const double* src, int64_t mt, int n_stat, int64_t n_rep, int row_stat,
                               int64_t lo) {
    ssde_plan::place_track_stats(dst, NT, track0, src, mt, n_stat, n_rep, row_stat, lo);
}

int64_t hostsim_max_distinct_offsets(const int64_t* q_row, const double* q_off, int64_t nq) { return ssde_plan::max_distinct_offsets(q_row, q_off, nq); }

}  // extern "C"
