// hostsim_predict_draws.cpp -- TEST INFRASTRUCTURE, not an engine.
//
// Compiles smoothsde_amd/csrc/ssde_bridge.hpp (the lane math of k_predict_draws.hip) over ssde_draws.hpp / ssde_predict.hpp with g++
// and walks each track the way one lane of the kernels does: the record pass with side rows (hostsim_records.hpp), the draws' walk
// from the last record to the first with the walk's store rule -- a path's state at step s is the LEFT end of slot(s) when s is wanted
// and the RIGHT end of slot(s - 1) when s - 1 is --, then bridge_slot_walk per (slot, draw) over the host plan's CSR lists
// (plan_queries + plan_slot_offsets, lane = track).  tests/test_predict_draws_hostsim.py compares it with tests/bridge_ref.py.  It
// also exports plan_slot_offsets and the batch rule to tests/test_predict_draws_plan_host.py.
#include <cstring>

#include "../../smoothsde_amd/csrc/ssde_bridge.hpp"
#include "../../smoothsde_amd/csrc/ssde_smooth_plan.hpp"
#include "hostsim_records.hpp"

using namespace ssde;

namespace {

// out (n_draws x nq x SD, row-major) is written where an answer exists
template <int MODEL, int D>
void run_predict_draws(const TwinProblem& pb, int64_t nq, const int64_t* q_row, const double* q_off, uint64_t seed, int64_t draw0,
                       int n_draws, double* out) {
    typedef SmoothRec<MODEL, D> RC;
    typedef DrawFac<MODEL, D> FC;
    typedef BridgePk<MODEL, D> BK;
    constexpr int SD = RC::SD, R = RC::R, SW = BK::SW, Q = BK::Q;
    std::vector<int64_t> row0(pb.row0, pb.row0 + pb.n_tracks);
    std::vector<int32_t> nsv((size_t)pb.n_tracks);
    for (int64_t m = 0; m < pb.n_tracks; m++) nsv[(size_t)m] = (int32_t)(pb.nrows[m] - 1);
    const ssde_plan::QueryPlan P = ssde_plan::plan_queries(row0, nsv, nullptr, 0.0, q_row, q_off, nq);
    const ssde_plan::SlotOffsets S = ssde_plan::plan_slot_offsets(P);
    std::vector<double> recs, side;
    for (int64_t m = 0; m < pb.n_tracks; m++) {
        const int64_t w0 = P.want_off[(size_t)m], w1 = P.want_off[(size_t)m + 1];
        if (w1 == w0) continue;
        const int64_t ns = twin_record_track<MODEL, D>(pb, m, recs, &side);
        if (ns <= 0) continue;
        const int64_t nw = w1 - w0;
        std::vector<double> ends((size_t)nw * n_draws * BK::EZ, 0.0), sidepk((size_t)nw * SW, 0.0);
        std::vector<double> al((size_t)n_draws * SD, 0.0);
        DrawNext<SD> nx;
        draw_next_init<SD>(nx);
        int64_t cur = w1 - 1;
        const int smin = P.want_step[(size_t)w0];
        for (int64_t s = ns - 1; s >= smin; s--) {
            const double* rp = &recs[(size_t)s * R];
            const bool tail = s == ns - 1;
            double fac[FC::R];
            draw_factor_row<MODEL, D, SD>([&](int k) -> double { return rp[k]; }, tail, nx, [&](int k) -> double& { return fac[k]; });
            int64_t il = -1, ir = -1;
            if (cur >= w0 && P.want_step[(size_t)cur] == s) {
                il = cur - w0;
                const double* sp = &side[(size_t)s * SW];
                double* pk = &sidepk[(size_t)il * SW];
                bridge_side_row<MODEL, D>([&](int k) -> double { return sp[k]; }, tail, [&](int k) -> double& { return pk[k]; });
                cur--;
            }
            if (cur >= w0 && P.want_step[(size_t)cur] == s - 1) ir = cur - w0;
            for (int q = 0; q < n_draws; q++) {
                double z[SD], a[SD];
                draw_deviates<SD>(seed, (uint64_t)m, (uint32_t)s, (uint32_t)(draw0 + q), 0, z);
                for (int c = 0; c < SD; c++) a[c] = al[(size_t)q * SD + c];
                draw_step<MODEL, D, SD>([&](int k) -> double { return fac[k]; }, tail, a, z);
                for (int c = 0; c < SD; c++) {
                    al[(size_t)q * SD + c] = a[c];
                    if (il >= 0) ends[((size_t)il * n_draws + q) * BK::EZ + BK::L + c] = a[c];
                    if (ir >= 0) ends[((size_t)ir * n_draws + q) * BK::EZ + BK::R + c] = a[c];
                }
            }
        }
        for (int64_t i = 0; i < nw; i++) {
            const int64_t slot = w0 + i, g0 = S.off_ptr[(size_t)slot], n_off = S.off_ptr[(size_t)slot + 1] - g0;
            const double* pk = &sidepk[(size_t)i * SW];
            DualN<0> par[Q];
            for (int j = 0; j < Q; j++) par[j] = DualN<0>(pk[BK::PAR + j]);
            const uint32_t s = (uint32_t)P.want_step[(size_t)slot];
            for (int q = 0; q < n_draws; q++) {
                double left[SD], right[SD];
                for (int c = 0; c < SD; c++) {
                    left[c] = ends[((size_t)i * n_draws + q) * BK::EZ + BK::L + c];
                    right[c] = ends[((size_t)i * n_draws + q) * BK::EZ + BK::R + c];
                }
                bridge_slot_walk<MODEL, D>(
                    par, pk[BK::DT], left, right, n_off, [&](int64_t r) -> double { return S.off_val[(size_t)(g0 + r)]; },
                    [&](int64_t r, double (&z)[SD]) { bridge_deviates<SD>(seed, (uint64_t)m, s, (uint32_t)r, (uint32_t)(draw0 + q), 0, z); },
                    [&](int64_t r, const double (&x)[SD]) {
                        for (int64_t k = S.q_ptr[(size_t)(g0 + r)]; k < S.q_ptr[(size_t)(g0 + r) + 1]; k++)
                            for (int c = 0; c < SD; c++) out[((int64_t)q * nq + S.q_dest[(size_t)k]) * SD + c] = x[c];
                    });
            }
        }
    }
}

template <class T>
void copy_out(const std::vector<T>& v, T* dst) { if (!v.empty()) memcpy(dst, v.data(), v.size() * sizeof(T)); }

}  // namespace

extern "C" {

int hostsim_predict_draws(int model, int d, TWIN_PARAMS, int64_t nq, const int64_t* q_row, const double* q_off, uint64_t seed,
                          int64_t draw0, int n_draws, double* out) {
#define PD(MODEL, D) if (model == MODEL && d == D) { run_predict_draws<MODEL, D>(TWIN_ARGS, nq, q_row, q_off, seed, draw0, n_draws, out); return 0; }
    TWIN_D12(PD)
#undef PD
    return 1;
}

// One bridge_step of (model, d): par [Q], the rest [SD]
int hostsim_bridge_step(int model, int d, const double* par, const double* x_prev, const double* alpha_next, double d1, double d2,
                        int tail, const double* z, double* x_out) {
#define BS(MODEL, D) if (model == MODEL && d == D) { \
        constexpr int SD = DenseDims<MODEL, D>::SD, Q = DenseDims<MODEL, D>::Q; \
        DualN<0> p[Q]; double xp[SD], an[SD], zz[SD], xo[SD]; \
        for (int j = 0; j < Q; j++) p[j] = DualN<0>(par[j]); \
        for (int c = 0; c < SD; c++) { xp[c] = x_prev[c]; an[c] = alpha_next[c]; zz[c] = z[c]; } \
        bridge_step<MODEL, D>(p, xp, an, d1, d2, tail != 0, zz, xo); \
        for (int c = 0; c < SD; c++) x_out[c] = xo[c]; \
        return 0; }
    TWIN_D12(BS)
#undef BS
    return 1;
}

// plan_queries + plan_slot_offsets over nl lanes and nq queries (pad_row NULL: the rows are the caller's).  q_slot, q_rank, q_dest,
// off_val, q_ptr (+ 1): room for nq (+ 1); off_ptr: nq + 1.  counts = planned queries, slots, distinct offsets, the longest list.
void hostsim_plan_slot_offsets(int64_t nl, const int64_t* row0, const int32_t* ns, const int64_t* pad_row, double pad_step, int64_t nq,
                               const int64_t* q_row, const double* q_off, int64_t* counts, int64_t* order, int64_t* q_slot,
                               int64_t* q_rank, int64_t* off_ptr, double* off_val, int64_t* q_ptr, int64_t* q_dest) {
    const ssde_plan::QueryPlan P = ssde_plan::plan_queries(std::vector<int64_t>(row0, row0 + nl), std::vector<int32_t>(ns, ns + nl),
                                                           pad_row, pad_step, q_row, q_off, nq);
    const ssde_plan::SlotOffsets S = ssde_plan::plan_slot_offsets(P);
    counts[0] = (int64_t)P.order.size(); counts[1] = (int64_t)P.want_step.size(); counts[2] = (int64_t)S.off_val.size(); counts[3] = S.most;
    copy_out(P.order, order); copy_out(P.q_slot, q_slot); copy_out(S.q_rank, q_rank); copy_out(S.off_ptr, off_ptr);
    copy_out(S.off_val, off_val); copy_out(S.q_ptr, q_ptr); copy_out(S.q_dest, q_dest);
}

int hostsim_predict_draws_batch_cap(int64_t budget, int64_t n_slots, int sd, int64_t n_query, int ch, int n_draws) {
    return ssde_plan::predict_draws_batch_cap(budget, n_slots, sd, n_query, ch, n_draws);
}

}  // extern "C"
