// hostsim_predict.cpp -- TEST INFRASTRUCTURE, not an engine.
//
// Compiles smoothsde_amd/csrc/ssde_predict.hpp (the lane math of k_predict.hip) over ssde_smooth.hpp / ssde_dense.hpp with g++ and
// walks each track the way one lane of the kernels does: smooth_record_row + predict_side_row -> dense_step per state row, then from
// the last record to the first predict_packet_row (before the row is processed) and smooth_back_row; predict_query_row answers the
// queries from the packets.  tests/test_predict_hostsim.py compares it with tests/predict_ref.py.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../smoothsde_amd/csrc/ssde_predict.hpp"

using namespace ssde;

namespace {

// parmat: n x q row-major linear predictors; harr: n x d x d (row-major per row) or NULL (h I); p0f: SD x SD column-major;
// a0: n_tracks x SD.  Queries (q_row, q_off); a_pred (nq x SD) and P_pred (nq x SD x SD), row-major, are written where a state exists.
template <int MODEL, int D>
void run_predict(int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows, const double* times,
                 const double* obs, const double* parmat, const double* harr, double h, const double* p0f, const double* a0,
                 int64_t nq, const int64_t* q_row, const double* q_off, double* a_pred, double* P_pred) {
    typedef DenseDims<MODEL, D> DM;
    typedef SmoothRec<MODEL, D> RC;
    typedef PredictPk<MODEL, D> PK;
    constexpr int SD = DM::SD, Q = DM::Q, R = RC::R, SW = PK::SW, SZ = PK::SZ;
    std::vector<double> packets((size_t)n * SZ, 0.0);
    std::vector<char> has((size_t)n, 0);
    for (int64_t m = 0; m < n_tracks; m++) {
        const int64_t ns = nrows[m] - 1;
        if (ns <= 0) continue;
        DenseLane<MODEL, D, 0> L;
        L.init(a0 + m * SD, p0f);
        std::vector<double> recs((size_t)ns * R), side((size_t)ns * SW);
        for (int64_t s = 0; s < ns; s++) {
            const int64_t i = row0[m] + 1 + s;
            const double dt = (i + 1 < n) ? times[i + 1] - times[i] : 1.0;
            double y[D];
            for (int c = 0; c < D; c++) y[c] = obs[i + c * n];
            DualN<0> H[D][D], par[Q];
            for (int p = 0; p < D; p++)
                for (int q = 0; q < D; q++) H[p][q] = DualN<0>(harr ? harr[(i * D + p) * D + q] : (p == q ? h : 0.0));
            for (int j = 0; j < Q; j++) par[j] = DualN<0>(parmat[i * Q + j]);
            const bool na = is_na(y[0], any_nan);
            double* rp = &recs[(size_t)s * R];
            double* sp = &side[(size_t)s * SW];
            const bool upd = smooth_record_row<MODEL, D>(L, par, H, dt, y, na, [&](int k) -> double& { return rp[k]; });
            predict_side_row<MODEL, D>(par, dt, na, upd, [&](int k) -> double& { return sp[k]; });
            dense_step<MODEL, D, 0>(L, par, H, dt, y, na);
        }
        double r[SD] = {}, N[SD][SD] = {};
        for (int64_t s = ns - 1; s >= 0; s--) {
            const int64_t i = row0[m] + 1 + s;
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

}  // namespace

extern "C" {

int hostsim_predict(int model, int d, int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows,
                    const double* times, const double* obs, const double* parmat, const double* harr, double h, const double* p0f,
                    const double* a0, int64_t nq, const int64_t* q_row, const double* q_off, double* a_pred, double* P_pred) {
#define PR(MODEL, D) if (model == MODEL && d == D) { run_predict<MODEL, D>(any_nan, n, n_tracks, row0, nrows, times, obs, parmat, harr, h, p0f, a0, nq, q_row, q_off, a_pred, P_pred); return 0; }
    PR(M_CTCRW, 1) PR(M_CTCRW, 2) PR(M_OU_SSM, 1) PR(M_OU_SSM, 2) PR(M_BM_SSM, 1) PR(M_BM_SSM, 2)
#undef PR
    return 1;
}

int hostsim_predict_packet_doubles(int model, int d) {
#define PD(MODEL, D) if (model == MODEL && d == D) return PredictPk<MODEL, D>::SZ;
    PD(M_CTCRW, 1) PD(M_CTCRW, 2) PD(M_OU_SSM, 1) PD(M_OU_SSM, 2) PD(M_BM_SSM, 1) PD(M_BM_SSM, 2)
#undef PD
    return 0;
}

}  // extern "C"
