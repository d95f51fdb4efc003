// hostsim_records.hpp -- TEST INFRASTRUCTURE, not an engine.
//
// What the host twins of the smoother's consumers share (hostsim.cpp: run_smooth, hostsim_draws.cpp, hostsim_predict.cpp,
// hostsim_path.cpp): the problem as tests/hostsim_lib.py marshals it, the forward record pass of one track the way one lane of the
// record kernels runs it, and the list of (MODEL, D) the twins are compiled for.  The backward walks stay with their twins.
#ifndef HOSTSIM_RECORDS_HPP
#define HOSTSIM_RECORDS_HPP

#include <cstdint>
#include <vector>

#include "../../smoothsde_amd/csrc/ssde_predict.hpp"

// parmat: n x q row-major linear predictors; harr: n x d x d (row-major per row) or NULL (h I); p0f: SD x SD column-major;
// a0: n_tracks x SD; track m holds the rows row0[m] .. row0[m] + nrows[m] - 1
struct TwinProblem {
    int any_nan;
    int64_t n, n_tracks;
    const int64_t *row0, *nrows;
    const double *times, *obs, *parmat, *harr;
    double h;
    const double *p0f, *a0;
};
#define TWIN_PARAMS int any_nan, int64_t n, int64_t n_tracks, const int64_t* row0, const int64_t* nrows, const double* times, \
                    const double* obs, const double* parmat, const double* harr, double h, const double* p0f, const double* a0
#define TWIN_ARGS TwinProblem{any_nan, n, n_tracks, row0, nrows, times, obs, parmat, harr, h, p0f, a0}

// the responses of one or two columns (every twin), and of three to eight (the smoother's only)
#define TWIN_D12(X) X(M_CTCRW, 1) X(M_CTCRW, 2) X(M_OU_SSM, 1) X(M_OU_SSM, 2) X(M_BM_SSM, 1) X(M_BM_SSM, 2)
#define TWIN_D38_OF(X, M) X(M, 3) X(M, 4) X(M, 5) X(M, 6) X(M, 7) X(M, 8)
#define TWIN_D38(X) TWIN_D38_OF(X, M_CTCRW) TWIN_D38_OF(X, M_OU_SSM) TWIN_D38_OF(X, M_BM_SSM)

// The records of track m's state rows (ns = nrows[m] - 1 of them, R doubles each) and, where `side` is given (D <= 2), the side
// rows of ssde_predict.  Returns ns (<= 0: no state row, nothing written).
template <int MODEL, int D>
int64_t twin_record_track(const TwinProblem& pb, int64_t m, std::vector<double>& recs, std::vector<double>* side = nullptr) {
    using namespace ssde;
    typedef DenseDims<MODEL, D> DM;
    constexpr int SD = DM::SD, Q = DM::Q, R = SmoothRec<MODEL, D>::R;
    const int64_t ns = pb.nrows[m] - 1, n = pb.n;
    if (ns <= 0) return ns;
    DenseLane<MODEL, D, 0> L;
    L.init(pb.a0 + m * SD, pb.p0f);
    recs.assign((size_t)ns * R, 0.0);
    if constexpr (D <= 2) { if (side) side->assign((size_t)ns * PredictPk<MODEL, D>::SW, 0.0); }
    for (int64_t s = 0; s < ns; s++) {
        const int64_t i = pb.row0[m] + 1 + s;
        const double dt = (i + 1 < n) ? pb.times[i + 1] - pb.times[i] : 1.0;
        double y[D];
        for (int c = 0; c < D; c++) y[c] = pb.obs[i + c * n];
        DualN<0> H[D][D], par[Q];
        for (int p = 0; p < D; p++)
            for (int q = 0; q < D; q++) H[p][q] = DualN<0>(pb.harr ? pb.harr[(i * D + p) * D + q] : (p == q ? pb.h : 0.0));
        for (int j = 0; j < Q; j++) par[j] = DualN<0>(pb.parmat[i * Q + j]);
        const bool na = is_na(y[0], pb.any_nan);
        double* rp = &recs[(size_t)s * R];
        const bool upd = smooth_record_row<MODEL, D>(L, par, H, dt, y, na, [&](int k) -> double& { return rp[k]; });
        if constexpr (D <= 2) {
            if (side) {
                constexpr int SW = PredictPk<MODEL, D>::SW;
                double* sp = &(*side)[(size_t)s * SW];
                predict_side_row<MODEL, D>(par, dt, na, upd, [&](int k) -> double& { return sp[k]; });
            }
        }
        dense_step<MODEL, D, 0>(L, par, H, dt, y, na);
    }
    return ns;
}

#endif
