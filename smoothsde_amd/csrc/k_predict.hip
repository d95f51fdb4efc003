// k_predict.hip -- the state at any time from the smoother's records for gfx950 (ssde_predict; math in ssde_predict.hpp, definitions
// DESIGN.md §3.11).
//
// predict_walk_kernel: smooth_back_kernel's walk (lane = track, one wave per group of 64 tracks, the records' 512-B wave loads,
// smooth_back_row unchanged) without the smoother's n-row outputs.  Each lane holds a cursor into its own list of wanted steps;
// before it processes a wanted step it stores that step's packet (filtered moments, the r and N it holds at that moment, the row's
// linear predictors and interval) into the step's slot.  Packets are slot-minor (double k of slot i at pk + k * stride + i), so the
// query kernel's loads coalesce over consecutive slots.
// predict_query_kernel: lane = query, in slot order; one prediction step over the offset and the correction by the interval's right
// end, written to the caller's row of the outputs.  64-bit offsets throughout.
#include "ssde_device.hpp"
#include "ssde_predict.hpp"

namespace ssde {

template <int MODEL, int D>
__global__ __launch_bounds__(WAVE) void predict_walk_kernel(const PredictArgs A) {
    typedef SmoothRec<MODEL, D> RC;
    typedef PredictPk<MODEL, D> PK;
    constexpr int SD = RC::SD;
    const RecLane L = rec_lane(A.s);
    const int ns = L.ns;
    const int64_t w0 = L.has ? A.want_off[L.l] : 0;
    int64_t cur = L.has ? A.want_off[L.l + 1] - 1 : -1;        // the lane's wanted steps ascend: the walk takes them from the end
    int next = cur >= w0 ? A.want_step[cur] : -1;
    // the wave stops below its lowest wanted step: nothing under it is asked for
    int smin = cur >= w0 ? A.want_step[w0] : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) smin = min(smin, __shfl_xor(smin, o, 64));
    smin = __builtin_amdgcn_readfirstlane(smin);
    double r[SD], N[SD][SD];
#pragma unroll
    for (int a = 0; a < SD; a++) {
        r[a] = 0.0;
#pragma unroll
        for (int b = 0; b < SD; b++) N[a][b] = 0.0;
    }
    for (int s = L.smax - 1; s >= smin; s--) {
        if (s >= ns) continue;
        const RecRow rec = L.row<RC::R>(s);
        if (s == next) {
            double* pp = A.pk + (cur - A.slot0);
            predict_packet_row<MODEL, D, SD>(rec, rec_side_row<RC::R, PK::SW>(A.s.rc, L.goff, L.lane, s), r, N, s == ns - 1,
                                             [&](int k) -> double& { return pp[(int64_t)k * A.pk_stride]; });
            cur--;
            next = cur >= w0 ? A.want_step[cur] : -1;
        }
        double am[SD], V[SD][SD];
        smooth_back_row<MODEL, D, SD>(r, N, s == ns - 1, rec, am, V);
    }
}

constexpr int PREDICT_QB = 256;

template <int MODEL, int D>
__global__ __launch_bounds__(PREDICT_QB) void predict_query_kernel(const PredictArgs A) {
    typedef PredictPk<MODEL, D> PK;
    constexpr int SD = PK::SD;
    const int64_t i = A.q0 + (int64_t)blockIdx.x * PREDICT_QB + threadIdx.x;
    if (i >= A.q1) return;
    const double* pp = A.pk + (A.q_slot[i] - A.slot0);
    double am[SD], V[SD][SD];
    if (!predict_query_row<MODEL, D, SD>([&](int k) -> double { return pp[(int64_t)k * A.pk_stride]; }, A.q_off[i], am, V)) return;
    const int64_t row = A.order[i], n = A.n_query;
#pragma unroll
    for (int c = 0; c < SD; c++) A.a_pred[row + (int64_t)c * n] = am[c];
    if (A.P_pred) {
#pragma unroll
        for (int c = 0; c < SD; c++)
#pragma unroll
            for (int q = 0; q < SD; q++) A.P_pred[row + n * ((int64_t)q + (int64_t)SD * c)] = V[q][c];
    }
}

#define SSDE_PALL(X) X(M_CTCRW, 1) X(M_CTCRW, 2) X(M_OU_SSM, 1) X(M_OU_SSM, 2) X(M_BM_SSM, 1) X(M_BM_SSM, 2)

int predict_packet_doubles(int model, int d) {
#define SSDE_PP(MODEL, D) if (model == MODEL && d == D) return PredictPk<MODEL, D>::SZ;
    SSDE_PALL(SSDE_PP)
#undef SSDE_PP
    return 0;
}

int predict_side_doubles(int model, int d) {
#define SSDE_PS(MODEL, D) if (model == MODEL && d == D) return PredictPk<MODEL, D>::SW;
    SSDE_PALL(SSDE_PS)
#undef SSDE_PS
    return 0;
}

hipError_t launch_predict_walk(const PredictArgs& a, hipStream_t s) {
    if (a.s.rc.n_groups == 0) return hipSuccess;
#define SSDE_PW(MODEL, D) \
    if (a.s.model == MODEL && a.s.d == D) { hipLaunchKernelGGL((predict_walk_kernel<MODEL, D>), dim3(a.s.rc.n_groups), dim3(WAVE), 0, s, a); return hipGetLastError(); }
    SSDE_PALL(SSDE_PW)
#undef SSDE_PW
    return hipErrorInvalidValue;
}

hipError_t launch_predict_query(const PredictArgs& a, hipStream_t s) {
    if (a.q1 <= a.q0) return hipSuccess;
    const dim3 grid((unsigned)((a.q1 - a.q0 + PREDICT_QB - 1) / PREDICT_QB));
#define SSDE_PQ(MODEL, D) \
    if (a.s.model == MODEL && a.s.d == D) { hipLaunchKernelGGL((predict_query_kernel<MODEL, D>), grid, dim3(PREDICT_QB), 0, s, a); return hipGetLastError(); }
    SSDE_PALL(SSDE_PQ)
#undef SSDE_PQ
    return hipErrorInvalidValue;
}
#undef SSDE_PALL

}  // namespace ssde
