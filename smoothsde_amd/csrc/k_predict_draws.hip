// k_predict_draws.hip -- joint posterior draws of the state at any time for gfx950 (ssde_predict_draws; math in ssde_bridge.hpp,
// definitions DESIGN.md §3.14).
//
// predict_draws_walk_kernel: smooth_draws_kernel's walk (rec_draw_walk: lane = track, one wave per (group of 64 tracks, chunk of
// DRAW_CH draws)) with the n-row stores replaced by the ends of the wanted intervals.  Each lane holds predict_walk_kernel's cursor
// into its own list of wanted steps; at step s a path's state goes to the LEFT end of slot(s) when s is wanted and to the RIGHT end
// of slot(s - 1) when s - 1 is, and the slot's side packet (linear predictors, interval) is stored once per slot by the wave of the
// first chunk of draws.  Packets are slot-minor (double k of slot i at base + k * stride + i): a wave's stores of one double land in
// as many runs as it has lanes with a wanted step there, and the next kernel's loads coalesce over consecutive slots.  The wave stops
// below its lowest wanted step.
// predict_draws_query_kernel: lane = (slot, draw), slots fastest; bridge_slot_walk chains the slot's distinct offsets in ascending
// order from a CSR list and every answer is scattered to all the caller's queries that carry that offset.  A slot with many offsets
// (a long forecast) is a long loop in one lane.  64-bit offsets throughout.
#include "ssde_device.hpp"
#include "ssde_bridge.hpp"

namespace ssde {

template <int MODEL, int D>
__global__ __launch_bounds__(WAVE) void predict_draws_walk_kernel(const PredictDrawArgs A) {
    typedef SmoothRec<MODEL, D> RC;
    typedef BridgePk<MODEL, D> BK;
    constexpr int SD = RC::SD;
    const RecLane L = rec_lane(A.d.s);
    const int k0 = blockIdx.y * DRAW_CH;
    const uint64_t trk = L.has ? (uint64_t)(A.d.track0 + A.d.lane_trk[L.l]) : 0;
    const int64_t w0 = L.has ? A.want_off[L.l] : 0;
    int64_t cur = L.has ? A.want_off[L.l + 1] - 1 : -1;        // the lane's wanted steps ascend: the walk takes them from the end
    int next = cur >= w0 ? A.want_step[cur] : -1;
    int smin = cur >= w0 ? A.want_step[w0] : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) smin = min(smin, __shfl_xor(smin, o, 64));
    smin = __builtin_amdgcn_readfirstlane(smin);
    const int64_t stride = A.pk_stride;
    int64_t il = -1, ir = -1;                                   // this step's slots (chunk-relative): left end here, right end here
    rec_draw_walk<MODEL, D, DRAW_CH>(
        L, A.d.seed, trk, A.d.draw0 + (uint32_t)k0, A.d.col0,
        [&](int64_t row) {
            const int s = (int)(row - L.row0 - 1);
            il = -1;
            if (s == next) {
                il = cur - A.slot0;
                if (blockIdx.y == 0) {
                    double* sp = A.sidepk + il;
                    bridge_side_row<MODEL, D>(rec_side_row<RC::R, BK::SW>(A.d.s.rc, L.goff, L.lane, s), s == L.ns - 1,
                                              [&](int k) -> double& { return sp[(int64_t)k * stride]; });
                }
                cur--;
                next = cur >= w0 ? A.want_step[cur] : -1;
            }
            ir = (next >= 0 && next == s - 1) ? cur - A.slot0 : -1;
        },
        [&](int q, const double (&al)[SD]) {
            if (k0 + q >= A.d.n_draws) return;
            double* e = A.ends + (int64_t)(k0 + q) * BK::EZ * stride;
            if (il >= 0) {
#pragma unroll
                for (int c = 0; c < SD; c++) e[(int64_t)(BK::L + c) * stride + il] = al[c];
            }
            if (ir >= 0) {
#pragma unroll
                for (int c = 0; c < SD; c++) e[(int64_t)(BK::R + c) * stride + ir] = al[c];
            }
        },
        smin);
}

constexpr int PREDICT_DRAWS_QB = 256;

template <int MODEL, int D>
__global__ __launch_bounds__(PREDICT_DRAWS_QB) void predict_draws_query_kernel(const PredictDrawArgs A) {
    typedef BridgePk<MODEL, D> BK;
    constexpr int SD = BK::SD, Q = BK::Q;
    const int64_t t = (int64_t)blockIdx.x * PREDICT_DRAWS_QB + threadIdx.x, stride = A.pk_stride;
    if (t >= stride * (int64_t)A.d.n_draws) return;
    const int64_t i = t % stride, q = t / stride, slot = A.slot0 + i;
    const double* sp = A.sidepk + i;
    const double* e = A.ends + q * BK::EZ * stride + i;
    const double dt = sp[(int64_t)BK::DT * stride];
    DualN<0> par[Q];
#pragma unroll
    for (int j = 0; j < Q; j++) par[j] = DualN<0>(sp[(int64_t)(BK::PAR + j) * stride]);
    double left[SD], right[SD];
#pragma unroll
    for (int c = 0; c < SD; c++) {
        left[c] = e[(int64_t)(BK::L + c) * stride];
        right[c] = dt < 0.0 ? 0.0 : e[(int64_t)(BK::R + c) * stride];      // (a tail has no right end: nothing was stored)
    }
    const int64_t g0 = A.off_ptr[slot], n_off = A.off_ptr[slot + 1] - g0;
    const uint64_t trk = (uint64_t)(A.d.track0 + A.d.lane_trk[A.slot_lane[slot]]);
    const uint32_t s = (uint32_t)A.want_step[slot], draw = A.d.draw0 + (uint32_t)q;
    const int64_t n = A.n_query;
    double* out = A.out + n * SD * q;
    bridge_slot_walk<MODEL, D>(
        par, dt, left, right, n_off, [&](int64_t r) -> double { return A.off_val[g0 + r]; },
        [&](int64_t r, double (&z)[SD]) { bridge_deviates<SD>(A.d.seed, trk, s, (uint32_t)r, draw, A.d.col0, z); },
        [&](int64_t r, const double (&x)[SD]) {
            for (int64_t k = A.q_ptr[g0 + r]; k < A.q_ptr[g0 + r + 1]; k++) {
                const int64_t dst = A.q_dest[k];
#pragma unroll
                for (int c = 0; c < SD; c++) out[dst + (int64_t)c * n] = x[c];
            }
        });
}

#define SSDE_PDALL(X) X(M_CTCRW, 1) X(M_CTCRW, 2) X(M_OU_SSM, 1) X(M_OU_SSM, 2) X(M_BM_SSM, 1) X(M_BM_SSM, 2)

hipError_t launch_predict_draws_walk(const PredictDrawArgs& a, hipStream_t s) {
    if (a.d.s.rc.n_groups == 0 || a.d.n_draws <= 0 || a.pk_stride <= 0) return hipSuccess;
    const dim3 grid((unsigned)a.d.s.rc.n_groups, (unsigned)((a.d.n_draws + DRAW_CH - 1) / DRAW_CH));
    if (grid.y > 65535u) return hipErrorInvalidValue;
#define SSDE_PDW(MODEL, D) \
    if (a.d.s.model == MODEL && a.d.s.d == D) { hipLaunchKernelGGL((predict_draws_walk_kernel<MODEL, D>), grid, dim3(WAVE), 0, s, a); return hipGetLastError(); }
    SSDE_PDALL(SSDE_PDW)
#undef SSDE_PDW
    return hipErrorInvalidValue;
}

hipError_t launch_predict_draws_query(const PredictDrawArgs& a, hipStream_t s) {
    const int64_t lanes = a.pk_stride * (int64_t)a.d.n_draws;
    if (lanes <= 0) return hipSuccess;
    const int64_t blocks = (lanes + PREDICT_DRAWS_QB - 1) / PREDICT_DRAWS_QB;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
#define SSDE_PDQ(MODEL, D) \
    if (a.d.s.model == MODEL && a.d.s.d == D) { hipLaunchKernelGGL((predict_draws_query_kernel<MODEL, D>), grid, dim3(PREDICT_DRAWS_QB), 0, s, a); return hipGetLastError(); }
    SSDE_PDALL(SSDE_PDQ)
#undef SSDE_PDQ
    return hipErrorInvalidValue;
}
#undef SSDE_PDALL

}  // namespace ssde
