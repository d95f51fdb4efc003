// k_sim_rows.hip -- ssde_simulate_rows: replicate data sets simulated on the data's own rows, and their check statistics, for gfx950
// (include/ssde.h; lane math ssde_simrows.hpp; definitions DESIGN.md §3.19).  The reference's SDE$simulate (R/sde.R:1395-1508) with
// parameters that vary by row through the design blocks, dt = diff(time), tracks = ID segments and one coefficient row per replicate.
//
// simrows_kernel<KIND, D, KT>: one wave per block, lane = one (track, replicate) with the replicate fastest, so with 64 or more
// replicates a wave holds one track and every lane reads the same design row (one fetch), and with one replicate and many tracks the
// waves are full all the same.  The lane's coefficient row sits in dynamic LDS as [column][lane] (n_coef 64 doubles); a parameter whose
// block is the intercept alone is evaluated once, the others once per row, into a lane-private LDS slot [parameter][lane].  The
// recursion and the statistic accumulators stay in registers (D <= 2 or 8 columns bound at compile time; KT = 16 or 64 bounds the
// columns of one parameter's dot product).  obs_rep goes out through an LDS tile [column][lane][TT + 1] written along the rows: 64 / TT
// owners per store, TT consecutive rows each (TT = 32 for D <= 2, 8 for D = 8: 33.8 / 36.9 KB).
// Every load is at a row i in [row0[t], row0[t + 1]) of a lane's own track t < n_tracks and a column c < K_j; every obs store at
// (row0[t] + p) + n (c + d k) with p < rows of t, c < d, k < nb; every stats store at t + n_tracks (s + n_stat k), s < n_stat.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ssde.h"
#include "ssde_simrows.hpp"

namespace ssde_engine { extern thread_local std::string g_create_error; }   // what ssde_last_error(NULL) returns
#define g_simrows_error ssde_engine::g_create_error

namespace ssde {

namespace {

constexpr int RW = 64;     // one wave per block

template <int KIND, int D, int KT>
__global__ __launch_bounds__(RW) void simrows_kernel(const SimrowsArgs A) {
    constexpr int TT = D <= 2 ? 32 : 8;                  // rows of the tile
    constexpr int PER = RW / TT;                         // owners per store
    __shared__ double tile[D][RW][TT + 1];
    __shared__ double parv[SIMROWS_MAX_PAR][RW];
    __shared__ int64_t own_r0[RW], own_T[RW];
    __shared__ int own_k[RW];
    extern __shared__ double cf[];                       // [n_coef][RW]
    const int lane = threadIdx.x, d = A.d;
    const int64_t w = (int64_t)blockIdx.x * RW + lane;
    const bool valid = w < A.n_tracks * (int64_t)A.nb;
    const int64_t trk = valid ? w / A.nb : 0;
    const int kl = valid ? (int)(w % A.nb) : 0;
    const int64_t r0 = valid ? A.row0[trk] : 0;
    const int64_t T = valid ? A.row0[trk + 1] - r0 : 0;
    const int64_t crow = A.n_coeff_rows == 1 ? 0 : A.coef_first + kl;
    const uint32_t rep = (uint32_t)(A.rep_first + kl);
    own_r0[lane] = r0; own_T[lane] = T; own_k[lane] = kl;
    for (int c = 0; c < A.n_coef; c++) cf[c * RW + lane] = A.coeff[crow * A.n_coef + c];
    const double so = A.sigma_obs ? A.sigma_obs[crow] : 0.0;
    const bool with_error = so > 0.0;
    // the parameters whose block is the intercept alone: once
    unsigned varying = 0;
    for (int j = 0; j < A.n_par; j++) {
        if (A.kf[j] + A.kr[j] == 1 && !A.xf[j]) parv[j][lane] = bands_ginv(1.0 * cf[A.off[j] * RW + lane], A.link[j], 1);
        else varying |= 1u << j;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    int64_t Tmax = 0;
    for (int j = 0; j < RW; j++) Tmax = own_T[j] > Tmax ? own_T[j] : Tmax;

    double z[D], v[D], y[D];
    SSDE_RLOOP for (int c = 0; c < D; c++) { z[c] = c < d ? A.z0[c] : 0.0; v[c] = 0.0; y[c] = 0.0; }
    SimrowsAcc<D> acc;
    simrows_stat_init(acc);
    auto thr = [&](int r) -> double { return A.thr[r]; };

    for (int64_t t0 = 0; t0 < Tmax; t0 += TT) {
        for (int s = 0; s < TT; s++) {
            const int64_t p = t0 + s;
            if (p >= Tmax) break;
            if (p < T) {
                SimrowsFac F{};
                if (p > 0) {
                    const int64_t i1 = r0 + p - 1;                            // the row whose parameters the transition uses
                    for (int j = 0; j < A.n_par; j++) {
                        if (!((varying >> j) & 1u)) continue;
                        const int kf = A.kf[j], K = kf + A.kr[j];
                        const double* xf = A.xf[j];
                        const double* xr = A.xr[j];
                        const double* cj = cf + A.off[j] * RW + lane;
                        const double lp = bands_dot<KT>(
                            [&](int c) -> double { return c < kf ? (xf ? xf[i1 + A.ldx * c] : 1.0) : xr[i1 + A.ldx * (c - kf)]; },
                            [&](int c) -> double { return cj[c * RW]; }, K);
                        parv[j][lane] = bands_ginv(lp, A.link[j], 1);
                    }
                    const double p1 = parv[d][lane], p2 = A.n_par > d + 1 ? parv[d + 1][lane] : 0.0;
                    if (!bands_finite(p1) || !bands_finite(p2)) acc.bad = 1;
                    F = simrows_factors<KIND>(A.times[i1 + 1] - A.times[i1], p1, p2);
                }
                SSDE_RLOOP for (int c = 0; c < D; c++) {
                    if (c < d) {
                        double na, nb, no;
                        simrows_deviates<KIND>(A.k0, A.k1, (uint32_t)p, (uint32_t)trk, rep, c, with_error, na, nb, no);
                        if (p > 0) {
                            const double mu = parv[c][lane];
                            if (!bands_finite(mu)) acc.bad = 1;
                            simrows_step<KIND>(F, mu, na, nb, z[c], v[c]);
                        }
                        y[c] = fma(so, no, z[c]);
                        tile[c][lane][s] = y[c];
                    }
                }
                simrows_stat_row(acc, y, d, (uint32_t)p, thr, A.n_thr);
            }
        }
        if (A.obs) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            // the tile goes out along the rows: each group of TT lanes writes TT consecutive rows of one owner per store
            for (int j = 0; j < TT; j++) {
                const int o = j * PER + lane / TT, s = lane % TT;
                const int64_t p = t0 + s;
                if (p >= own_T[o]) continue;
                double* out = A.obs + (own_r0[o] + p) + A.n * ((int64_t)d * own_k[o]);
                SSDE_RLOOP for (int c = 0; c < D; c++)
                    if (c < d) out[A.n * c] = tile[c][o][s];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
    if (valid && A.stats) {
        double* st = A.stats + trk + A.n_tracks * ((int64_t)A.n_stat * kl);
        simrows_finish(acc, d, A.n_thr, T, [&](int s, double x) { st[A.n_tracks * s] = x; });
    }
}

bool simrows_args_ok(const SimrowsArgs& a) {
    if (a.kind < 0 || a.kind > 2 || a.d < 1 || a.d > SIMROWS_MAX_DIM || a.n_par != a.d + (a.kind == SIMROWS_BM ? 1 : 2)) return false;
    if (a.n_coef < a.n_par || a.n_coef > SIMROWS_MAX_COEF || a.n_thr < 0 || a.n_thr > SIMROWS_NTHR) return false;
    if (a.n_stat != 3 * a.d + 2 + a.n_thr || a.n_coeff_rows < 1 || a.nb < 1 || a.n < 0 || a.n_tracks < 1) return false;
    if (!a.row0 || !a.times || !a.coeff || (!a.obs && !a.stats)) return false;
    int off = 0;
    for (int j = 0; j < a.n_par; j++) {
        const int K = a.kf[j] + a.kr[j];
        if (a.kf[j] < 1 || a.kr[j] < 0 || K > BANDS_MAX_COLS || a.off[j] != off) return false;
        if ((!a.xf[j] && a.kf[j] != 1) || (!a.xr[j] && a.kr[j] != 0)) return false;
        off += K;
    }
    if (off != a.n_coef) return false;
    return (a.n_tracks * (int64_t)a.nb + RW - 1) / RW <= 0x7fffffff;
}

template <int KIND, int D, int KT>
hipError_t simrows_launch_one(const SimrowsArgs& a, hipStream_t s) {
    static bool set = false;
    if (!set) {
        const hipError_t e = hipFuncSetAttribute((const void*)simrows_kernel<KIND, D, KT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 SIMROWS_MAX_COEF * RW * (int)sizeof(double));
        if (e != hipSuccess) return e;
        set = true;
    }
    const dim3 grid((unsigned)((a.n_tracks * (int64_t)a.nb + RW - 1) / RW));
    hipLaunchKernelGGL((simrows_kernel<KIND, D, KT>), grid, dim3(RW), (size_t)a.n_coef * RW * sizeof(double), s, a);
    return hipGetLastError();
}

template <int KIND>
hipError_t simrows_launch_kind(const SimrowsArgs& a, hipStream_t s) {
    int kmax = 0;
    for (int j = 0; j < a.n_par; j++) kmax = std::max(kmax, a.kf[j] + a.kr[j]);
    if (a.d <= 2) return kmax <= 16 ? simrows_launch_one<KIND, 2, 16>(a, s) : simrows_launch_one<KIND, 2, 64>(a, s);
    return kmax <= 16 ? simrows_launch_one<KIND, 8, 16>(a, s) : simrows_launch_one<KIND, 8, 64>(a, s);
}

hipError_t launch_simrows(const SimrowsArgs& a, hipStream_t s) {
    if (!simrows_args_ok(a)) return hipErrorInvalidValue;
    if (a.kind == SIMROWS_CTCRW) return simrows_launch_kind<SIMROWS_CTCRW>(a, s);
    if (a.kind == SIMROWS_OU) return simrows_launch_kind<SIMROWS_OU>(a, s);
    return simrows_launch_kind<SIMROWS_BM>(a, s);
}

// device buffers of one call, freed on every way out
struct SimrowsBuffers {
    std::vector<void*> p;
    ~SimrowsBuffers() { for (void* q : p) (void)hipFree(q); }
    template <class T>
    hipError_t get(T** out, int64_t count) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, (size_t)(count > 0 ? count : 1) * sizeof(T));
        if (e == hipSuccess) { p.push_back(q); *out = (T*)q; }
        return e;
    }
};

int simrows_fail(int status, const char* what, hipError_t e) {
    g_simrows_error = std::string("ssde_simulate_rows: ") + what + (e != hipSuccess ? std::string(": ") + hipGetErrorString(e) : std::string());
    return status;
}

}  // namespace
}  // namespace ssde

extern "C" {

int ssde_simulate_rows(const ssde_simrows_desc* d, double* obs_rep, double* stats) {
    using namespace ssde;
#define SIMROWS_ARG(msg) return simrows_fail(SSDE_ERR_ARG, msg, hipSuccess)
    if (!d) SIMROWS_ARG("NULL descriptor");
    if (!obs_rep && !stats) SIMROWS_ARG("both outputs are NULL");
    if (d->abi_version != SSDE_ABI_VERSION) SIMROWS_ARG("descriptor built for another ABI version");
    if (d->flags & ~(SSDE_SIMROWS_DEVICE_DATA | SSDE_SIMROWS_DEVICE_OUT)) SIMROWS_ARG("unknown flag");
    SimrowsArgs a;
    memset(&a, 0, sizeof(a));
    switch (d->model) {
    case SSDE_MODEL_CTCRW: a.kind = SIMROWS_CTCRW; break;
    case SSDE_MODEL_OU: case SSDE_MODEL_OU_SSM: a.kind = SIMROWS_OU; break;
    case SSDE_MODEL_BM: case SSDE_MODEL_BM_SSM: a.kind = SIMROWS_BM; break;
    default: g_simrows_error = "Simulation not implemented yet for this model (R/sde.R:1496)"; return SSDE_ERR_MODEL;
    }
    if (d->n_dim < 1 || d->n_dim > SIMROWS_MAX_DIM) SIMROWS_ARG("n_dim in 1 .. 8 is required");
    const int q = d->n_dim + (a.kind == SIMROWS_BM ? 1 : 2);
    if (d->n_par != q) SIMROWS_ARG("n_par is n_dim + 1 (BM, BM_SSM) or n_dim + 2 (OU, OU_SSM, CTCRW)");
    if (d->n < 0 || d->n_tracks < 0 || d->n_tracks >= ((int64_t)1 << 32)) SIMROWS_ARG("n >= 0 and 0 <= n_tracks < 2^32 are required");
    if (!d->row0 || (!d->times && d->n > 0)) SIMROWS_ARG("NULL row0 / times");
    if (!d->ncol_fe || !d->ncol_re || !d->x_fe || !d->x_re || !d->link || !d->coeff) SIMROWS_ARG("NULL ncol_fe / ncol_re / x_fe / x_re / link / coeff");
    if (d->row0[0] != 0 || d->row0[d->n_tracks] != d->n) SIMROWS_ARG("row0[0] == 0 and row0[n_tracks] == n are required");
    for (int64_t t = 0; t < d->n_tracks; t++) {
        const int64_t len = d->row0[t + 1] - d->row0[t];
        if (len < 0 || d->row0[t + 1] > d->n) SIMROWS_ARG("row0 decreases or passes n");
        if (len >= ((int64_t)1 << 32)) SIMROWS_ARG("a track of 2^32 or more rows");
        for (int64_t i = d->row0[t] + 1; i < d->row0[t + 1]; i++) {
            const double dt = d->times[i] - d->times[i - 1];
            if (!(dt > 0.0) || !std::isfinite(dt)) SIMROWS_ARG("inside a track every time step must be finite and > 0");
        }
    }
    int n_coef = 0;
    for (int j = 0; j < q; j++) {
        const int kf = d->ncol_fe[j], kr = d->ncol_re[j];
        if (kf < 1 || kr < 0 || kf > SSDE_BANDS_MAX_COLS || kr > SSDE_BANDS_MAX_COLS || kf + kr > SSDE_BANDS_MAX_COLS)
            SIMROWS_ARG("ncol_fe >= 1, ncol_re >= 0 and ncol_fe + ncol_re <= SSDE_BANDS_MAX_COLS are required");
        if (!d->x_fe[j] && kf != 1) SIMROWS_ARG("a NULL fixed-effect block needs ncol_fe == 1 (the intercept)");
        if (!d->x_re[j] && kr != 0) SIMROWS_ARG("a NULL random-effect block needs ncol_re == 0");
        if (d->link[j] > 1) SIMROWS_ARG("link is 0 (identity) or 1 (log)");
        a.kf[j] = kf; a.kr[j] = kr; a.off[j] = n_coef; a.link[j] = d->link[j];
        n_coef += kf + kr;
    }
    if (d->n_coef != n_coef) SIMROWS_ARG("n_coef is not the sum of the blocks' columns");
    if (n_coef > SSDE_SIMROWS_MAX_COEF) SIMROWS_ARG("n_coef over SSDE_SIMROWS_MAX_COEF");
    if (d->rep0 < 0 || d->n_rep < 1 || d->rep0 + d->n_rep >= ((int64_t)1 << 28) || d->n_rep >= ((int64_t)1 << 28))
        SIMROWS_ARG("rep0 >= 0, n_rep >= 1 and rep0 + n_rep < 2^28 are required");
    if (d->n_coeff_rows != 1 && d->n_coeff_rows != d->n_rep) SIMROWS_ARG("n_coeff_rows is 1 or n_rep");
    const int64_t n_tab = (int64_t)d->n_coeff_rows * n_coef;
    for (int64_t e = 0; e < n_tab; e++)
        if (!std::isfinite(d->coeff[e])) SIMROWS_ARG("a coeff entry is not finite");
    if (d->sigma_obs)
        for (int k = 0; k < d->n_coeff_rows; k++)
            if (!(d->sigma_obs[k] >= 0.0) || !std::isfinite(d->sigma_obs[k])) SIMROWS_ARG("sigma_obs entries are finite and >= 0");
    for (int c = 0; c < d->n_dim; c++)
        if (!std::isfinite(d->z0[c])) SIMROWS_ARG("z0 is not finite");
    if (d->n_thr < 0 || d->n_thr > SSDE_SIMROWS_MAX_THR) SIMROWS_ARG("n_thr outside 0 .. SSDE_SIMROWS_MAX_THR");
    if (d->n_thr > 0 && !d->thr) SIMROWS_ARG("thr is NULL with n_thr > 0");
    for (int r = 0; r < d->n_thr; r++)
        if (!(d->thr[r] >= 0.0)) SIMROWS_ARG("a threshold is NaN or negative");
#undef SIMROWS_ARG
    const bool dev_data = d->flags & SSDE_SIMROWS_DEVICE_DATA, dev_out = d->flags & SSDE_SIMROWS_DEVICE_OUT;
    const int64_t n = d->n, M = d->n_tracks;
    const int n_dim = d->n_dim, n_stat = 3 * n_dim + 2 + d->n_thr;
    if (M == 0) return SSDE_OK;                            // no track: nothing to write

    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return simrows_fail(SSDE_ERR_NODEVICE, "no HIP device visible: there is no CPU fallback", hipSuccess);
    if (d->device >= 0 && hipSetDevice(d->device) != hipSuccess) return simrows_fail(SSDE_ERR_HIP, "hipSetDevice failed", hipSuccess);
    hipError_t e;
#define SIMROWS_HIP(call, what) do { e = (call); if (e != hipSuccess) return simrows_fail(e == hipErrorOutOfMemory ? SSDE_ERR_ALLOC : SSDE_ERR_HIP, what, e); } while (0)

    // the batch: what one replicate costs in staged outputs, against the budget
    const int64_t rep_bytes = (int64_t)sizeof(double) * ((obs_rep && !dev_out ? n * n_dim : 0) + (stats ? M * n_stat : 0));
    int64_t nb = d->n_rep;
    if (rep_bytes > 0) {
        int64_t budget = (int64_t)d->budget_mb << 20;
        if (d->budget_mb <= 0) {
            size_t fr = 0, tot = 0;
            SIMROWS_HIP(hipMemGetInfo(&fr, &tot), "hipMemGetInfo");
            budget = (int64_t)(fr / 4);
        }
        nb = std::max<int64_t>(1, std::min<int64_t>(nb, budget / rep_bytes));
    }
    nb = std::min<int64_t>(nb, ((int64_t)0x7fffffff * 64) / M);       // the grid's limit; M < 2^32 leaves 31 or more

    SimrowsBuffers buf;
    int64_t* d_row0 = nullptr;
    double *d_times = nullptr, *d_coeff = nullptr, *d_so = nullptr, *d_x = nullptr, *d_obs = nullptr, *d_stats = nullptr;
    SIMROWS_HIP(buf.get(&d_row0, M + 1), "hipMalloc (row0)");
    SIMROWS_HIP(hipMemcpy(d_row0, d->row0, (size_t)(M + 1) * sizeof(int64_t), hipMemcpyHostToDevice), "hipMemcpy (row0)");
    SIMROWS_HIP(buf.get(&d_times, n), "hipMalloc (times)");
    if (n > 0) SIMROWS_HIP(hipMemcpy(d_times, d->times, (size_t)n * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy (times)");
    SIMROWS_HIP(buf.get(&d_coeff, n_tab), "hipMalloc (coeff)");
    SIMROWS_HIP(hipMemcpy(d_coeff, d->coeff, (size_t)n_tab * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy (coeff)");
    if (d->sigma_obs) {
        SIMROWS_HIP(buf.get(&d_so, d->n_coeff_rows), "hipMalloc (sigma_obs)");
        SIMROWS_HIP(hipMemcpy(d_so, d->sigma_obs, (size_t)d->n_coeff_rows * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy (sigma_obs)");
    }
    a.ldx = n;
    if (dev_data) {
        for (int j = 0; j < q; j++) { a.xf[j] = d->x_fe[j]; a.xr[j] = d->x_re[j]; }
    } else {
        int64_t x_cols = 0;
        for (int j = 0; j < q; j++) x_cols += (d->x_fe[j] ? a.kf[j] : 0) + a.kr[j];
        if (x_cols && n > 0) SIMROWS_HIP(buf.get(&d_x, n * x_cols), "hipMalloc (design blocks)");
        double* w = d_x;
        for (int j = 0; j < q; j++) {
            if (d->x_fe[j] && n > 0) {
                SIMROWS_HIP(hipMemcpy(w, d->x_fe[j], (size_t)(n * a.kf[j]) * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy (x_fe)");
                a.xf[j] = w; w += n * a.kf[j];
            } else if (d->x_fe[j]) {
                a.xf[j] = d_times;                           // (n == 0: never read, but the block is not the intercept case)
            }
            if (d->x_re[j] && n > 0) {
                SIMROWS_HIP(hipMemcpy(w, d->x_re[j], (size_t)(n * a.kr[j]) * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy (x_re)");
                a.xr[j] = w; w += n * a.kr[j];
            } else if (d->x_re[j]) {
                a.xr[j] = d_times;
            }
        }
    }
    if (obs_rep && !dev_out) SIMROWS_HIP(buf.get(&d_obs, n * n_dim * nb), "hipMalloc (obs batch)");
    if (stats) SIMROWS_HIP(buf.get(&d_stats, M * n_stat * nb), "hipMalloc (stats batch)");

    a.d = n_dim; a.n_par = q; a.n_coef = n_coef; a.n_thr = d->n_thr; a.n_stat = n_stat; a.n_coeff_rows = d->n_coeff_rows;
    a.n = n; a.n_tracks = M; a.row0 = d_row0; a.times = d_times; a.coeff = d_coeff; a.sigma_obs = d_so;
    for (int c = 0; c < SIMROWS_MAX_DIM; c++) a.z0[c] = c < n_dim ? d->z0[c] : 0.0;
    for (int r = 0; r < d->n_thr; r++) a.thr[r] = d->thr[r];
    a.k0 = (uint32_t)d->seed; a.k1 = (uint32_t)(d->seed >> 32);
    hipStream_t s = nullptr;
    for (int64_t kb = 0; kb < d->n_rep; kb += nb) {
        const int64_t nc = std::min(nb, d->n_rep - kb);
        a.nb = (int)nc; a.rep_first = d->rep0 + kb; a.coef_first = d->n_coeff_rows == 1 ? 0 : kb;
        a.obs = !obs_rep ? nullptr : (dev_out ? obs_rep + n * n_dim * kb : d_obs);
        a.stats = d_stats;
        SIMROWS_HIP(launch_simrows(a, s), "launch");
        SIMROWS_HIP(hipStreamSynchronize(s), "kernel");
        if (obs_rep && !dev_out && n > 0)
            SIMROWS_HIP(hipMemcpy(obs_rep + n * n_dim * kb, d_obs, (size_t)(n * n_dim * nc) * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy (obs_rep)");
        if (stats)
            SIMROWS_HIP(hipMemcpy(stats + M * n_stat * kb, d_stats, (size_t)(M * n_stat * nc) * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy (stats)");
    }
#undef SIMROWS_HIP
    return SSDE_OK;
}

}  // extern "C"
