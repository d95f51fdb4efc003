// k_par_bands.hip -- confidence bands of the SDE parameters for gfx950 (ssde_par_bands; math in ssde_bands.hpp, definitions
// DESIGN.md §3.18).  Three passes over one chunk of whole rows, one wave per block:
//   bands_rows_kernel<KT>   pass 1, lane = row, blockIdx.y = parameter.  The lane holds its row's K <= KT design values in registers and
//       walks the n_post draws in order; a draw's coefficients are the same for every lane (uniform loads).  The m smallest and the m
//       largest linear predictors of each lane live in LDS, slot-major ([slot][lane]: a wave's access to one slot is 64 consecutive
//       doubles, and lanes at different slots still sit on their own banks), 2 m 64 doubles of dynamic LDS per wave (64 KiB at the cap
//       m = 64); the two cut-offs are registers, and an insert runs only where a value beats one.  After the walk bands_finish reads
//       the order statistics and the lane stores est / pw_low / pw_upp and, for the later passes, lp0 / se.
//   bands_dev_kernel<KT>    pass 2, lane = draw, blockIdx = (row block, block of 64 draws, parameter).  The lane holds coeff[k] -
//       coeff[0] of its draw in registers; the rows of the block are streamed with addresses that are the same for every lane,
//       together with the row's se; each lane keeps a running maximum of |dev / se| and stores it plainly at [row block][j][k].
//   bands_max_kernel        the maxima of the row blocks in the order of the blocks, max-ed into max_dev[j][k] (which carries the
//       earlier chunks).  A maximum: any order gives the same bits.
//   bands_sim_kernel        pass 3, elementwise g(lp0 -+ crit se).
// 64-bit offsets throughout.  Every load and store is at row i < n of a column c < K_j of a block or an output (i and the draw k are
// clamped or masked where a block overhangs), or at part[(rb n_par + j) n_post + k - 1] with rb < gridDim.x, k <= n_post.
#include <hip/hip_runtime.h>

#include "ssde_bands.hpp"

namespace ssde {

namespace {

constexpr int BW = 64;     // one wave per block

// the design value of column c of parameter j at row i (c < K_j): fixed-effect columns first; a NULL fixed-effect block is a column of ones
__device__ __forceinline__ double bands_x(const BandsArgs& A, int j, int kf, int64_t i, int c) {
    if (c < kf) return A.xf[j] ? A.xf[j][i + A.ldx * c] : 1.0;
    return A.xr[j][i + A.ldx * (c - kf)];
}

template <int KT>
__global__ __launch_bounds__(BW) void bands_rows_kernel(const BandsArgs A) {
    extern __shared__ double tails[];
    const int lane = threadIdx.x, j = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * BW + lane;
    const bool has = i0 < A.n;
    const int64_t i = has ? i0 : A.n - 1;                                  // a lane past the end walks the last row and stores nothing
    const int kf = A.kf[j], K = kf + A.kr[j], m = A.plan.m;
    double x[KT];
#pragma unroll
    for (int c = 0; c < KT; c++) x[c] = c < K ? bands_x(A, j, kf, i, c) : 0.0;
    auto xv = [&](int c) -> double { return x[c]; };
    auto lo = [&](int s) -> double& { return tails[(int64_t)s * BW + lane]; };
    auto up = [&](int s) -> double& { return tails[(int64_t)(m + s) * BW + lane]; };
    const double* c0 = A.coeff + A.off[j];
    const double lp0 = bands_dot<KT>(xv, [&](int c) -> double { return c0[c]; }, K);
    bool bad = !bands_finite(lp0);
    int n_lo = 0, n_up = 0;
    double cut_lo = INFINITY, cut_up = INFINITY;
    for (int k = 1; k <= A.n_post; k++) {
        const double* cf = c0 + (int64_t)k * A.n_coef;
        const double lp = bands_dot<KT>(xv, [&](int c) -> double { return cf[c]; }, K);
        if (!bands_finite(lp)) bad = true;
        if (lp < cut_lo) tail_insert(lo, m, n_lo, cut_lo, lp);
        const double nl = -lp;
        if (nl < cut_up) tail_insert(up, m, n_up, cut_up, nl);
    }
    if (n_lo < m || n_up < m) bad = true;                                  // (only where a value was NaN: n_post >= m)
    const BandsRow r = bands_finish(lo, up, A.plan, lp0, bad, A.link[j], A.resp, A.z);
    if (!has) return;
    if (A.est) A.est[i + A.ldo * j] = r.est;
    if (A.pw_low) A.pw_low[i + A.ldo * j] = r.pw_low;
    if (A.pw_upp) A.pw_upp[i + A.ldo * j] = r.pw_upp;
    if (A.lp0) A.lp0[i + A.lds * j] = r.lp0;
    if (A.se) A.se[i + A.lds * j] = r.se;
}

template <int KT>
__global__ __launch_bounds__(BW) void bands_dev_kernel(const BandsArgs A) {
    const int lane = threadIdx.x, j = blockIdx.z;
    const int k0 = 1 + (int)blockIdx.y * BW + lane;
    const bool has = k0 <= A.n_post;
    const int k = has ? k0 : A.n_post;
    const int kf = A.kf[j], K = kf + A.kr[j];
    const double* c0 = A.coeff + A.off[j];
    const double* ck = c0 + (int64_t)k * A.n_coef;
    double dc[KT];
#pragma unroll
    for (int c = 0; c < KT; c++) dc[c] = c < K ? ck[c] - c0[c] : 0.0;
    auto dv = [&](int c) -> double { return dc[c]; };
    const int64_t r0 = (int64_t)blockIdx.x * A.rows_per_block;
    const int64_t r1 = r0 + A.rows_per_block < A.n ? r0 + A.rows_per_block : A.n;
    const double* se = A.se + A.lds * j;
    double mx = 0.0;
    for (int64_t i = r0; i < r1; i++) {                                    // i, and every address below, is the same in every lane
        const double s = se[i];
        const double dev = bands_dot<KT>([&](int c) -> double { return bands_x(A, j, kf, i, c); }, dv, K);
        const double a = bands_ratio(dev, s);
        if (s == s && a > mx) mx = a;                                      // se is NaN exactly on the rows that take no part
    }
    if (has) A.part[((int64_t)blockIdx.x * A.n_par + j) * A.n_post + (k - 1)] = mx;
}

__global__ __launch_bounds__(BW) void bands_max_kernel(const BandsArgs A, int n_blocks) {
    const int64_t tot = (int64_t)A.n_par * A.n_post;
    const int64_t e = (int64_t)blockIdx.x * BW + threadIdx.x;
    if (e >= tot) return;
    double mx = A.max_dev[e];
    for (int b = 0; b < n_blocks; b++) {
        const double a = A.part[(int64_t)b * tot + e];
        if (a > mx) mx = a;
    }
    A.max_dev[e] = mx;
}

__global__ __launch_bounds__(BW) void bands_sim_kernel(const BandsArgs A) {
    const int j = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * BW + threadIdx.x;
    if (i >= A.n) return;
    const double lp0 = A.lp0[i + A.lds * j], se = A.se[i + A.lds * j], crit = A.crit[j];
    const bool nan = !(se == se);
    const double qn = __builtin_nan("");
    if (A.sim_low) A.sim_low[i + A.ldo * j] = nan ? qn : bands_ginv(bands_sim(lp0, se, crit, 0), A.link[j], A.resp);
    if (A.sim_upp) A.sim_upp[i + A.ldo * j] = nan ? qn : bands_ginv(bands_sim(lp0, se, crit, 1), A.link[j], A.resp);
}

int bands_kmax(const BandsArgs& a) {
    int k = 0;
    for (int j = 0; j < a.n_par; j++) k = a.kf[j] + a.kr[j] > k ? a.kf[j] + a.kr[j] : k;
    return k;
}

bool bands_args_ok(const BandsArgs& a) {
    if (a.n < 1 || a.n_par < 1 || a.n_par > BANDS_MAX_PAR || a.n_post < 2 || !a.coeff) return false;
    if (a.plan.m < 1 || a.plan.m > BANDS_MAX_TAIL || a.plan.m > a.n_post) return false;
    for (int j = 0; j < a.n_par; j++) {
        const int K = a.kf[j] + a.kr[j];
        if (a.kf[j] < 1 || a.kr[j] < 0 || K > BANDS_MAX_COLS) return false;
        if ((!a.xf[j] && a.kf[j] != 1) || (!a.xr[j] && a.kr[j] != 0)) return false;
    }
    return (a.n + BW - 1) / BW <= 0x7fffffff;
}

}  // namespace

// one instantiation per bound on the columns: the registers of a lane hold KT design values (pass 1) or differences (pass 2)
#define SSDE_BANDS_KT(CALL) \
    if (kmax <= 4) { CALL(4); } else if (kmax <= 16) { CALL(16); } else { CALL(64); }

hipError_t launch_bands_rows(const BandsArgs& a, hipStream_t s) {
    if (!bands_args_ok(a)) return hipErrorInvalidValue;
    const int kmax = bands_kmax(a);
    const dim3 grid((unsigned)((a.n + BW - 1) / BW), (unsigned)a.n_par);
    const size_t lds = (size_t)2 * a.plan.m * BW * sizeof(double);
#define SSDE_BR(KT) \
    { static bool set = false; \
      if (!set) { (void)hipFuncSetAttribute((const void*)bands_rows_kernel<KT>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * BANDS_MAX_TAIL * BW * (int)sizeof(double)); set = true; } \
      hipLaunchKernelGGL((bands_rows_kernel<KT>), grid, dim3(BW), lds, s, a); }
    SSDE_BANDS_KT(SSDE_BR)
#undef SSDE_BR
    return hipGetLastError();
}

// n_blocks: the row blocks of the chunk, (n + rows_per_block - 1) / rows_per_block <= BANDS_MAX_ROW_BLOCKS; part holds n_blocks n_par n_post doubles
hipError_t launch_bands_dev(const BandsArgs& a, hipStream_t s) {
    if (!bands_args_ok(a) || !a.se || !a.part || !a.max_dev || a.rows_per_block < BW) return hipErrorInvalidValue;
    const int64_t n_blocks = (a.n + a.rows_per_block - 1) / a.rows_per_block;
    if (n_blocks > BANDS_MAX_ROW_BLOCKS) return hipErrorInvalidValue;
    const int kmax = bands_kmax(a);
    const dim3 grid((unsigned)n_blocks, (unsigned)((a.n_post + BW - 1) / BW), (unsigned)a.n_par);
    if (grid.y > 65535u) return hipErrorInvalidValue;
#define SSDE_BD(KT) hipLaunchKernelGGL((bands_dev_kernel<KT>), grid, dim3(BW), 0, s, a)
    SSDE_BANDS_KT(SSDE_BD)
#undef SSDE_BD
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t tot = (int64_t)a.n_par * a.n_post;
    hipLaunchKernelGGL(bands_max_kernel, dim3((unsigned)((tot + BW - 1) / BW)), dim3(BW), 0, s, a, (int)n_blocks);
    return hipGetLastError();
}

hipError_t launch_bands_sim(const BandsArgs& a, hipStream_t s) {
    if (!bands_args_ok(a) || !a.se || !a.lp0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.n + BW - 1) / BW), (unsigned)a.n_par);
    hipLaunchKernelGGL(bands_sim_kernel, grid, dim3(BW), 0, s, a);
    return hipGetLastError();
}

}  // namespace ssde
