// k_path_prox.hip -- proximity of posterior paths between tracks for gfx950 (ssde_path_proximity; math in ssde_prox.hpp, definitions
// DESIGN.md §3.16).
//
// prox_tile_kernel: one workgroup of PROX_TILE = 256 threads per (tile, draw of the batch); lane t is the tile's point t.  It reads
// the D position doubles of both sides of its point from the batch buffer that predict_draws_query_kernel filled (element (k, c, q) at
// k + n_query * (c + n_col * q): consecutive lanes read consecutive k, every load coalesced), forms the point's ProxAcc, combines over
// the wave with __shfl_xor and over the four waves through ONE LDS array, and stores one partial record per (tile, draw).  The draws
// are folded into the grid's FIRST dimension (block = tile + n_tiles * draw), which takes 2^31 - 1 blocks: the second dimension's
// 65535 would cap the batch for no reason.
// prox_fold_kernel: lane = (pair, draw), pairs fastest; it combines the pair's tiles in ascending order and writes the n_stat doubles:
// store-then-fold, no atomics.  The combine is order-independent anyway (ssde_prox.hpp); the fixed order costs nothing.
// prox_gather_kernel: the position columns of one shard's batch buffer placed at the parent's query indices (route 2).
// 64-bit offsets throughout; every store is a plain C++ store.
#include "ssde_device.hpp"
#include "ssde_prox.hpp"

namespace ssde {

namespace {

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int o) { return (uint64_t)__shfl_xor((unsigned long long)v, o, 64); }

// combine with the lane `o` away, all 64 lanes taking part
__device__ __forceinline__ void prox_wave_step(ProxAcc& a, int o, int n_radii) {
    ProxAcc b;
    b.dist = __shfl_xor(a.dist, o, 64);
    b.idx = (int64_t)shfl_u64((uint64_t)a.idx, o);
    b.bad = shfl_u64(a.bad, o);
#pragma unroll
    for (int r = 0; r < PROX_NRAD; r++) b.sum[r] = r < n_radii ? shfl_u64(a.sum[r], o) : 0;
    prox_combine(a, b);
}

}  // namespace

template <int MODEL, int D>
__global__ __launch_bounds__(PROX_TILE) void prox_tile_kernel(const ProxArgs A) {
    typedef DenseDims<MODEL, D> DM;
    constexpr int NW = PROX_TILE / WAVE;
    __shared__ uint64_t lds[NW * PROX_REC];                         // the one LDS object of this kernel: a record per wave
    const int64_t tile = (int64_t)blockIdx.x % A.n_tiles, q = (int64_t)blockIdx.x / A.n_tiles;
    const int t = threadIdx.x, cnt = A.tile_count[tile];
    ProxAcc a;
    prox_init(a);
    if (t < cnt) {
        const int64_t i = A.tile_first[tile] + t;
        const double* base = A.pos + A.draw_stride * q + i;
        double pa[D], pb[D];
#pragma unroll
        for (int c = 0; c < D; c++) {
            const int64_t col = A.packed ? c : DM::z(c);
            pa[c] = base[col * A.n_query];
            pb[c] = base[col * A.n_query + A.n_point];
        }
        prox_step<D>(a, pa, pb, A.tile_idx0[tile] + t, A.wq ? A.wq[i] : A.unit, [&](int r) { return A.radii[r]; }, A.n_radii);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) prox_wave_step(a, o, A.n_radii);
    const int w = t / WAVE;
    if ((t & (WAVE - 1)) == 0) prox_store(a, lds + w, NW);
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int k = 1; k < NW; k++) {
            ProxAcc b;
            prox_load(b, lds + k, NW);
            prox_combine(a, b);
        }
        const int64_t n_rec = A.n_tiles * (int64_t)A.n_draws;
        prox_store(a, A.part + tile + A.n_tiles * q, n_rec);
    }
}

constexpr int PROX_FOLD_TB = 256;

__global__ __launch_bounds__(PROX_FOLD_TB) void prox_fold_kernel(const ProxArgs A) {
    const int64_t t = (int64_t)blockIdx.x * PROX_FOLD_TB + threadIdx.x;
    if (t >= A.n_pairs * (int64_t)A.n_draws) return;
    const int64_t p = t % A.n_pairs, q = t / A.n_pairs;
    const int64_t n_rec = A.n_tiles * (int64_t)A.n_draws;
    ProxAcc a;
    prox_init(a);
    for (int64_t k = A.pair_tile[p]; k < A.pair_tile[p + 1]; k++) {
        ProxAcc b;
        prox_load(b, A.part + k + A.n_tiles * q, n_rec);
        prox_combine(a, b);
    }
    double out[PROX_NSTAT_MAX];
    prox_finish(a, A.n_radii, A.e, out);
    const int n_stat = 2 + A.n_radii;
    double* dst = A.stats + p + A.n_pairs * (int64_t)n_stat * q;
#pragma unroll
    for (int k = 0; k < PROX_NSTAT_MAX; k++)
        if (k < n_stat) dst[A.n_pairs * (int64_t)k] = out[k];
}

// dst[idx[i] + n_dst * (c + D * q)] = src[i + n_src * (col(c) + n_col * q)] for i < n_src, c < D, q < n_draws: lane = (i, c, q), i
// fastest.  col_step: 2 for a CTCRW (positions at the even state columns), 1 otherwise.
__global__ __launch_bounds__(PROX_FOLD_TB) void prox_gather_kernel(const double* src, int64_t n_src, int n_col, int col_step, int D,
                                                                   int n_draws, const int64_t* idx, double* dst, int64_t n_dst) {
    const int64_t t = (int64_t)blockIdx.x * PROX_FOLD_TB + threadIdx.x;
    if (t >= n_src * (int64_t)D * n_draws) return;
    const int64_t i = t % n_src, c = (t / n_src) % D, q = t / (n_src * (int64_t)D);
    dst[idx[i] + n_dst * (c + (int64_t)D * q)] = src[i + n_src * (c * col_step + (int64_t)n_col * q)];
}

#define SSDE_PXALL(X) X(M_CTCRW, 1) X(M_CTCRW, 2) X(M_OU_SSM, 1) X(M_OU_SSM, 2) X(M_BM_SSM, 1) X(M_BM_SSM, 2)

hipError_t launch_prox_tile(const ProxArgs& a, hipStream_t s) {
    const int64_t blocks = a.n_tiles * (int64_t)a.n_draws;
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
#define SSDE_PXT(MODEL, D) \
    if (a.model == MODEL && a.d == D) { hipLaunchKernelGGL((prox_tile_kernel<MODEL, D>), grid, dim3(PROX_TILE), 0, s, a); return hipGetLastError(); }
    SSDE_PXALL(SSDE_PXT)
#undef SSDE_PXT
    return hipErrorInvalidValue;
}
#undef SSDE_PXALL

hipError_t launch_prox_fold(const ProxArgs& a, hipStream_t s) {
    const int64_t lanes = a.n_pairs * (int64_t)a.n_draws;
    if (lanes <= 0) return hipSuccess;
    const int64_t blocks = (lanes + PROX_FOLD_TB - 1) / PROX_FOLD_TB;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prox_fold_kernel, dim3((unsigned)blocks), dim3(PROX_FOLD_TB), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_prox_gather(const double* src, int64_t n_src, int n_col, int col_step, int d, int n_draws, const int64_t* idx,
                              double* dst, int64_t n_dst, hipStream_t s) {
    const int64_t lanes = n_src * (int64_t)d * n_draws;
    if (lanes <= 0) return hipSuccess;
    const int64_t blocks = (lanes + PROX_FOLD_TB - 1) / PROX_FOLD_TB;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prox_gather_kernel, dim3((unsigned)blocks), dim3(PROX_FOLD_TB), 0, s, src, n_src, n_col, col_step, d, n_draws, idx,
                       dst, n_dst);
    return hipGetLastError();
}

}  // namespace ssde
