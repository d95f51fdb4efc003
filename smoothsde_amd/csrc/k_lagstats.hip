// k_lagstats.hip -- the lag statistics of a stationary batch (ssde_create, once).  The bulk forms built from them at every
// evaluation that takes that path run on the host (ssde_lagforms.hpp).  Derivation and layout: ssde_lagstats.hpp, DESIGN.md
// §3.3d.  Every sum runs in a fixed order: two creates of the same data give bitwise-equal statistics.  The kernels come in two
// compile-time modes: the increments y_t - y_{t-1} (CTCRW, BM_SSM) and the levels y_t - ref (OU_SSM).
#include "ssde_device.hpp"
#include "ssde_lagstats.hpp"
#include "ssde_headforms.hpp"

namespace ssde {

namespace {

constexpr int LAG_NB = LAG_N / LAG_LB;        // lag blocks of the Toeplitz pass

// what the levels mode centres the data on (ssde_lagstats.hpp), by value
struct LagRef { double v[2]; };

// Toeplitz lag sums Q_l = sum_{t = LAG_A}^{n - 1} Dy_t Dy_{t-l} (summed over the coordinates) of the 64 tracks of a group, for the
// LAG_LB lags of one block: one wave per (group, lag block), lane = track.  The rows walk in blocks of LAG_LB; the lagged
// increments of the block before stay in registers (old), so each row is loaded twice per work item: as the current row and
// as the lagged one.  A lane without a bulk (n <= LAG_A, or no track) contributes zeros; rows past a lane's track are zeroed
// before they are multiplied (the tile slots there hold whatever the layout put there).
// LEVELS (OU_SSM): the same sums of the levels z_t = y_t - ref_a instead of the increments, and -- from the waves of lag block 0 --
// s0g[g][a] = sum_{t >= LAG_A} z_{a,t} of the group, which no longer telescopes.
// EARLY (an early cut, ssde_lagstats.hpp; increments only): the first bulk row is `cut` instead of LAG_A and every track is cut off after
// LAG_A rows -- the head rows' own contribution.  Only the lags < cut mean anything: a lag block past them writes zeros; inside the
// block that straddles the cut the rows before row 0 a lag >= cut would read are clamped to row 0 (nothing reads those sums).
template <bool LEVELS, bool EARLY>
__global__ __launch_bounds__(WG_WAVES * WAVE) void lag_toeplitz_kernel(const TileView tv, int d, double* Qg, const LagRef ref, double* s0g, int cut) {
    static_assert(!(LEVELS && EARLY), "early cuts: the increments");
    const int id = blockIdx.x * WG_WAVES + (threadIdx.x >> 6);
    const int g = id / LAG_NB, b = id % LAG_NB;
    if (g >= tv.n_groups) return;
    const int lane = threadIdx.x & 63;
    const int l0 = b * LAG_LB;
    const int A = EARLY ? cut : LAG_A;
    const int C = tv.C, c_obs = tv.c_obs;
    const double* base = tv.tiles + tv.group_off[g] + lane;
    int ns = tv.lane_nsteps[g * WAVE + lane];
    if (EARLY) ns = min(ns, LAG_A);
    if (ns <= A) ns = 0;
    int nmax = ns;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, 64));
    double acc[LAG_LB];
#pragma unroll
    for (int j = 0; j < LAG_LB; j++) acc[j] = 0.0;
    // A group without a bulk (its longest track <= LAG_A rows) writes its zeros and leaves BEFORE any load: the tiles give a group
    // only its own (padded) length, and the last group -- the shortest tracks -- may be shorter than the rows below.
    if (nmax <= A || (EARLY && l0 >= A)) {
        if (lane < LAG_LB) Qg[(int64_t)g * LAG_N + l0 + lane] = 0.0;
        if (LEVELS && b == 0 && lane < 2) s0g[(int64_t)g * 2 + lane] = 0.0;
        return;
    }
    double zsum[2] = {0.0, 0.0};
    for (int a = 0; a < d; a++) {
        const double rf = LEVELS ? ref.v[a] : 0.0;
        const double* p = base + (int64_t)(c_obs + a) * WAVE;
        const int64_t rs = (int64_t)C * WAVE;
        double old[LAG_LB], nw[LAG_LB], cur[LAG_LB];
        // old[j] = Dy_{LAG_A - l0 - LAG_LB + j}: the lagged increments of the rows before the first block (row >= LAG_A - LAG_N - 1 >= 0)
        double yl = LEVELS ? rf : p[(EARLY ? max(A - l0 - LAG_LB - 1, 0) : A - l0 - LAG_LB - 1) * rs];
#pragma unroll
        for (int j = 0; j < LAG_LB; j++) {
            const double y = p[(EARLY ? max(A - l0 - LAG_LB + j, 0) : A - l0 - LAG_LB + j) * rs];
            old[j] = ns > 0 ? y - yl : 0.0;
            if (!LEVELS) yl = y;
        }
        double yc = LEVELS ? rf : p[(A - 1) * rs];
        for (int t0 = A; t0 < nmax; t0 += LAG_LB) {     // (loads reach row nmax + LAG_LB - 2 < group length + TILE_SPARE)
#pragma unroll
            for (int j = 0; j < LAG_LB; j++) {
                const double y = p[(t0 - l0 + j) * rs];
                nw[j] = (t0 - l0 + j < ns) ? y - yl : 0.0;
                if (!LEVELS) yl = y;
            }
#pragma unroll
            for (int j = 0; j < LAG_LB; j++) {
                const double y = p[(t0 + j) * rs];
                cur[j] = (t0 + j < ns) ? y - yc : 0.0;
                if (!LEVELS) yc = y;
            }
            if (LEVELS && b == 0) {
#pragma unroll
                for (int j = 0; j < LAG_LB; j++) zsum[a] += cur[j];
            }
            // row t0 + u, lag l0 + j: Dy_{t0 + u - l0 - j} = nw[u - j] (u >= j) or old[LAG_LB + u - j]
#pragma unroll
            for (int u = 0; u < LAG_LB; u++)
#pragma unroll
                for (int j = 0; j < LAG_LB; j++) acc[j] = fma(cur[u], u >= j ? nw[u - j] : old[LAG_LB + u - j], acc[j]);
#pragma unroll
            for (int j = 0; j < LAG_LB; j++) old[j] = nw[j];
        }
    }
#pragma unroll
    for (int j = 0; j < LAG_LB; j++) {
        const double t = wave_sum(acc[j]);
        if (lane == 0) Qg[(int64_t)g * LAG_N + l0 + j] = t;
    }
    if (LEVELS && b == 0) {
#pragma unroll
        for (int a = 0; a < 2; a++) {
            const double t = wave_sum(zsum[a]);
            if (lane == 0) s0g[(int64_t)g * 2 + a] = t;
        }
    }
}

__device__ __forceinline__ double readlane_d(double x, int k) {
    const long long v = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)v, k), hi = __builtin_amdgcn_readlane((int)(v >> 32), k);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// The end corrections D_pq = sum (h_p h_q - g_p g_q) of one group (h_j = Dy_{LAG_A-1-j}, g_j = Dy_{n-1-j}) for 64 rows p x 64
// columns q: one wave per (group, p block, q block), lane = p; the group's tracks one after the other (fixed order), column q's
// values broadcast from the lane that loaded them.  The q block 0 waves also sum s_{a,p} = y_{n-1-p} - y_{LAG_A-1-p}.
// LEVELS: h_j = z_{LAG_A-1-j}, g_j = z_{n-1-j} of the levels z = y - ref_a, and the q block 0 waves sum e_{a,p} = h_{a,p} - g_{a,p}, the
// steps of s_{a,p+1} = s_{a,p} + e_{a,p} (lag_levels_s, on the host).
// EARLY: h_j = Dy_{cut-1-j}, g_j = Dy_{n-1-j} with n = min(n, LAG_A), for p, q <= cut - 2 (s: p <= cut - 1); zeros elsewhere -- the rows
// those entries would read lie before row 0 and are clamped to it.
template <bool LEVELS, bool EARLY>
__global__ __launch_bounds__(WG_WAVES * WAVE) void lag_ends_kernel(const TileView tv, int d, double* Dg, double* sg, const LagRef ref, int cut) {
    static_assert(!(LEVELS && EARLY), "early cuts: the increments");
    constexpr int PB = LAG_N / 64;
    const int id = blockIdx.x * WG_WAVES + (threadIdx.x >> 6);
    const int g = id / (PB * PB), pb = (id / PB) % PB, qb = id % PB;
    if (g >= tv.n_groups) return;
    const int lane = threadIdx.x & 63;
    const int p = pb * 64 + lane, q = qb * 64 + lane;
    const int C = tv.C, c_obs = tv.c_obs;
    const int64_t rs = (int64_t)C * WAVE;
    double acc[64], sacc[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 64; k++) acc[k] = 0.0;
    if (EARLY) {
        const int A = cut;
        const bool vp = p <= A - 2, vq = q <= A - 2, vs = p <= A - 1;
        const bool any = pb * 64 <= A - 1 && qb * 64 <= A - 2;       // (wave-uniform)
        for (int m = 0; any && m < WAVE; m++) {
            const int n = min(tv.lane_nsteps[g * WAVE + m], LAG_A);
            if (n <= A) continue;
            const double* bm = tv.tiles + tv.group_off[g] + m;
            for (int a = 0; a < d; a++) {
                const double* y = bm + (int64_t)(c_obs + a) * WAVE;
                // rows 0 <= .. < n: cut - 2 - p >= 0 and n - 2 - p >= 0 where vp, the clamp elsewhere
                const double hp = vp ? y[max(A - 1 - p, 0) * rs] - y[max(A - 2 - p, 0) * rs] : 0.0;
                const double gp = vp ? y[(int64_t)max(n - 1 - p, 0) * rs] - y[(int64_t)max(n - 2 - p, 0) * rs] : 0.0;
                const double hq = vq ? y[max(A - 1 - q, 0) * rs] - y[max(A - 2 - q, 0) * rs] : 0.0;
                const double gq = vq ? y[(int64_t)max(n - 1 - q, 0) * rs] - y[(int64_t)max(n - 2 - q, 0) * rs] : 0.0;
#pragma unroll
                for (int k = 0; k < 64; k++) acc[k] = fma(hp, readlane_d(hq, k), fma(-gp, readlane_d(gq, k), acc[k]));
                if (qb == 0 && vs) sacc[a] += y[(int64_t)max(n - 1 - p, 0) * rs] - y[max(A - 1 - p, 0) * rs];
            }
        }
    } else
    for (int m = 0; m < WAVE; m++) {
        const int n = tv.lane_nsteps[g * WAVE + m];
        if (n <= LAG_A) continue;
        const double* bm = tv.tiles + tv.group_off[g] + m;
        for (int a = 0; a < d; a++) {
            const double* y = bm + (int64_t)(c_obs + a) * WAVE;
            // rows >= n - LAG_N - 1 >= LAG_A - LAG_N >= 0, all < n
            double hp, gp, hq, gq;
            if (LEVELS) {
                const double rf = ref.v[a];
                hp = y[(LAG_A - 1 - p) * rs] - rf;
                gp = y[(int64_t)(n - 1 - p) * rs] - rf;
                hq = y[(LAG_A - 1 - q) * rs] - rf;
                gq = y[(int64_t)(n - 1 - q) * rs] - rf;
            } else {
                hp = y[(LAG_A - 1 - p) * rs] - y[(LAG_A - 2 - p) * rs];
                gp = y[(int64_t)(n - 1 - p) * rs] - y[(int64_t)(n - 2 - p) * rs];
                hq = y[(LAG_A - 1 - q) * rs] - y[(LAG_A - 2 - q) * rs];
                gq = y[(int64_t)(n - 1 - q) * rs] - y[(int64_t)(n - 2 - q) * rs];
            }
#pragma unroll
            for (int k = 0; k < 64; k++) acc[k] = fma(hp, readlane_d(hq, k), fma(-gp, readlane_d(gq, k), acc[k]));
            if (qb == 0) sacc[a] += LEVELS ? hp - gp : y[(int64_t)(n - 1 - p) * rs] - y[(LAG_A - 1 - p) * rs];
        }
    }
    double* o = Dg + ((int64_t)g * LAG_N + p) * LAG_N + qb * 64;
#pragma unroll
    for (int k = 0; k < 64; k++) o[k] = acc[k];
    if (qb == 0)
        for (int a = 0; a < 2; a++) sg[((int64_t)g * 2 + a) * LAG_N + p] = a < d ? sacc[a] : 0.0;
}

// The Gram statistics of the head's rows (ssde_headforms.hpp): per (track, coordinate) the vector w = (x0 - y_0, v0, the increments of
// rows 1 .. HEAD_C - 1), HEAD_NW components; G_pq = sum w_p w_q of one group for 64 rows p x 64 columns q, in lag_ends_kernel's
// geometry and layout (LAG_N x LAG_N per group, zeros past HEAD_NW): one wave per (group, p block, q block), lane = p, the group's
// tracks and coordinates one after the other (fixed order), column q's values broadcast from the lane that loaded them.  The
// q block 0 waves also sum s_{a,p} = sum w_{a,p}.  A lane whose track has fewer than HEAD_C rows contributes nothing (the engine
// builds these statistics only where there is none: rows 0 .. HEAD_C - 1 of every track that is read lie inside it).
__global__ __launch_bounds__(WG_WAVES * WAVE) void head_gram_kernel(const TileView tv, int d, double* Dg, double* sg) {
    static_assert(HEAD_NW <= LAG_N, "the head's statistics fit the per-group temporaries of the lag statistics");
    constexpr int PB = LAG_N / 64;
    const int id = blockIdx.x * WG_WAVES + (threadIdx.x >> 6);
    const int g = id / (PB * PB), pb = (id / PB) % PB, qb = id % PB;
    if (g >= tv.n_groups) return;
    const int lane = threadIdx.x & 63;
    const int p = pb * 64 + lane, q = qb * 64 + lane;
    const int C = tv.C, c_obs = tv.c_obs, SD = 2 * d;
    const int64_t rs = (int64_t)C * WAVE;
    double acc[64], sacc[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 64; k++) acc[k] = 0.0;
    const bool any = pb * 64 < HEAD_NW && qb * 64 < HEAD_NW;          // (wave-uniform)
    for (int m = 0; any && m < WAVE; m++) {
        if (tv.lane_nsteps[g * WAVE + m] < HEAD_C) continue;
        const double* bm = tv.tiles + tv.group_off[g] + m;
        for (int a = 0; a < d; a++) {
            const double* y = bm + (int64_t)(c_obs + a) * WAVE;
            const double* a0 = tv.a0 + ((int64_t)g * SD + 2 * a) * WAVE + m;
            // component i of w: rows <= i - 1 <= HEAD_C - 1 of the track
            auto w = [&](int i) -> double {
                if (i >= HEAD_NW) return 0.0;
                if (i == 0) return a0[0] - y[0];
                if (i == 1) return a0[WAVE];
                return y[(int64_t)(i - 1) * rs] - y[(int64_t)(i - 2) * rs];
            };
            const double wp = w(p), wq = w(q);
#pragma unroll
            for (int k = 0; k < 64; k++) acc[k] = fma(wp, readlane_d(wq, k), acc[k]);
            if (qb == 0) sacc[a] += wp;
        }
    }
    double* o = Dg + ((int64_t)g * LAG_N + p) * LAG_N + qb * 64;
#pragma unroll
    for (int k = 0; k < 64; k++) o[k] = acc[k];
    if (qb == 0)
        for (int a = 0; a < 2; a++) sg[((int64_t)g * 2 + a) * LAG_N + p] = a < d ? sacc[a] : 0.0;
}

// dst[e] = sum over g (in order) of src[g * n + e]
__global__ __launch_bounds__(256) void lag_group_sum_kernel(const double* src, int64_t n, int G, double* dst) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int g = 0; g < G; g++) s += src[(int64_t)g * n + e];
    dst[e] = s;
}

}  // namespace

hipError_t launch_lagstats(const TileView& tv, int d, double* Qg, double* Dg, double* sg, double* Q, double* D, double* s, hipStream_t st,
                           const double* levels_ref, double* s0g, double* s0) {
    const int G = tv.n_groups;
    const dim3 grid_t((G * LAG_NB + WG_WAVES - 1) / WG_WAVES), block(WG_WAVES * WAVE);
    constexpr int PB = LAG_N / 64;
    const dim3 grid_e((G * PB * PB + WG_WAVES - 1) / WG_WAVES);
    if (levels_ref) {
        if (!s0g || !s0) return hipErrorInvalidValue;
        const LagRef ref = {{levels_ref[0], d > 1 ? levels_ref[1] : 0.0}};
        hipLaunchKernelGGL((lag_toeplitz_kernel<true, false>), grid_t, block, 0, st, tv, d, Qg, ref, s0g, LAG_A);
        hipLaunchKernelGGL((lag_ends_kernel<true, false>), grid_e, block, 0, st, tv, d, Dg, sg, ref, LAG_A);
    } else {
        const LagRef ref = {{0.0, 0.0}};
        hipLaunchKernelGGL((lag_toeplitz_kernel<false, false>), grid_t, block, 0, st, tv, d, Qg, ref, (double*)nullptr, LAG_A);
        hipLaunchKernelGGL((lag_ends_kernel<false, false>), grid_e, block, 0, st, tv, d, Dg, sg, ref, LAG_A);
    }
    auto sum = [&](const double* src, int64_t n, double* dst) {
        hipLaunchKernelGGL(lag_group_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, n, G, dst);
    };
    sum(Qg, LAG_N, Q);
    sum(Dg, (int64_t)LAG_N * LAG_N, D);
    sum(sg, 2 * LAG_N, s);
    if (levels_ref) sum(s0g, 2, s0);
    return hipGetLastError();
}

// The head rows' own contribution to the statistics of the early cut `cut` (ssde_lagstats.hpp): the same two passes over the tracks cut off
// after LAG_A rows, the same fixed-order sums over the groups.  Q, D, s hold the lags / entries below the cut; the others are
// not to be read (the host assembles from the former alone: lag_assemble_cut).
hipError_t launch_lagstats_cut(const TileView& tv, int d, int cut, double* Qg, double* Dg, double* sg, double* Q, double* D, double* s, hipStream_t st) {
    if (lag_cut_index(cut) < 0) return hipErrorInvalidValue;
    const int G = tv.n_groups;
    const dim3 grid_t((G * LAG_NB + WG_WAVES - 1) / WG_WAVES), block(WG_WAVES * WAVE);
    constexpr int PB = LAG_N / 64;
    const dim3 grid_e((G * PB * PB + WG_WAVES - 1) / WG_WAVES);
    const LagRef ref = {{0.0, 0.0}};
    hipLaunchKernelGGL((lag_toeplitz_kernel<false, true>), grid_t, block, 0, st, tv, d, Qg, ref, (double*)nullptr, cut);
    hipLaunchKernelGGL((lag_ends_kernel<false, true>), grid_e, block, 0, st, tv, d, Dg, sg, ref, cut);
    hipLaunchKernelGGL(lag_group_sum_kernel, dim3((unsigned)((LAG_N + 255) / 256)), dim3(256), 0, st, Qg, (int64_t)LAG_N, G, Q);
    hipLaunchKernelGGL(lag_group_sum_kernel, dim3((unsigned)(((int64_t)LAG_N * LAG_N + 255) / 256)), dim3(256), 0, st, Dg, (int64_t)LAG_N * LAG_N, G, D);
    hipLaunchKernelGGL(lag_group_sum_kernel, dim3((unsigned)((2 * LAG_N + 255) / 256)), dim3(256), 0, st, sg, (int64_t)2 * LAG_N, G, s);
    return hipGetLastError();
}

// The Gram statistics of the head's rows (ssde_headforms.hpp) in the lag statistics' per-group temporaries: Dg [G][LAG_N][LAG_N] and
// sg [G][2][LAG_N], summed over the groups in order into D [LAG_N][LAG_N] and s [2][LAG_N] (the leading HEAD_NW entries; zeros past them).
hipError_t launch_headstats(const TileView& tv, int d, double* Dg, double* sg, double* D, double* s, hipStream_t st) {
    const int G = tv.n_groups;
    constexpr int PB = LAG_N / 64;
    const dim3 grid_e((G * PB * PB + WG_WAVES - 1) / WG_WAVES), block(WG_WAVES * WAVE);
    hipLaunchKernelGGL(head_gram_kernel, grid_e, block, 0, st, tv, d, Dg, sg);
    hipLaunchKernelGGL(lag_group_sum_kernel, dim3((unsigned)(((int64_t)LAG_N * LAG_N + 255) / 256)), dim3(256), 0, st, Dg, (int64_t)LAG_N * LAG_N, G, D);
    hipLaunchKernelGGL(lag_group_sum_kernel, dim3((unsigned)((2 * LAG_N + 255) / 256)), dim3(256), 0, st, sg, (int64_t)2 * LAG_N, G, s);
    return hipGetLastError();
}

}  // namespace ssde
