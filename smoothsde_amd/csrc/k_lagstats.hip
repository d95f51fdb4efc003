// k_lagstats.hip -- the lag statistics of a stationary batch (ssde_create, once) and the bulk forms built from them (every
// evaluation that takes that path).  Derivation and layout: ssde_lagstats.hpp, DESIGN.md §3.3d.  Every sum runs in a fixed
// order: two creates of the same data give bitwise-equal statistics, two evaluations at the same theta bitwise-equal forms.
#include "ssde_device.hpp"
#include "ssde_lagstats.hpp"
#include "ssde_tf.hpp"

namespace ssde {

namespace {

constexpr int LAG_NB = LAG_N / LAG_LB;        // lag blocks of the Toeplitz pass

// Toeplitz lag sums Q_l = sum_{t = LAG_A}^{n - 1} Dy_t Dy_{t-l} (summed over the coordinates) of the 64 tracks of a group, for the
// LAG_LB lags of one block: one wave per (group, lag block), lane = track.  The rows walk in blocks of LAG_LB; the lagged
// increments of the block before stay in registers (old), so each row is loaded twice per work item: as the current row and
// as the lagged one.  A lane without a bulk (n <= LAG_A, or no track) contributes zeros; rows past a lane's track are zeroed
// before they are multiplied (the tile slots there hold whatever the layout put there).
__global__ __launch_bounds__(WG_WAVES * WAVE) void lag_toeplitz_kernel(const TileView tv, int d, double* Qg) {
    const int id = blockIdx.x * WG_WAVES + (threadIdx.x >> 6);
    const int g = id / LAG_NB, b = id % LAG_NB;
    if (g >= tv.n_groups) return;
    const int lane = threadIdx.x & 63;
    const int l0 = b * LAG_LB;
    const int C = tv.C, c_obs = tv.c_obs;
    const double* base = tv.tiles + tv.group_off[g] + lane;
    int ns = tv.lane_nsteps[g * WAVE + lane];
    if (ns <= LAG_A) ns = 0;
    int nmax = ns;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, 64));
    double acc[LAG_LB];
#pragma unroll
    for (int j = 0; j < LAG_LB; j++) acc[j] = 0.0;
    // A group without a bulk (its longest track <= LAG_A rows) writes its zeros and leaves BEFORE any load: the tiles give a group
    // only its own (padded) length, and the last group -- the shortest tracks -- may be shorter than the rows below.
    if (nmax <= LAG_A) {
        if (lane < LAG_LB) Qg[(int64_t)g * LAG_N + l0 + lane] = 0.0;
        return;
    }
    for (int a = 0; a < d; a++) {
        const double* p = base + (int64_t)(c_obs + a) * WAVE;
        const int64_t rs = (int64_t)C * WAVE;
        double old[LAG_LB], nw[LAG_LB], cur[LAG_LB];
        // old[j] = Dy_{LAG_A - l0 - LAG_LB + j}: the lagged increments of the rows before the first block (row >= LAG_A - LAG_N - 1 >= 0)
        double yl = p[(LAG_A - l0 - LAG_LB - 1) * rs];
#pragma unroll
        for (int j = 0; j < LAG_LB; j++) {
            const double y = p[(LAG_A - l0 - LAG_LB + j) * rs];
            old[j] = ns > 0 ? y - yl : 0.0;
            yl = y;
        }
        double yc = p[(LAG_A - 1) * rs];
        for (int t0 = LAG_A; t0 < nmax; t0 += LAG_LB) {     // (loads reach row nmax + LAG_LB - 2 < group length + TILE_SPARE)
#pragma unroll
            for (int j = 0; j < LAG_LB; j++) {
                const double y = p[(t0 - l0 + j) * rs];
                nw[j] = (t0 - l0 + j < ns) ? y - yl : 0.0;
                yl = y;
            }
#pragma unroll
            for (int j = 0; j < LAG_LB; j++) {
                const double y = p[(t0 + j) * rs];
                cur[j] = (t0 + j < ns) ? y - yc : 0.0;
                yc = y;
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
}

__device__ __forceinline__ double readlane_d(double x, int k) {
    const long long v = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)v, k), hi = __builtin_amdgcn_readlane((int)(v >> 32), k);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// The end corrections D_pq = sum (h_p h_q - g_p g_q) of one group (h_j = Dy_{LAG_A-1-j}, g_j = Dy_{n-1-j}) for 64 rows p x 64
// columns q: one wave per (group, p block, q block), lane = p; the group's tracks one after the other (fixed order), column q's
// values broadcast from the lane that loaded them.  The q block 0 waves also sum s_{a,p} = y_{n-1-p} - y_{LAG_A-1-p}.
__global__ __launch_bounds__(WG_WAVES * WAVE) void lag_ends_kernel(const TileView tv, int d, double* Dg, double* sg) {
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
    for (int m = 0; m < WAVE; m++) {
        const int n = tv.lane_nsteps[g * WAVE + m];
        if (n <= LAG_A) continue;
        const double* bm = tv.tiles + tv.group_off[g] + m;
        for (int a = 0; a < d; a++) {
            const double* y = bm + (int64_t)(c_obs + a) * WAVE;
            // rows >= n - LAG_N - 1 >= LAG_A - LAG_N >= 0, all < n
            const double hp = y[(LAG_A - 1 - p) * rs] - y[(LAG_A - 2 - p) * rs];
            const double gp = y[(int64_t)(n - 1 - p) * rs] - y[(int64_t)(n - 2 - p) * rs];
            const double hq = y[(LAG_A - 1 - q) * rs] - y[(LAG_A - 2 - q) * rs];
            const double gq = y[(int64_t)(n - 1 - q) * rs] - y[(int64_t)(n - 2 - q) * rs];
#pragma unroll
            for (int k = 0; k < 64; k++) acc[k] = fma(hp, readlane_d(hq, k), fma(-gp, readlane_d(gq, k), acc[k]));
            if (qb == 0) sacc[a] += y[(int64_t)(n - 1 - p) * rs] - y[(LAG_A - 1 - p) * rs];
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

// The bulk's forms at one theta: v = M lam (and the same for the check's shorter cut), then per tap row i its share of S, C_1..3
// and su_a (the mu dt terms through s and n), summed over the rows by a fixed tree and turned into the accumulators
// tf_finish forms (ssde_tf.hpp, as TfCtcrw::finish) -- written as window `chunk` of group 0 of the partial sums (every other group of that window: zero).
constexpr int LF_THREADS = 4 * LAG_N;
__global__ __launch_bounds__(LF_THREADS) void lag_forms_kernel(const LagFormArgs A) {
    __shared__ double sv[2][4][LAG_N];
    __shared__ double red[12][256];
    const int tid = threadIdx.x;
    {
        const int r = tid % LAG_N, qq = tid / LAG_N, k0 = qq * (LAG_N / 4);
        double v = 0.0, vc = 0.0;
        // (fully unrolled this loop measured 32 against 14 us per launch on the headline batch)
        for (int k = k0; k < k0 + LAG_N / 4; k++) {
            const double m = A.M[(int64_t)k * LAG_N + r];       // (symmetric: column r, coalesced)
            const double lk = k <= A.K ? A.lam[k] : 0.0;
            v = fma(m, lk, v);
            vc = fma(m, k <= A.Kc ? lk : 0.0, vc);
        }
        sv[0][qq][r] = v; sv[1][qq][r] = vc;
    }
    __syncthreads();
    if (tid < 256) {
        double x[2][6];
        for (int c = 0; c < 2; c++)
            for (int j = 0; j < 6; j++) x[c][j] = 0.0;
        const int i = tid;
        if (i < LAG_N) {
            for (int c = 0; c < 2; c++) {
                const int K = c ? A.Kc : A.K;
                const double V = (sv[c][0][i] + sv[c][1][i]) + (sv[c][2][i] + sv[c][3][i]);
                const double li = i <= K ? A.lam[i] : 0.0, Lam = A.sum_lam[c];
                double rho[3];
                for (int k = 0; k < 3; k++) rho[k] = (i >= k + 1 && i <= K) ? A.rr[i - k - 1] : 0.0;
                double S = li * V, Ck[3] = {rho[0] * V, rho[1] * V, rho[2] * V};
                for (int a = 0; a < A.d; a++) {
                    const double sa = A.s[a * LAG_N + i], cm = A.cm[a];
                    S -= 2.0 * Lam * cm * li * sa;
                    for (int k = 0; k < 3; k++) Ck[k] -= cm * (Lam * rho[k] * sa + A.sum_rho[c][k] * li * sa);
                    double su = li * sa;
                    if (i == 0) {
                        S += A.n * cm * cm * Lam * Lam;
                        for (int k = 0; k < 3; k++) Ck[k] += A.n * cm * cm * Lam * A.sum_rho[c][k];
                        su -= A.n * cm * Lam;
                    }
                    x[c][4 + a] = su;
                }
                x[c][0] = S; x[c][1] = Ck[0]; x[c][2] = Ck[1]; x[c][3] = Ck[2];
            }
        }
        for (int c = 0; c < 2; c++)
            for (int j = 0; j < 6; j++) red[c * 6 + j][tid] = x[c][j];
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o)
            for (int j = 0; j < 12; j++) red[j][tid] += red[j][tid + o];
        __syncthreads();
    }
    const int NACC = 4 + A.d, G = A.n_groups;
    auto at = [&](int g, int k) -> int64_t {
        return A.kfast ? ((int64_t)A.chunk * G + g) * NACC + k : ((int64_t)A.chunk * NACC + k) * G + g;
    };
    for (int e = tid; e < G * NACC; e += LF_THREADS) {
        const int g = e / NACC, k = e % NACC;
        if (g != 0) A.partials[at(g, k)] = 0.0;
    }
    if (tid == 0) {
        double out[NACC_MAX];
        const double su[2] = {red[4][0], red[5][0]};
        tf_finish(A.statc, A.d, A.mask, red[0][0], red[1][0], red[2][0], red[3][0], su, out);     // (what the streaming lanes finish with)
        for (int k = 0; k < NACC; k++) A.partials[at(0, k)] = out[k];
        // the check: every raw sum of the two cuts, relative to itself or to sqrt(S n) (the size of a sum of n products of u with a
        // unit-scale signal), whichever is larger
        const double floor_ = sqrt(fabs(red[0][0]) * A.n);
        double w = 0.0;
        for (int j = 0; j < 4 + A.d; j++) {
            const double a = red[j][0], b = red[6 + j][0];
            const double sc = fmax(fmax(fabs(a), fabs(b)), floor_);
            const double r = fabs(a - b) / sc;
            w = (r == r) ? fmax(w, r) : INFINITY;
        }
        if (!(w == w)) w = INFINITY;
        if (w > 0.0) atomicMax((unsigned long long*)A.chk, (unsigned long long)__double_as_longlong(w));
    }
}

}  // namespace

hipError_t launch_lagstats(const TileView& tv, int d, double* Qg, double* Dg, double* sg, double* Q, double* D, double* s, hipStream_t st) {
    const int G = tv.n_groups;
    hipLaunchKernelGGL(lag_toeplitz_kernel, dim3((G * LAG_NB + WG_WAVES - 1) / WG_WAVES), dim3(WG_WAVES * WAVE), 0, st, tv, d, Qg);
    constexpr int PB = LAG_N / 64;
    hipLaunchKernelGGL(lag_ends_kernel, dim3((G * PB * PB + WG_WAVES - 1) / WG_WAVES), dim3(WG_WAVES * WAVE), 0, st, tv, d, Dg, sg);
    auto sum = [&](const double* src, int64_t n, double* dst) {
        hipLaunchKernelGGL(lag_group_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, n, G, dst);
    };
    sum(Qg, LAG_N, Q);
    sum(Dg, (int64_t)LAG_N * LAG_N, D);
    sum(sg, 2 * LAG_N, s);
    return hipGetLastError();
}

hipError_t launch_lag_forms(const LagFormArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(lag_forms_kernel, dim3(1), dim3(LF_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace ssde
