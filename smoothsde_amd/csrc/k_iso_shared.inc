// k_iso_shared.hip -- shared-covariance kernels for gfx950: constant coefficients, regular time
// grid, track groups without missing rows (CTCRW, OU_SSM, BM_SSM).
//
// In that regime the covariance half of the Kalman filter (P, F, K and all their sensitivities;
// ssde_math.hpp ctcrw_cov_step / scal_cov_step) does not depend on the observations and is the
// same for every track, so ssde_engine.hip evaluates it ONCE per evaluation into a small gain
// table that becomes stationary after the filter's transient (tens of rows).  The lanes run the
// mean half only:
//   * rows inside the transient read their gains from the table (wave-uniform addresses),
//   * rows past it use the stationary gains held in scalar registers, with the update written as
//     the minimal FMA chain (~62 fp64 instructions per row for 2-D CTCRW with three
//     covariance directions, against ~245 for the general per-lane filter) and the quadratic
//     forms accumulated as plain sums that are scaled once at the end.
// Observations stream from the tiled HBM layout with coalesced 512-B wave loads, prefetched
// SHARED_U rows ahead into registers; the dt channel is never read (16 B/row actual traffic
// for 24 B/row of algorithmic input).  Time windows and their hand-over check work exactly as
// in k_iso.hip, except that only the mean state needs a warm-up (the gains are exact).
#include <hip/hip_ext.h>

#include <type_traits>

#include "ssde_device.hpp"
#include "ssde_tf.hpp"   // TfCtcrw, BasisScal: the stationary-only lanes (also the quiet rows of k_iso.hip)

namespace ssde {

// -DSSDE_HEAD_STAMPS (a measuring build of k_iso_shared_cut.hip; off by default -- the default code object has none of this): where a
// wave of the lag-path head spends its time.  stamp[0] the first row's data and gains have arrived, [1] end of the table rows, [2] end of
// the stationary rows ([3], after the barrier, is the kernel's).  wall_clock64: 100 MHz, as SSDE_WAVE_CLOCK's own two stamps.
#ifdef SSDE_HEAD_STAMPS
#define SSDE_STAMP_PARAM , long long* stamp = nullptr
#define SSDE_STAMP_ARG , stamp
#define SSDE_STAMP(k) do { if (stamp) stamp[k] = wall_clock64(); } while (0)
#else
#define SSDE_STAMP_PARAM
#define SSDE_STAMP_ARG
#define SSDE_STAMP(k) do { } while (0)
#endif

// C = channels per step of the tile, c_obs = channel of the first obs column (a dt channel, if present, is not read).
// nt (wave-uniform): non-temporal loads.  A batch that is streamed once per evaluation and is far larger than the 256 MB
// Infinity Cache wants them (the headline batch, 1.6 GB: 0.259 against 0.274 ms with ordinary loads); a batch that FITS that
// cache wants ordinary loads -- the cache then still holds it at the next evaluation (one rank's share of a strong-scaled
// batch, 205 MB: 0.053 -> 0.044 ms; profiles/r04_a_nt_vs_plain.txt).  The engine decides at create (IsoArgs.stream_nt).
template <int D, int U = SHARED_U>
__device__ __forceinline__ void load_obs_block(double (&dst)[U][D], const double* p, int C, int c_obs, bool nt) {
#ifdef SSDE_DIAG_NOSTREAM   // timing-only diagnostic build (results are wrong): every block re-reads one 8-KB window
#pragma unroll
    for (int u = 0; u < U; u++)
#pragma unroll
        for (int a = 0; a < D; a++) dst[u][a] = p[((u * C + c_obs + a) * WAVE) & 1023];
#else
    if (nt) {
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int a = 0; a < D; a++) dst[u][a] = __builtin_nontemporal_load(&p[(u * C + c_obs + a) * WAVE]);   // read once
    } else {
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int a = 0; a < D; a++) dst[u][a] = p[(u * C + c_obs + a) * WAVE];
    }
#endif
}

// ---- CTCRW -------------------------------------------------------------------------------------
template <int D, int MASK>
struct SharedCtcrw {
    static constexpr int SD = 2 * D;
    static constexpr int NSTATE = shared_nstate(2 * D, MASK, true);
    CtcrwMean<D, MASK> M;          // state + table-phase accumulators
    double acc2, sacc[NDIRP], macc[D];  // stationary-phase sums: u'u, u' tx_j, u_a mx_a
    // stationary constants (wave-uniform)
    double k1, k2, c1, t12, e, iF, hd[NDIRP], dk1[NDIRP], dk2[NDIRP], dt12, de, cb1, cb2;
    double cx[D], cv[D], bmu[D];
    CtcrwTrans tr;

    template <class Args>      // (IsoArgs, or the cut kernel's HeadArgs: the same field names)
    __device__ __forceinline__ void setup(const Args& A) {
        tr = A.ctr;
        const double* c = A.statc;   // static indices into the kernel argument block: scalar loads
        iF = c[0]; k1 = c[1]; k2 = c[2]; c1 = c[3]; t12 = c[4]; e = c[5]; dt12 = c[6]; de = c[7]; cb1 = c[8]; cb2 = c[9];
#pragma unroll
        for (int j = 0; j < NDIRP; j++) { hd[j] = c[10 + j]; dk1[j] = c[13 + j]; dk2[j] = c[16 + j]; }
#pragma unroll
        for (int a = 0; a < D; a++) {
            cx[a] = c[19 + a]; bmu[a] = c[23 + a];
            // fma(e, v, cv) has two scalar sources (one allowed per VALU op): keep cv in a VGPR for good
            // instead of re-materialising it every row
            double t = c[21 + a];
            asm volatile("v_mov_b64 %0, %1" : "=v"(cv[a]) : "s"(t));
        }
    }
    __device__ __forceinline__ void init(const double* a0) { M.init(a0); reset_acc(); }
    __device__ __forceinline__ void reset_acc() {
        M.reset_acc();
        acc2 = 0.0;
#pragma unroll
        for (int j = 0; j < NDIRP; j++) sacc[j] = 0.0;
#pragma unroll
        for (int a = 0; a < D; a++) macc[a] = 0.0;
    }
    // table phase: generic mean half with the row's gains
    __device__ __forceinline__ void step_table(const double* __restrict__ row, const double* mu, const double* y) {
        CtcrwGain G;
        G.iF = row[0]; G.k1 = row[1]; G.k2 = row[2]; G.bm = row[3];
#pragma unroll
        for (int j = 0; j < NDIRP; j++) { G.diF[j] = row[4 + j]; G.dk1[j] = row[7 + j]; G.dk2[j] = row[10 + j]; }
        ctcrw_mean_step<D, MASK>(M, tr, G, mu, y, G.iF != 0.0);
    }
    // stationary phase: same recursion (nllk_ctcrw.hpp:221, 238 and its derivatives) with
    // du = -tx folded in: tx' = (1-k1) tx + t12 tv + dk1 u [+ dt12 (v - B mu)], etc.
    __device__ __forceinline__ void step_stat(const double* y) {
#pragma unroll
        for (int a = 0; a < D; a++) {
            const double u = y[a] - M.x[a];
            acc2 = fma(u, u, acc2);
#pragma unroll
            for (int j = 0; j < NDIRP; j++) {
                if (!(MASK & dir_bit(j))) continue;
                const double tx = M.tx[j][a], tv = M.tv[j][a];
                sacc[j] = fma(u, tx, sacc[j]);
                double nx = dk1[j] * u, nv = dk2[j] * u;
                if (j == 1) {
                    const double w = M.v[a] - bmu[a];
                    nx = fma(dt12, w, nx);
                    nv = fma(de, w, nv);
                }
                M.tx[j][a] = fma(c1, tx, fma(t12, tv, nx));
                M.tv[j][a] = fma(e, tv, fma(-k2, tx, nv));
            }
            if (MASK & DIR_MU) {
                const double mx = M.mx[a], mv = M.mv[a];
                macc[a] = fma(u, mx, macc[a]);
                M.mx[a] = fma(c1, mx, fma(t12, mv, cb1));
                M.mv[a] = fma(e, mv, fma(-k2, mx, cb2));
            }
            const double x = M.x[a], v = M.v[a];
            M.x[a] = fma(k1, u, fma(t12, v, x)) + cx[a];
            M.v[a] = fma(k2, u, fma(e, v, cv[a]));
        }
    }
    __device__ __forceinline__ void finish(double* out) const {
        const double z[NDIRP] = {0.0, 0.0, 0.0};
        ctcrw_finish_parts<D, MASK>(0.0, z, M, out);
        out[0] += 0.5 * iF * acc2;
        if (MASK & DIR_SIG) out[1] += hd[0] * acc2 - iF * sacc[0];
        if (MASK & DIR_MU) {
#pragma unroll
            for (int a = 0; a < D; a++) out[2 + a] -= iF * macc[a];
        }
        if (MASK & DIR_P1) out[2 + D] += hd[1] * acc2 - iF * sacc[1];
        if (MASK & DIR_P2) out[3 + D] += hd[2] * acc2 - iF * sacc[2];
    }
    // compact hand-over layout of the shared-covariance kernels: state, wanted directions, mu
    __device__ __forceinline__ void dump(double* o) const {
        int k = 0;
#pragma unroll
        for (int a = 0; a < D; a++) { o[k++] = M.x[a]; o[k++] = M.v[a]; }
#pragma unroll
        for (int j = 0; j < NDIRP; j++) {
            if (!(MASK & dir_bit(j))) continue;
#pragma unroll
            for (int a = 0; a < D; a++) { o[k++] = M.tx[j][a]; o[k++] = M.tv[j][a]; }
        }
        if (MASK & DIR_MU) {
#pragma unroll
            for (int a = 0; a < D; a++) { o[k++] = M.mx[a]; o[k++] = M.mv[a]; }
        }
    }
    __device__ static __forceinline__ void warm_a0(const double* y, double* a0) {
#pragma unroll
        for (int a = 0; a < D; a++) { a0[2 * a] = (y[a] == y[a]) ? y[a] : 0.0; a0[2 * a + 1] = 0.0; }
    }
};

// ---- OU_SSM / BM_SSM ---------------------------------------------------------------------------
template <int MODEL, int D, int MASK>
struct SharedScal {
    static constexpr int SD = D;
    static constexpr bool HAS_P2 = (MODEL == M_OU_SSM);
    static constexpr int NSTATE = shared_nstate(D, MASK, HAS_P2);
    ScalMean<D, MASK> M;
    double acc2, sacc[NDIRP], macc[D];
    double k, c, t, b, iF, hd[NDIRP], dk[NDIRP], dt_, cmu[D], dbmu[D];
    ScalTrans tr;

    __device__ __forceinline__ void setup(const IsoArgs& A) {
        tr = A.str;
        const double* cc = A.statc;
        iF = cc[0]; k = cc[1]; c = cc[2]; t = cc[3]; b = cc[4]; dt_ = cc[5];
#pragma unroll
        for (int j = 0; j < NDIRP; j++) { hd[j] = cc[10 + j]; dk[j] = cc[13 + j]; }
#pragma unroll
        for (int a = 0; a < D; a++) { cmu[a] = cc[19 + a]; dbmu[a] = cc[21 + a]; }
    }
    __device__ __forceinline__ void init(const double* a0) { M.init(a0); reset_acc(); }
    __device__ __forceinline__ void reset_acc() {
        M.reset_acc();
        acc2 = 0.0;
#pragma unroll
        for (int j = 0; j < NDIRP; j++) sacc[j] = 0.0;
#pragma unroll
        for (int a = 0; a < D; a++) macc[a] = 0.0;
    }
    __device__ __forceinline__ void step_table(const double* __restrict__ row, const double* mu, const double* y) {
        ScalGain G;
        G.iF = row[0]; G.k = row[1]; G.c = row[2];
#pragma unroll
        for (int j = 0; j < NDIRP; j++) { G.diF[j] = row[4 + j]; G.dk[j] = row[7 + j]; }
        scal_mean_step<D, MASK, HAS_P2>(M, tr, G, mu, y, G.iF != 0.0);
    }
    // x' = t x + k u + b mu;  tx' = (t - k) tx + dk u [+ dt_ x + db mu]   (nllk_ou_ssm.hpp:204, nllk_bm_ssm.hpp:166)
    __device__ __forceinline__ void step_stat(const double* y) {
#pragma unroll
        for (int a = 0; a < D; a++) {
            const double x = M.x[a];
            const double u = y[a] - x;
            acc2 = fma(u, u, acc2);
#pragma unroll
            for (int j = 0; j < NDIRP; j++) {
                if (!(MASK & dir_bit(j)) || (j == 2 && !HAS_P2)) continue;
                const double tx = M.tx[j][a];
                sacc[j] = fma(u, tx, sacc[j]);
                double nx = dk[j] * u;
                if (j == 1) nx = fma(dt_, x, nx) + dbmu[a];
                M.tx[j][a] = fma(c, tx, nx);
            }
            if (MASK & DIR_MU) {
                const double mx = M.mx[a];
                macc[a] = fma(u, mx, macc[a]);
                M.mx[a] = fma(c, mx, b);
            }
            M.x[a] = fma(k, u, fma(t, x, cmu[a]));
        }
    }
    __device__ __forceinline__ void finish(double* out) const {
        const double z[NDIRP] = {0.0, 0.0, 0.0};
        scal_finish_parts<D, MASK>(0.0, z, M, out);
        out[0] += 0.5 * iF * acc2;
        if (MASK & DIR_SIG) out[1] += hd[0] * acc2 - iF * sacc[0];
        if (MASK & DIR_MU) {
#pragma unroll
            for (int a = 0; a < D; a++) out[2 + a] -= iF * macc[a];
        }
        if (MASK & DIR_P1) out[2 + D] += hd[1] * acc2 - iF * sacc[1];
        if (HAS_P2 && (MASK & DIR_P2)) out[3 + D] += hd[2] * acc2 - iF * sacc[2];
    }
    __device__ __forceinline__ void dump(double* o) const {
        int kk = 0;
#pragma unroll
        for (int a = 0; a < D; a++) o[kk++] = M.x[a];
#pragma unroll
        for (int j = 0; j < NDIRP; j++) {
            if (!(MASK & dir_bit(j)) || (j == 2 && !HAS_P2)) continue;
#pragma unroll
            for (int a = 0; a < D; a++) o[kk++] = M.tx[j][a];
        }
        if (MASK & DIR_MU) {
#pragma unroll
            for (int a = 0; a < D; a++) o[kk++] = M.mx[a];
        }
    }
    __device__ static __forceinline__ void warm_a0(const double* y, double* a0) {
#pragma unroll
        for (int a = 0; a < D; a++) a0[a] = (y[a] == y[a]) ? y[a] : 0.0;
    }
};


// direction form for windows that touch the transient, basis form for the stationary-only kernel
template <int MODEL, int D, int MASK, bool STATONLY>
struct SharedSel { typedef SharedScal<MODEL, D, MASK> type; };
template <int D, int MASK>
struct SharedSel<M_CTCRW, D, MASK, false> { typedef SharedCtcrw<D, MASK> type; };
template <int MODEL, int D, int MASK>
struct SharedSel<MODEL, D, MASK, true> { typedef BasisScal<MODEL, D, MASK> type; };
template <int D, int MASK>
struct SharedSel<M_CTCRW, D, MASK, true> { typedef TfCtcrw<D, MASK> type; };

// The gain table in the table phase.  Its rows used to be fetched row by row with wave-uniform vector loads (13 per row,
// an L2 round trip each, competing with the observation prefetch for the 63 outstanding-load slots): 600 cycles per row
// for a ~70-instruction step, and the transient window (~100 such rows, one wave per track group) was a fixed ~30 us in
// EVERY evaluation of this path -- most of C2's 50 us kernel.  Now every wave stages GAIN_SLAB_ROWS rows at a time into
// its own LDS slab with coalesced loads (one round trip per slab) and the steps read them as LDS broadcasts.
constexpr int GAIN_SLAB_ROWS = 64;      // multiple of 2 * SHARED_U
static_assert(GAIN_SLAB_ROWS % (2 * SHARED_U) == 0, "gain slab");

// (iso_shared_cut_kernel reads a COPY of its argument block, k_iso_shared_cut.hip: a pointer out of the copy is a number to the compiler: said to point to global memory, as a kernel's pointer argument does, or every
//  load through it would be a flat one)
template <class T>
__device__ __forceinline__ T* head_global(T* p) { return (T*)(__attribute__((address_space(1))) T*)(unsigned long long)p; }      // (through the integer: a cast pair alone is folded away)
__device__ __forceinline__ const double* gain_table_ptr(const IsoArgs& A) { return A.gain; }
__device__ __forceinline__ const double* gain_table_ptr(const HeadArgs& A) { return head_global(A.gain); }
template <class Args>
__device__ __forceinline__ void stage_gain(const Args& A, double* slab, int row0) {
    const int lane = threadIdx.x & 63, glast = A.gain_last;
    const double* __restrict__ gain = gain_table_ptr(A);
#pragma unroll 4
    for (int r = 0; r < GAIN_SLAB_ROWS; r += WAVE / GAIN_ROW) {          // 4 rows of 16 doubles per wave load
        const int rr = r + lane / GAIN_ROW;
        slab[rr * GAIN_ROW + (lane % GAIN_ROW)] = gain[(int64_t)min(row0 + rr, glast) * GAIN_ROW + (lane % GAIN_ROW)];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The same slab from a table that came BY VALUE in the launch's argument block (HeadGain, ssde_gain_feed.hpp; iso_shared_wg_kernel): no
// copy precedes the launch and no pointer is chased -- the lanes read the packed rows straight from the block, same lane -> slab
// element map as above, rows past the last repeat it, the columns no model writes are zero.
// (rows: HeadGain.rows, which the cut kernel has in its hot block -- head_gain_rows.  In two halves: the cut kernel issues the first
//  slab's loads with its first round of loads and stores when the rows begin.)
constexpr int GAIN_SLAB_NL = GAIN_SLAB_ROWS / (WAVE / GAIN_ROW);      // loads per lane and slab
__device__ __forceinline__ void gain_value_loads(const HeadGain& G, int rows, int row0, double (&t)[GAIN_SLAB_NL]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < GAIN_SLAB_NL; i++) t[i] = head_gain_slab_at(G.v, rows, row0 + i * (WAVE / GAIN_ROW) + lane / GAIN_ROW, lane % GAIN_ROW);
}
__device__ __forceinline__ void gain_value_stores(const double (&t)[GAIN_SLAB_NL], double* slab) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < GAIN_SLAB_NL; i++) slab[(i * (WAVE / GAIN_ROW) + lane / GAIN_ROW) * GAIN_ROW + (lane % GAIN_ROW)] = t[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void stage_gain_value(const HeadGain& G, int rows, double* slab, int row0) {
    // every load of the slab is issued before the first store waits for one: one round trip to the block
    double t[GAIN_SLAB_NL];
    gain_value_loads(G, rows, row0, t);
    gain_value_stores(t, slab);
}

// rows [s0, s0 + SHARED_U) from a register block; `grow` = the slab row of s0 (table phase)
template <bool STAT, int D, class Lane, class Args>
__device__ __forceinline__ void run_block(Lane& S, const Args& A, const double (&blk)[SHARED_U][D], int s0, int ns,
                                          int ns_min, const double* mu, const double* grow) {
    if (s0 + SHARED_U <= ns_min) {
        // every lane's track covers the whole block: no per-row predication
#pragma unroll
        for (int u = 0; u < SHARED_U; u++) {
            if (STAT) S.step_stat(blk[u]);
            else S.step_table(grow + u * GAIN_ROW, mu, blk[u]);
        }
    } else {
#pragma unroll
        for (int u = 0; u < SHARED_U; u++) {
            if (s0 + u < ns) {
                if (STAT) S.step_stat(blk[u]);
                else S.step_table(grow + u * GAIN_ROW, mu, blk[u]);
            }
        }
    }
}

// rows [sa, sb) of the lane's window; STAT = stationary gains.  sa is a multiple of SHARED_U.
// Two register blocks in ping-pong: while one is consumed the other is in flight (no copies).
// WG: the waves of the workgroup run the windows of ONE group (iso_shared_wg_kernel) -- only wave 0 walks table rows: one gain slab.
// PRE (iso_shared_cut_kernel): the caller issued the loads of the segment's first TWO blocks and of its first gain slab (by value) with
// its own first round of loads; `pre` holds them.
template <int D>
struct HeadPre {
    double a[SHARED_U][D], b[SHARED_U][D];
    double gt[GAIN_SLAB_NL];         // (gain_rows > 0 only)
};
__device__ __forceinline__ int head_gain_rows(const IsoArgs&, const HeadGain& G) { return G.rows; }
__device__ __forceinline__ int head_gain_rows(const HeadArgs& A, const HeadGain&) { return A.gain_rows; }
template <bool STAT, int D, bool DEEP, bool WG, class Lane, class Args, bool PRE = false>
__device__ __forceinline__ void run_segment(Lane& S, const Args& A, const double* base, int sa, int sb, int ns,
                                            int ns_min, const double* mu, const HeadGain* G = nullptr, const HeadPre<D>* pre = nullptr SSDE_STAMP_PARAM) {
    const int C = A.tv.C, c_obs = A.tv.c_obs;
    const bool nt = A.stream_nt != 0;
    if (sa >= sb) return;
    double bufA[SHARED_U][D], bufB[SHARED_U][D];
#ifdef SSDE_DIAG_NOSTREAM
#define SSDE_ROWPTR(s) (base)
#else
#define SSDE_ROWPTR(s) (base + (int64_t)(s) * C * WAVE)
#endif
    __shared__ double gain_slab[(STAT || WG) ? 1 : WG_WAVES][STAT ? 1 : GAIN_SLAB_ROWS * GAIN_ROW];
    double* slab = gain_slab[(STAT || WG) ? 0 : (threadIdx.x >> 6)];
    if constexpr (DEEP && STAT) {
        // THREE register blocks in rotation keep TWO blocks (16 rows) in flight: one response column is 8 B per lane and row,
        // a block in flight is half the bytes of the two-column case, and the stream sat at 4.7 TB/s against 5.7-6.2.  With two
        // columns the deeper rotation was measured twice and changes nothing -- on the headline batch (0.280-0.285 against
        // 0.256-0.274 ms, round 2) and on one rank's share of a strong-scaled batch (1250 tracks x 10^4 rows, round 3: 0.0592
        // against 0.0597 ms): there the wave is not waiting for memory but for its own dependent instructions (SQ counters,
        // profiles/r03_*_pmc_share8.txt: 47 % of the wave cycles issue-stalled, 19 % on s_waitcnt, 29 % issuing VALU).
        static_assert(5 * SHARED_U <= TILE_SPARE, "look-ahead of the three-block rotation");
        double bufC[SHARED_U][D];
        load_obs_block<D>(bufA, SSDE_ROWPTR(sa), C, c_obs, nt);
        load_obs_block<D>(bufB, SSDE_ROWPTR(sa + SHARED_U), C, c_obs, nt);
        for (int s0 = sa; s0 < sb; s0 += 3 * SHARED_U) {       // TILE_SPARE (64 rows) covers the 5 blocks of look-ahead
            load_obs_block<D>(bufC, SSDE_ROWPTR(s0 + 2 * SHARED_U), C, c_obs, nt);
            run_block<STAT, D>(S, A, bufA, s0, ns, ns_min, mu, slab);
            load_obs_block<D>(bufA, SSDE_ROWPTR(s0 + 3 * SHARED_U), C, c_obs, nt);
            if (s0 + SHARED_U < sb) run_block<STAT, D>(S, A, bufB, s0 + SHARED_U, ns, ns_min, mu, slab);
            load_obs_block<D>(bufB, SSDE_ROWPTR(s0 + 4 * SHARED_U), C, c_obs, nt);
            if (s0 + 2 * SHARED_U < sb) run_block<STAT, D>(S, A, bufC, s0 + 2 * SHARED_U, ns, ns_min, mu, slab);
        }
        return;
    }
    if constexpr (PRE) {
#pragma unroll
        for (int u = 0; u < SHARED_U; u++)
#pragma unroll
            for (int a = 0; a < D; a++) { bufA[u][a] = pre->a[u][a]; bufB[u][a] = pre->b[u][a]; }
    } else load_obs_block<D>(bufA, SSDE_ROWPTR(sa), C, c_obs, nt);
    for (int s0 = sa; s0 < sb; s0 += 2 * SHARED_U) {
        // TILE_SPARE (>= 3 blocks) keeps the look-ahead loads inside the allocation
        if (!(PRE && s0 == sa)) load_obs_block<D>(bufB, SSDE_ROWPTR(s0 + SHARED_U), C, c_obs, nt);
        const int srow = (s0 - sa) % GAIN_SLAB_ROWS;
        if (!STAT && srow == 0) {
            const int grows = WG ? head_gain_rows(A, *G) : 0;
            if (PRE && s0 == sa && grows > 0) gain_value_stores(pre->gt, slab);
            else if (WG && grows > 0) stage_gain_value(*G, grows, slab, s0);
            else stage_gain(A, slab, s0);
            if (s0 == 0) SSDE_STAMP(0);
        }
        run_block<STAT, D>(S, A, bufA, s0, ns, ns_min, mu, slab + srow * GAIN_ROW);
        load_obs_block<D>(bufA, SSDE_ROWPTR(s0 + 2 * SHARED_U), C, c_obs, nt);
        if (s0 + SHARED_U < sb) run_block<STAT, D>(S, A, bufB, s0 + SHARED_U, ns, ns_min, mu, slab + (srow + SHARED_U) * GAIN_ROW);
    }
}

// STATONLY: the whole window (warm-up included) lies past the covariance transient -- the lean
// kernel; otherwise the window touches the transient and also carries the table-phase code.
// WG (iso_shared_wg_kernel): nothing of the window goes to global memory -- the record after its warm-up to rec_in (LDS, this lane's
// column: component k at rec_in[k * WAVE]), the record at its end to rec_end and the lane's accumulators to acc_out (registers).
template <int MODEL, int D, int MASK, bool STATONLY, bool DEEP, bool WG = false>
__device__ __forceinline__ int run_lane_shared(const IsoArgs& A, int g, int part, int chunk, double* rec_in = nullptr,
                                               double* rec_end = nullptr, double* acc_out = nullptr, const HeadGain* G = nullptr) {
    typedef typename SharedSel<MODEL, D, MASK, STATONLY>::type Lane;
    constexpr int NACC = 4 + D;
    constexpr int SD = Lane::SD;
    const int lane = threadIdx.x & 63;
    const TileView& tv = A.tv;
    const int C = tv.C, c_obs = tv.c_obs;
    const double* base = tv.tiles + tv.group_off[g] + lane;
    const int L = tv.group_len[g];
    const int ns = tv.lane_nsteps[g * WAVE + lane];
    // Rows every lane's track covers run without per-row predication.  A lane WITHOUT a track (the batch's last group is
    // rarely full) does not count: it walks the rows like its neighbours, on whatever its tile slots hold, and its sums are
    // dropped at the end -- a single empty lane used to put the whole wave on the predicated path for every row (one rank's
    // share of a strong-scaled batch: the launch waited 6 us for that one group, profiles/r04_a_wave_clock_share8.txt).
    int ns_min = ns > 0 ? ns : INT32_MAX;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ns_min = min(ns_min, __shfl_xor(ns_min, o, 64));
    ns_min = __builtin_amdgcn_readfirstlane(ns_min);
    const int pc = part * A.n_chunks + chunk;

    int s_begin, s_acc, s_end;
    window_bounds(L, A.n_chunks, A.window, A.t0, chunk, s_begin, s_acc, s_end, A.t0_delta);
    // first row from which the stationary gains apply (gain_stat[0] == 0 would mean "never scored":
    // that degenerate case stays on the table path)
    int s_stat = (A.gain_last + SHARED_U - 1) / SHARED_U * SHARED_U;
    if (A.gain_stat[0] == 0.0) s_stat = INT32_MAX;

    Lane S;
    S.setup(A);
    double mu[D];
#pragma unroll
    for (int a = 0; a < D; a++) mu[a] = A.mu[a];
    {
        double a0[SD];
        if (STATONLY && MODEL == M_CTCRW) {
            // transfer-function lanes start from the observation of the row before the window (s_begin > 0:
            // stationary-only windows lie past the covariance transient)
#pragma unroll
            for (int a = 0; a < D; a++) a0[a] = base[((int64_t)(s_begin - 1) * C + c_obs + a) * WAVE];
        } else if (s_begin == 0) {
#pragma unroll
            for (int c = 0; c < SD; c++) a0[c] = tv.a0[((int64_t)g * SD + c) * WAVE + lane];
        } else {
            double y0[D];
#pragma unroll
            for (int a = 0; a < D; a++) y0[a] = base[((int64_t)s_begin * C + c_obs + a) * WAVE];
            Lane::warm_a0(y0, a0);
        }
        S.init(a0);
    }
    // warm-up rows [s_begin, s_acc), then scored rows [s_acc, s_end); each split at s_stat
    {
        const int m = STATONLY ? s_begin : min(max(s_stat, s_begin), s_acc);
        if (!STATONLY) run_segment<false, D, DEEP, WG>(S, A, base, s_begin, m, ns, ns_min, mu, G);
        run_segment<true, D, DEEP, WG>(S, A, base, m, s_acc, ns, ns_min, mu);
    }
    if (s_acc > s_begin) {
        double st[Lane::NSTATE];
        S.dump(st);
        double* o = WG ? rec_in : A.bnd + (((int64_t)pc * tv.n_groups + g) * 2 + 0) * A.bnd_stride * WAVE + lane;
#pragma unroll
        for (int k = 0; k < Lane::NSTATE; k++) { if (!WG && A.fused) dev_store(o + k * WAVE, st[k]); else o[k * WAVE] = st[k]; }      // (fused: device scope -- another wave of this launch reads it)
        S.reset_acc();
    }
    {
        const int m = STATONLY ? s_acc : min(max(s_stat, s_acc), s_end);
        if (!STATONLY) run_segment<false, D, DEEP, WG>(S, A, base, s_acc, m, ns, ns_min, mu, G);
        run_segment<true, D, DEEP, WG>(S, A, base, m, s_end, ns, ns_min, mu);
    }
    if (WG) {
        if (chunk + 1 < A.n_chunks) S.dump(rec_end);
    } else
    if (A.n_chunks > 1 && chunk + 1 < A.n_chunks) {
        double st[Lane::NSTATE];
        S.dump(st);
        double* o = A.bnd + (((int64_t)pc * tv.n_groups + g) * 2 + 1) * A.bnd_stride * WAVE + lane;
#pragma unroll
        for (int k = 0; k < Lane::NSTATE; k++) { if (A.fused) dev_store(o + k * WAVE, st[k]); else o[k * WAVE] = st[k]; }
    }
    double out[NACC];
    S.finish(out);
    if (s_acc >= s_end || ns == 0) {
#pragma unroll
        for (int k = 0; k < NACC; k++) out[k] = 0.0;
    }
    if (WG) {
#pragma unroll
        for (int k = 0; k < NACC; k++) acc_out[k] = out[k];
        return s_end - s_begin;
    }
#pragma unroll
    for (int k = 0; k < NACC; k++) {
        const double t = wave_sum(out[k]);
        if (lane == 0) {
            if (A.fused) dev_store(&A.partials[((int64_t)pc * tv.n_groups + g) * NACC + k], t);      // ([window][group][accumulator])
            else A.partials[((int64_t)pc * NACC + k) * tv.n_groups + g] = t;
        }
    }
    return s_end - s_begin;       // rows this work item walked (SSDE_WAVE_CLOCK)
}

// (Two stationary-only windows per wave in one instruction stream -- twice the independent chains, twice the loads in flight -- were
//  built and measured in round 4 and are NOT here: the pair's rows cost exactly what two single rows cost (0.1315 against 0.1267 us
//  per row and wave), because a lone wave is not waiting for its own instructions -- the row's arithmetic takes 100 cycles, 3.9 per
//  instruction -- but for memory: with one wave per SIMD the chip delivers 6.3-6.7 TB/s to this access pattern whatever the bytes in
//  flight per wave (8-40 KB) and whether the buffer is 200 MB or 1.6 GB.  tools/microbench_issue.hip, profiles/r04_a_issue_microbench.txt.)

// One kernel per (model, dimension, direction mask): the register allocation of a kernel is the worst
// case over everything it contains, so the masks are NOT folded into one kernel with a switch here.
// With a dedicated transient window (t0 > 0) the grid enumerates windows 1..n_chunks-1; the wave that
// owns window 1 first runs window 0 (direction form, gain table), every window >= 1 runs the lean
// basis-form code.  Without it (short tracks, a single window) every wave runs the general shared code.
// A transient window with nothing taken off window 1 (t0 > 0, t0_delta == 0: the latency plan of the lag-statistics head,
// ssde_windows.hpp) has a wave of its own: the grid enumerates every window, wave 0 of a group runs window 0 and nothing else.
// the work of one wave; returns the rows it walked (SSDE_WAVE_CLOCK)
// g, c_lo .. c_hi: the group and the windows the wave ran (the fused finalising work announces them)
template <int MODEL, int D, int MASK, bool DEEP>
__device__ __forceinline__ int shared_wave(const IsoArgs& A, bool& valid, int& g, int& c_lo, int& c_hi) {
    int part, chunk, rows = 0;
    valid = false;
    if (A.t0 > 0) {
        const bool own = A.t0_delta == 0;
        if (!decode_block(A, own ? A.n_chunks : A.n_chunks - 1, g, part, chunk)) return 0;
        if (!group_selected(A, g)) return 0;
        valid = true;
        if (!own) chunk += 1;
        c_lo = c_hi = chunk;
        if (chunk == (own ? 0 : 1)) { rows += run_lane_shared<MODEL, D, MASK, false, DEEP>(A, g, part, 0); c_lo = 0; }
        if (chunk > 0) rows += run_lane_shared<MODEL, D, MASK, true, DEEP>(A, g, part, chunk);
    } else {
        if (!decode_block(A, A.n_chunks, g, part, chunk)) return 0;
        if (!group_selected(A, g)) return 0;
        valid = true;
        c_lo = c_hi = chunk;
        rows += run_lane_shared<MODEL, D, MASK, false, DEEP>(A, g, part, chunk);
    }
    return rows;
}

template <int MODEL, int D, int MASK, bool DEEP>
__global__ __launch_bounds__(WG_WAVES * WAVE, 1) void iso_shared_kernel(const IsoArgs A, const ReduceArgs R) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && A.chk_out && !A.fused) *A.chk_out = 0.0;   // raised by the finalize launch (fused: zeroed by the engine, on the stream)
    const long long wc0 = A.wave_clock ? wall_clock64() : 0;
    int g = -1, c_lo = 0, c_hi = 0;
    bool valid = false;
    const int rows = shared_wave<MODEL, D, MASK, DEEP>(A, valid, g, c_lo, c_hi);
    // (the finalising work, in the launch: hand-over checks by the second wave at a boundary, sums and publication by the last wave)
    if (A.fused && valid) fused_finalize_wave<4 + D>(A, R, A.nstate_clean, g, c_lo, c_hi);
    // (debugging: when did this wave run, where, over how many rows -- SSDE_WAVE_CLOCK)
    if (A.wave_clock && !(threadIdx.x & 63) && rows > 0) {
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        double* o = A.wave_clock + 4 * (int64_t)(blockIdx.x * WG_WAVES + (threadIdx.x >> 6));
        o[0] = (double)wc0; o[1] = (double)wall_clock64(); o[2] = (double)hw; o[3] = 1.0 + rows;
    }
}


// ---- one workgroup per track group -----------------------------------------------------------------------------------------------------
// The latency plan of the lag-statistics head with n_chunks == WG_WAVES (ssde_windows.hpp: head_latency_plan): the windows of a group
// are the waves of ONE workgroup, one per SIMD of its CU -- wave 0 the transient window and nothing else, wave w >= 1 the lean
// stationary-only code on window w.  Workgroup b owns group b (the groups padded to eight, as decode_block pads them; the padding
// workgroups leave whole).  What the two sides of a window boundary have to say to each other never leaves the CU: window w's record
// after its warm-up goes to LDS, the record at a window's end stays in registers, and after ONE barrier wave c compares its end with
// window c + 1's record -- the arithmetic of window_check_wave (per component the largest |a - b| and max(|a|, |b|) over the lanes,
// the worst ratio, not-a-number -> infinity, lanes whose track ends before the boundary masked): order-free maxima, so the value is
// bitwise what iso_finalize_kernel's check workgroups and fused_finalize_wave find.  Every wave leaves its 4 + D wave sums and its
// check in LDS; after a second barrier wave 0 owns the group's record and sends it out with ONE store instruction: to the host's
// mailbox (A.mbx: system-scope stores, a wait for them -- no fence, as publish_if_last --, then the evaluation's sequence word, which
// the host spins on: ssde_reduce_host.hpp forms the result) or to partials / chk[g] for a finalize launch without check workgroups.
template <int MODEL, int D, int MASK, bool DEEP>
__global__ __launch_bounds__(WG_WAVES * WAVE, 1) void iso_shared_wg_kernel(const IsoArgs A, const HeadGain GV) {
    typedef typename SharedSel<MODEL, D, MASK, false>::type Lane0;
    typedef typename SharedSel<MODEL, D, MASK, true>::type LaneS;
    constexpr int NACC = 4 + D, NST = Lane0::NSTATE;
    static_assert(NST == LaneS::NSTATE, "both lane forms dump the direction-form record");
    static_assert(WG_WAVES * NACC <= MBX_CHK && WG_WAVES * NACC < WAVE, "a group's record is one store of wave 0");
    __shared__ double rec[WG_WAVES - 1][NST][WAVE];           // [c]: window c + 1's record after its warm-up
    __shared__ double wsum[WG_WAVES][NACC + 1];               // a wave's sums | its boundary's check
    static_assert(sizeof(double) * ((WG_WAVES - 1) * NST * WAVE + WG_WAVES * (NACC + 1) + GAIN_SLAB_ROWS * GAIN_ROW) <= 64 * 1024,
                  "static LDS of a workgroup: the hand-over records, the sums and wave 0's gain slab");
    if (blockIdx.x == 0 && threadIdx.x == 0 && A.chk_out && !A.mbx) *A.chk_out = 0.0;       // raised by the finalize launch
    const int g = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (g >= A.tv.n_groups) return;                            // (the whole workgroup: nobody is left at a barrier)
    const long long wc0 = A.wave_clock ? wall_clock64() : 0;
    double end[NST], acc[NACC];
    int rows;
    if (w == 0) rows = run_lane_shared<MODEL, D, MASK, false, DEEP, true>(A, g, 0, 0, nullptr, end, acc, &GV);      // (only wave 0 walks table rows)
    else rows = run_lane_shared<MODEL, D, MASK, true, DEEP, true>(A, g, 0, w, &rec[w - 1][0][lane], end, acc);
    __syncthreads();                                           // every window's record is in LDS (a wave whose lanes all ended early is here too)
    double worst = 0.0;
    if (w + 1 < WG_WAVES) {
        int sb_, s_next, se_;
        window_bounds(A.tv.group_len[g], A.n_chunks, A.window, A.t0, w + 1, sb_, s_next, se_, A.t0_delta);
        const bool valid = (A.tv.lane_nsteps[g * WAVE + lane] > s_next) && (s_next < A.tv.group_len[g]);
#pragma unroll
        for (int k = 0; k < NST; k++) {
            const double a = valid ? end[k] : 0.0, b = valid ? rec[w][k][lane] : 0.0;
            double err = fabs(a - b), sc = fmax(fabs(a), fabs(b));
            if (valid && !(err == err)) err = INFINITY;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                err = fmax(err, __shfl_xor(err, o, 64));
                sc = fmax(sc, __shfl_xor(sc, o, 64));
            }
            if (err > 0.0) worst = fmax(worst, err / sc);
        }
    }
#pragma unroll
    for (int k = 0; k < NACC; k++) {
        const double t = wave_sum(acc[k]);
        if (lane == 0) wsum[w][k] = t;
    }
    if (lane == 0) wsum[w][NACC] = worst;
    __syncthreads();
    if (w == 0) {
        double chk = 0.0;
#pragma unroll
        for (int c = 0; c + 1 < WG_WAVES; c++) {
            const double v = wsum[c][NACC];
            chk = fmax(chk, v == v ? v : INFINITY);
        }
        const int c = lane / NACC, k = lane - c * NACC;
        const bool sum_lane = lane < WG_WAVES * NACC;
        const double v = sum_lane ? wsum[c][k] : chk;
        if (A.mbx) {
            double* o = A.mbx + (int64_t)g * MBX_STRIDE;
            if (sum_lane || lane == MBX_CHK) __hip_atomic_store(o + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the record has left before its sequence word does
            if (lane == 0) __hip_atomic_store((unsigned long long*)(o + MBX_SEQ), A.mbx_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
            const int G = A.tv.n_groups;
            if (sum_lane) A.partials[((int64_t)c * NACC + k) * G + g] = v;        // ([window][accumulator][group], as iso_shared_kernel)
            if (lane == WG_WAVES * NACC) A.chk[g] = chk;
        }
    }
    if (A.wave_clock && lane == 0 && rows > 0) {
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        double* o = A.wave_clock + 4 * (int64_t)(blockIdx.x * WG_WAVES + w);
        o[0] = (double)wc0; o[1] = (double)wall_clock64(); o[2] = (double)hw; o[3] = 1.0 + rows;
    }
}


// One translation unit per model (k_iso_shared_ctcrw.hip, ..._ou.hip, ..._bm.hip): one kernel per (dimension, direction
// mask, prefetch depth) is ~100 kernels, minutes of compile time each way -- split, they build side by side.
template <int MODEL, int D, bool DEEP>
static hipError_t launch_masks(const IsoArgs& a, const ReduceArgs& r, dim3 grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, const HeadGain* hg) {
    dim3 block(WG_WAVES * WAVE);
    static const HeadGain no_table = {};                 // (rows == 0: the wg entry stages from a.gain)
    const HeadGain& gv = hg ? *hg : no_table;
    if (MODEL == M_BM_SSM && (a.part_mask[0] & DIR_P2)) return hipErrorInvalidValue;     // BM_SSM has no second variance parameter
    switch (a.part_mask[0]) {
    // hipExtLaunchKernelGGL stamps ev0 / ev1 with the kernel's own begin / end (what rocprof reports), not with the
    // stream position of separately recorded events
    // (ev0 == NULL: a plain launch -- SSDE_OPT_KERNEL_STAMPS off -- which costs the host and the queue a few microseconds less)
#define SSDE_LAUNCH_K(K, M, X) { if (ev0) hipExtLaunchKernelGGL((K<MODEL, D, M, DEEP>), grid, block, 0, s, ev0, ev1, 0, a, X); \
                                 else hipLaunchKernelGGL((K<MODEL, D, M, DEEP>), grid, block, 0, s, a, X); }
#define SSDE_CASE(M) case M: if (a.wg_form) SSDE_LAUNCH_K(iso_shared_wg_kernel, M, gv) else SSDE_LAUNCH_K(iso_shared_kernel, M, r) break;
        SSDE_CASE(0) SSDE_CASE(1) SSDE_CASE(2) SSDE_CASE(3) SSDE_CASE(4) SSDE_CASE(5) SSDE_CASE(6) SSDE_CASE(7)
#if SSDE_SHARED_HAS_P2
        SSDE_CASE(8) SSDE_CASE(9) SSDE_CASE(10) SSDE_CASE(11) SSDE_CASE(12) SSDE_CASE(13) SSDE_CASE(14) SSDE_CASE(15)
#endif
#undef SSDE_CASE
#undef SSDE_LAUNCH_K
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// d = 1 runs the deep rotation, d = 2 the ping-pong pair (see run_segment)
template <int MODEL>
static hipError_t launch_shared_model(int d, const IsoArgs& a, const ReduceArgs& r, dim3 grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, bool,
                                      const HeadGain* hg) {
    if (d == 1) return launch_masks<MODEL, 1, true>(a, r, grid, s, ev0, ev1, hg);
    if (d == 2) return launch_masks<MODEL, 2, false>(a, r, grid, s, ev0, ev1, hg);
    return hipErrorInvalidValue;
}

}  // namespace ssde
