/*
 * ssde.h -- C ABI of the MI355X-native smoothSDE negative-log-likelihood engine.
 *
 * This is the drop-in boundary for ONE path of the reference package
 * (TheoMichelot/smoothSDE): the evaluation of the penalised negative
 * log-likelihood and its parameter gradient, which the reference reaches as
 *
 *     R: tmb_obj$fn(x) / tmb_obj$gr(x)                 (R/sde.R:694-697)
 *       -> .Call("EvalADFunObject", ptr, theta, ctrl)  (src/init.c:8)
 *         -> objective_function<Type>::operator()      (src/smoothSDE.cpp:9-28)
 *           -> nllk_ctcrw / nllk_ou_ssm / nllk_bm_ssm / nllk_sde
 *                                                      (src/nllk/ headers)
 *
 * and which TMB::MakeADFun sets up from `tmb_dat` / `tmb_par` / `map`
 * (R/sde.R:528-536, 542-598, 621-632, 656-669;
 *  .Call("MakeADFunObject", data, parameters, reportenv, control), src/init.c:6).
 *
 * Entry points and what they replace:
 *
 *   ssde_create        <- MakeADFunObject       (src/init.c:6;  R/sde.R:656-658)
 *   ssde_eval          <- EvalADFunObject       (src/init.c:8;  order 0 = fn, 1 = gr)
 *   ssde_eval_device   <- (new) same evaluation, asynchronous, result left in HBM so the
 *                         caller can all-reduce it over RCCL before reading it
 *   ssde_report        <- REPORT(aest_all)      (src/nllk/nllk_ctcrw.hpp:249,
 *                                                nllk_ou_ssm.hpp:215, nllk_bm_ssm.hpp:177)
 *   ssde_smooth        <- (new) fixed-interval Kalman smoother and whitened innovations of the state-space families: what
 *                         the reference's SDE$residuals() stops at (R/sde.R:1186-1228) and aest_all does not give
 *   ssde_smooth_loo    <- (new) leave-one-fix-out predictions of every fix from the rest of its track: deletion residuals, exact
 *                         leave-one-out log predictive densities and per-track outlier counts, from the smoother's own recursion
 *   ssde_forecast_scores <- (new) k-step-ahead forecast errors of every fix from the data k rows back, standardised, with log scores
 *                         and per-track calibration sums per horizon: what the reference gets by rebuilding the data with rows
 *                         blanked to NA once per origin and horizon
 *   ssde_smooth_draws  <- (new) joint posterior draws of the whole state path (backward sampling over the smoother's records):
 *                         what speed, distance travelled, time in a region or multiple imputation are computed from
 *   ssde_predict       <- (new) the smoothed state at any time between or after the rows, from the smoother's records: what the
 *                         reference gets by rebuilding the data with NA rows at the wanted times
 *   ssde_path_stats    <- (new) summaries of those draws reduced on the device: path length, net displacement and weighted time
 *                         inside up to eight boxes per track and draw, without a draw leaving the device
 *   ssde_path_speed    <- (new) the speed |v| along those draws of a CTCRW reduced on the device: integral, maximum and its row,
 *                         heading resultant and weighted time at or below up to eight speeds per track and draw, and per row the
 *                         number of draws at or below each speed
 *   ssde_path_occupancy <- (new) the weighted time those draws spend in every cell of a regular grid, pooled over draws and over
 *                         groups of tracks: a utilisation distribution, summed on the device as integers and so bitwise reproducible
 *   ssde_predict_draws <- (new) those draws' states at any time between or after the rows: the same paths as ssde_smooth_draws,
 *                         refined by Gaussian bridges inside the intervals and simulated past a track's last row, without NA rows
 *   ssde_path_occupancy_fine <- (new) that utilisation distribution on the refined paths of ssde_predict_draws: every interval's
 *                         weight spread over the points of a bridge between its two fixes, so that sparse data leave no holes
 *   ssde_path_proximity <- (new) how close the drawn paths of two tracks come, where, and for how long they are within up to eight
 *                         radii of each other: the states of ssde_predict_draws paired and reduced on the device, per pair and draw
 *   ssde_penalty       <- smoothing penalty     (nllk_ctcrw.hpp:254-280, nllk_sde.hpp:89-124)
 *   ssde_info          <- InfoADFunObject       (src/init.c:7)
 *   ssde_forget        <- (new) drops the memo of ssde_eval
 *   ssde_last_kernel_ms <- (new) measurement hook: duration of the last dominant kernel launch
 *   ssde_kernel_ms_history <- (new) the same for the last n evaluations, read after a timed region
 *   ssde_comm_unique_id / ssde_comm_init_rank
 *                      <- (new) one process per GPU: joins the handles of all ranks into one RCCL communicator, after
 *                         which ssde_eval / ssde_eval_device return the all-reduced batch result on every rank
 *   ssde_laplace_eval  <- what `random = "coeff_re"` makes TMB's fn/gr do (R/sde.R:510-525, 656-658): the Laplace
 *                         approximation of the marginal likelihood over the random-effect coefficients
 *   ssde_hess          <- MakeADHessObject2 / tmb_obj_joint$he(x) (src/init.c:13; R/sde.R:1363): second derivatives of the
 *                         joint penalised nllk -- exact for the Gaussian direct families (BM, OU)
 *   ssde_simulate      <- SDE$simulate          (R/sde.R:1393-1500; CTCRW_cov, R/utility.R:188-196): exact-transition
 *                         simulation of a batch of tracks, written straight into HBM in the reference's long format
 *   ssde_set_option    <- (new) per-handle switches of the measurement hooks
 *   ssde_last_phase_ms <- (new) measurement hook: where the last stamped synchronous evaluation spent its time (kernel,
 *                         finalising launch, all-reduce wait, host side) -- what a multi-GPU run's per-rank account is made of
 *   ssde_comm_allreduce <- (new) sums a caller's HBM buffer over the handle's communicator: hosts that drive several
 *                         handles at once issue ONE collective for all of them (SSDE_OPT_COMM_DEFER)
 *   ssde_destroy       <- external-pointer finalizer of the ADFun object
 *   ssde_last_error    <- Rf_error text         (src/smoothSDE.cpp:25)
 *
 * Plain C types only: no R, torch or HIP types appear in any signature.  A HIP
 * stream crosses the boundary as `void*` (NULL = the null stream).
 *
 * Layout conventions are those of the R objects the reference passes
 * (column-major matrices; `obs` is n x d as.matrix(self$obs()), R/sde.R:531).
 *
 * PARAMETER VECTOR.  `par` is the FULL parameter vector in TMB template order,
 * fixed ("mapped") entries included:
 *   Kalman families (BM_SSM, OU_SSM, CTCRW; nllk_ctcrw.hpp:135-140):
 *       [ log_sigma_obs | coeff_fe (sum ncol_fe) | log_lambda (n_smooth) | coeff_re (sum ncol_re) ]
 *   ESEAL_SSM (nllk_e_seal_ssm.hpp:114-124):
 *       [ log_tau | a1 | log_a2 | coeff_fe | log_lambda | coeff_re ]
 *   direct families (BM, BM_t, OU; nllk_sde.hpp:42-45):
 *       [ coeff_fe | log_lambda | log_decay (only with decaying columns, see n_decay) | coeff_re ]
 *   coeff_fe / coeff_re are ordered parameter-by-parameter exactly like the columns
 *   of the reference's block-diagonal X_fe / X_re (R/sde.R:443-447).
 * `par_fixed[k] != 0` marks an entry that TMB's `map` would hold fixed
 * (R/sde.R:514-515, 565, 595, 627-631): no derivative is computed for it and
 * its gradient slot is returned as 0.  The R shim scatters theta into the full
 * vector and gathers the free gradient entries.
 */
#ifndef SSDE_H
#define SSDE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSDE_ABI_VERSION 12

/* model codes: DATA_STRING(type) of src/smoothSDE.cpp:12-27 */
enum {
    SSDE_MODEL_BM     = 0, /* "BM"      -> nllk_sde + tr_dens BM branch  (tr_dens.hpp:32-37) */
    SSDE_MODEL_OU     = 1, /* "OU"      -> nllk_sde + tr_dens OU branch  (tr_dens.hpp:45-52) */
    SSDE_MODEL_BM_SSM = 2, /* "BM_SSM"  -> nllk_bm_ssm                                    */
    SSDE_MODEL_OU_SSM = 3, /* "OU_SSM"  -> nllk_ou_ssm                                    */
    SSDE_MODEL_CTCRW  = 4, /* "CTCRW"   -> nllk_ctcrw                                     */
    SSDE_MODEL_BM_T   = 5, /* "BM_t"    -> nllk_sde + tr_dens BM_t branch (tr_dens.hpp:38-44): one response,
                              par = (mu, log sigma), degrees of freedom in other_data[0] (R/sde.R:539-541) */
    SSDE_MODEL_ESEAL_SSM = 6, /* "ESEAL_SSM" -> nllk_eseal_ssm (nllk_e_seal_ssm.hpp:83-250): one response, par = (mu, log sigma),
                              state (1, lipid mass), Z_i = (a1, a2 / R_i), H_i = tau^2 / h_i; needs a0, eseal_h, eseal_R */
    SSDE_MODEL_CIR    = 7  /* "CIR"     -> nllk_sde + tr_dens CIR branch (tr_dens.hpp:53-67): par = (log mu_a, log beta, log sigma),
                              positive observations; log I_q(x) is formed directly (no overflow at large x) */
};

/* Which kernel family ran the last evaluation's rows (ssde_info_t.kernel_id).  `path` says which engine path a handle is on;
 * this says which of that path's kernels the dispatch picked for the batch at hand (kernel map). */
enum {
    SSDE_KERNEL_NONE          = 0,  /* nothing evaluated yet */
    SSDE_KERNEL_DIRECT        = 1,  /* direct_kernel: BM / BM_t / OU / CIR transition densities, any slot layout (k_direct.hip) */
    SSDE_KERNEL_DIRECT_FAST   = 2,  /* direct_fast_kernel: at most two parameters with streamed / table-evaluated columns */
    SSDE_KERNEL_ISO_SHARED    = 3,  /* iso_shared_kernel: regular grid, complete tracks -- shared covariance, stationary lanes */
    SSDE_KERNEL_ISO_MASK      = 4,  /* iso_mask_kernel: the lane's own covariance, irregular grid (k_iso.hip) */
    SSDE_KERNEL_ISO_MASK_UNI  = 5,  /* ... regular grid with missing rows (transition hoisted) */
    SSDE_KERNEL_ISO_QUIET     = 6,  /* iso_quiet_kernel: ... with quiet rows (stationary lanes between missing rows) */
    SSDE_KERNEL_ISO_MIXED     = 7,  /* iso_shared_kernel and a general kernel side by side (complete and incomplete wavefronts) */
    SSDE_KERNEL_ISO_SPLIT     = 8,  /* iso_kernel: gradient directions split over several waves per (group, window) */
    SSDE_KERNEL_ISO_DRIFT     = 9,  /* iso_drift_kernel: shared covariance + streamed row-varying drift (k_iso_drift.hip) */
    SSDE_KERNEL_ISO_DRIFT_GEN = 10, /* iso_drift_general_kernel: the same model with the lane's own covariance */
    SSDE_KERNEL_ISO_COLVAR    = 11, /* iso_colvar_kernel: row-varying tau / nu, eight-wave pipeline (k_iso_colvar.hip) */
    SSDE_KERNEL_ISO_FEW       = 12, /* iso_few_kernel: ... few design columns, one wave per (group, window) */
    SSDE_KERNEL_ISO_FULL      = 13, /* iso_full_kernel: per-row H_array, constant tau / nu (4 x 4 covariance lanes) */
    SSDE_KERNEL_DENSE         = 14, /* dense_kernel: general Kalman step, lane = track (k_dense.hip) */
    SSDE_KERNEL_TV            = 15, /* tv_filter_kernel: row-varying coefficients, lane = gradient direction (k_tv.hip) */
    SSDE_KERNEL_TV_DENSE      = 16, /* ... with full-covariance lanes (k_tv_dense.hip; ESEAL_SSM too) */
    SSDE_KERNEL_ISO_ADJ       = 17  /* iso_adj_kernel: row-varying tau / nu / drift, gradient by a reverse sweep (k_iso_adj.hip) */
};

/* status codes (0 = ok).  HIP runtime failures are reported as SSDE_ERR_HIP with
 * the hipError_t text in ssde_last_error(). */
enum {
    SSDE_OK            = 0,
    SSDE_ERR_ARG       = 1, /* malformed descriptor / argument                         */
    SSDE_ERR_MODEL     = 2, /* "Unknown SDE type" (src/smoothSDE.cpp:25) / unsupported */
    SSDE_ERR_HIP       = 3, /* HIP runtime error                                       */
    SSDE_ERR_NODEVICE  = 4, /* no gfx950 device visible: there is NO CPU fallback      */
    SSDE_ERR_ALLOC     = 5
};

/* how a missing observation is recognised (Q5 of SURVEY.md Appendix A) */
enum {
    SSDE_NA_R_ONLY = 0, /* R_IsNA(): NaN whose low word is 1954 (nllk_ctcrw.hpp:214, tr_dens.hpp:31) */
    SSDE_NA_ANY_NAN = 1 /* any NaN counts as missing (non-R hosts)                                    */
};

/* ssde_desc.flags */
#define SSDE_FLAG_DEVICE_DATA   0x1u /* id/times/obs/x_fe/x_re/h_array pointers are HBM pointers on `device` */
#define SSDE_FLAG_FORCE_DENSE   0x2u /* disable the isotropic register path (testing the dense path)         */
#define SSDE_FLAG_NO_UNIFORM_DT 0x4u /* disable hoisting of the transition matrices on a regular time grid    */
#define SSDE_FLAG_EXACT_HESS    0x8u /* the caller will ask for exact second derivatives (ssde_hess, ssde_laplace_eval): a state-space
                                        batch (H = sigma_obs^2 I) that ssde_create puts on the lane = track register kernels -- constant
                                        coefficients, a smooth drift, row-varying tau / nu: first-order kernels -- gets a second,
                                        lane = direction copy of its rows for the second-order pass (k_tv_hess.hip): ~0.64 KB of HBM
                                        per row on top of the tiles, kept only when that is at most a third of the device memory still
                                        free (ssde_info.exact_hess_scope tells).  Without the flag (or the copy) such a handle answers
                                        SSDE_ERR_MODEL and the Laplace layer differences the gradient.  Every track shard of a
                                        multi-device handle keeps its own copy; the ranks of a communicator sum theirs. */

/* A random-effect design block given as a FUNCTION of one covariate instead of as n x K numbers: a piecewise-cubic
 * table (regression-spline bases -- mgcv "cr", "cs", "bs", "ps" -- are exactly that; thin-plate bases are not and
 * keep being streamed):
 *     X[i, k] = sum_{m=0..3} coef[(iv * n_cols + k) * 4 + m] * t^m,   t = x[i] - knots[iv],
 *     iv = the interval knots[iv] <= x[i] < knots[iv+1] (x outside the knot range uses the first / last interval).
 * The direct families then read 8 B/row (x) where the streamed block costs 8 K B/row. */
typedef struct ssde_ppbasis {
    const double *x;              /* [n] covariate (host, or HBM with SSDE_FLAG_DEVICE_DATA) */
    int32_t  n_knots;             /* breakpoints; n_knots - 1 intervals */
    int32_t  n_cols;              /* K == ncol_re[j] */
    const double *knots;          /* [n_knots] increasing (host) */
    const double *coef;           /* [(n_knots - 1) * n_cols * 4] (host) */
} ssde_ppbasis;

typedef struct ssde_desc {
    int32_t  abi_version;     /* SSDE_ABI_VERSION */
    int32_t  model;           /* SSDE_MODEL_* */
    int32_t  n_dim;           /* d = ncol(obs).  Every kernel is sized for d <= 2; a wider response is evaluated as the pairs of
                                 columns (0,1), (2,3), ... behind the one handle (the likelihood is a sum over dimensions:
                                 nllk_ctcrw.hpp:49-89 are block-diagonal in the dimension, nllk_sde.hpp:77-84 loops over it),
                                 which needs a P0 and an H_array without entries between different pairs.  BOUND: a measurement
                                 covariance or P0 that couples the pairs is accepted for d <= 8 (the whole response as one filter, F by
                                 LU -- k_dense.hip, k_dense_wide.hip -- on one device, host or device-resident arrays, or on every
                                 whole-track shard of several); d >= 9 with coupling is SSDE_ERR_MODEL */
    int32_t  n_par;           /* q = SDE parameters per row: d+1 (BM, BM_t, BM_SSM), d+2 (OU, OU_SSM, CTCRW) */
    int64_t  n;               /* rows of the long-format data (all tracks concatenated) */
    const double *id;         /* [n] track codes (TMB passes the factor as doubles); only
                                 id[i] != id[i-1] is ever used (nllk_ctcrw.hpp:196)     */
    const double *times;      /* [n]   DATA_VECTOR(times).  Any increasing stamps; recognised at create (the numbers are the
                                 reference's either way): a regular grid (transition hoisted), and a regular
                                 schedule whose failed fixes are absent from the data -- intervals that are small whole
                                 multiples of one step -- which is laid out on its lattice and run as a regular grid with
                                 missing rows */
    const double *obs;        /* [n*d] DATA_MATRIX(obs), column-major */

    /* design blocks, one per SDE parameter j = 0..q-1: the X_list_fe[[j]] /
     * X_list_re[[j]] of R/sde.R:412-417 (the diagonal blocks of X_fe / X_re).
     * x_fe[j] == NULL with ncol_fe[j] == 1 means an intercept-only column of ones. */
    const int32_t *ncol_fe;       /* [q] */
    const double *const *x_fe;    /* [q] each n x ncol_fe[j], column-major, or NULL */
    const int32_t *ncol_re;       /* [q] number of random-effect columns of parameter j (may be 0) */
    const double *const *x_re;    /* [q] each n x ncol_re[j], column-major, or NULL when 0 columns  */

    /* smoothing penalty: DATA_IVECTOR(ncol_re) + DATA_SPARSE_MATRIX(S) of the reference */
    int32_t  n_smooth;            /* number of penalty blocks; 0 = no random effects (R/sde.R:511-518) */
    const int32_t *smooth_ncol;   /* [n_smooth] columns of each block (reference `ncol_re`)           */
    const double *s_blocks;       /* the diagonal blocks of S, each smooth_ncol[s]^2 column-major,
                                     concatenated */
    int32_t  include_penalty;     /* DATA_INTEGER(include_penalty): read by nllk_sde only (Q7) */

    /* Kalman families only */
    int64_t  n_seg;               /* rows of a0 = number of ID segments (R/sde.R:547,574) */
    const double *a0;             /* [n_seg x sdim] column-major, or NULL = built from obs as R/sde.R:549,576-580 */
    const double *p0;             /* [sdim x sdim] column-major, or NULL = default of R/sde.R:554,584 */
    const double *h_array;        /* [d x d x n] DATA_ARRAY(H_array), or NULL = sigma_obs^2 I (R/sde.R:563-568,593-598) */

    const uint8_t *par_fixed;     /* [n_par_full] or NULL (= nothing fixed) */
    int32_t  na_mode;             /* SSDE_NA_* */
    int32_t  device;              /* HIP device ordinal, -1 = current device */
    uint32_t flags;               /* SSDE_FLAG_* */
    uint32_t reserved;
    const double *other_data;     /* DATA_VECTOR(other_data) (nllk_sde.hpp:29): [0] = degrees of freedom for BM_t; NULL otherwise */
    int32_t  n_other_data;
    /* decaying random-effect columns, direct families only (nllk_sde.hpp:30-32, 47-58; R/sde.R:163-177, 635-648):
     * column col_decay[c] of X_re (0-based, counted over the concatenated blocks of all SDE parameters, i.e. the
     * index inside coeff_re) is multiplied row by row by exp(-exp(log_decay[ind_decay[c]]) * t_decay).
     * The parameter vector then carries log_decay: [ coeff_fe | log_lambda | log_decay (n_decay) | coeff_re ]. */
    int32_t  n_decay;             /* number of decay rates, 0 = feature unused (the reference's dummy log_decay is dropped) */
    const double *t_decay;        /* [q * n], entry j*n + i belongs to row i of SDE parameter j (the rows of X_re) */
    int32_t  n_decay_cols;
    int32_t  reserved3;
    const int32_t *col_decay;     /* [n_decay_cols] */
    const int32_t *ind_decay;     /* [n_decay_cols] 0-based index into log_decay */
    /* ESEAL_SSM only: DATA_VECTOR(h) (daily drift dives) and DATA_VECTOR(R) (non-lipid tissue mass),
     * nllk_e_seal_ssm.hpp:100-101, R/sde.R:611-614 */
    const double *eseal_h;        /* [n] */
    const double *eseal_R;        /* [n] */
    /* [q] or NULL.  basis_re[j] != NULL: the random-effect block of SDE parameter j is evaluated from this table
     * (x_re[j] is then ignored by the engine and may be NULL). */
    const ssde_ppbasis *const *basis_re;
    /* Single-process multi-GPU (the reference's host is ONE R process, R/sde.R:656-669): n_devices > 1 shards whole
     * tracks (contiguous ID segments, balanced by rows) over devices[0..n_devices), one engine per device; every
     * ssde_eval then runs all shards concurrently and sums their 2 + p doubles with one ncclAllReduce per device
     * inside ncclGroupStart/End (communicators from ncclCommInitAll).  Host arrays only (no SSDE_FLAG_DEVICE_DATA).
     * n_devices <= 1 or devices == NULL: the single device `device`.  A device listed more than once is accepted for
     * rehearsal on a one-GPU machine: its shards are then summed by a small kernel instead of RCCL (which refuses
     * two ranks on one device). */
    int32_t  n_devices;
    int32_t  reserved4;
    const int32_t *devices;       /* [n_devices] HIP device ordinals */
} ssde_desc;

typedef struct ssde_handle ssde_handle;

/* facts about a created engine (InfoADFunObject counterpart) */
typedef struct ssde_info_t {
    int32_t n_par_full;     /* length of `par` / `grad` */
    int32_t n_free;         /* entries with par_fixed == 0 */
    int32_t sdim;           /* Kalman state dimension (0 for direct families) */
    int32_t path;           /* 0 direct, 1 isotropic register Kalman (constant coefficients), 2 dense Kalman,
                               3 isotropic Kalman with row-varying coefficients */
    int32_t const_coeff;    /* 1 if every SDE parameter is intercept-only */
    int32_t uniform_dt;     /* 1 if one dt is shared by every scored interval (transition matrices hoisted) */
    int64_t n_tracks;       /* ID segments */
    int64_t n_rows;         /* n */
    int64_t n_steps;        /* rows that are not the first row of a segment */
    int64_t hbm_bytes;      /* resident bytes of the tiled streams */
    double  algo_bytes_per_row; /* 8*(d + 1 + d*d*[H_array] + K_row) */
    int32_t n_kernel_blocks;/* workgroups of the main kernel (last evaluation) */
    int32_t lanes_per_track;/* direction parts x time windows (register path), direction blocks (dense),
                               direction lanes x time windows (row-varying path) */
    int32_t window;         /* warm-up rows of a time window in the last evaluation (0 = sequential) */
    int32_t window_retries; /* evaluations repeated because the window hand-over check failed */
    double  window_check;   /* largest relative hand-over disagreement of the last ssde_eval (<= 1e-11 when the windows agree; a value up
                               to 1e-8 is accepted only as a ROUNDING FLOOR: one that stayed flat while the warm-up was quadrupled twice --
                               very precise fixes -- and is reported here as it is) */
    double  main_kernel_ms; /* HIP-event duration of the dominant kernel launch of the last evaluation */
    int64_t main_kernel_rows;/* rows scored by that launch (the rest belong to the small concurrent launches) */
    double  required_bytes_per_row; /* bytes per row the engine's resident layout really has to read: algo_bytes_per_row
                                       minus the 8 B/row of `times` when the grid is globally regular and the dt channel
                                       is not even stored (24 -> 16 for 2-D constant-coefficient models) */
    int64_t n_evals;        /* evaluations that ran on the device (window retries included) */
    int64_t n_memo_hits;    /* ssde_eval calls answered from the memoised last result (same par, bitwise) */
    int32_t n_devices;      /* shards of a single-process multi-GPU handle (1 otherwise) */
    int32_t comm_ranks;     /* ranks of the RCCL communicator joined with ssde_comm_init_rank (1 = none) */
    double  window_check_max; /* largest ACCEPTED hand-over disagreement over every ssde_eval since ssde_create */
    /* how the engine laid the batch out (Kalman register path; 0 elsewhere) -- ABI 7 */
    int64_t n_rows_tiled;   /* rows of the resident layout: n_rows, or more when a schedule with absent fixes was laid out
                               on its lattice */
    int32_t n_groups;       /* 64-track wavefront groups */
    int32_t n_clean_groups; /* ... of which every track has every row: the shared-covariance kernel's share on a regular grid */
    int32_t quiet_window;   /* > 0: the general kernel of the last evaluation ran rows that lie this many rows past the last missing
                               observation of their wavefront with the stationary gains; 0: no such rows */
    int32_t kernel_id;      /* SSDE_KERNEL_*: the kernel family that ran the rows of the last evaluation -- ABI 10 */
    double  quiet_share;    /* share of the blocks of wavefronts with missing rows that qualify, at a nominal 128-row memory
                               (found at ssde_create; 0 when the layout has no such wavefront or the grid is irregular) */
    int32_t comm_ranks_reported; /* what ncclCommCount says about the joined communicator (0 = none joined); comm_ranks above
                               echoes the caller's argument -- ABI 10 */
    int32_t exact_hess_scope; /* what ssde_hess is exact over on this handle: 0 nothing (difference the gradient), 1 the drift coefficients
                                 (+ log_lambda), 2 every coefficient of a direct family (+ log_lambda), 3 every free entry (was reserved: 0) */
    int64_t lagstat_rows;   /* rows of the last evaluation taken from the lag statistics built at create instead of streamed (DESIGN.md
                               §3.3d; 0: every row was streamed) -- ABI 11 */
    double  lagstat_create_ms; /* what building those statistics cost ssde_create (0: none built) -- ABI 11 */
} ssde_info_t;

/* Create an engine: validates the descriptor, finds the ID segments, uploads the
 * data ONCE and re-tiles it in HBM (tracks -> wavefront lanes, time-major) so that
 * every later evaluation streams it with coalesced loads.  The caller keeps
 * ownership of every host array; nothing is aliased after return. */
int ssde_create(const ssde_desc *desc, ssde_handle **out);

/* fn(par) / gr(par).  order 0: *value only.  order 1: *value and grad[n_par_full].
 * value = nllk including the smoothing penalty exactly as the reference adds it.
 * A non-finite nllk is RETURNED (status SSDE_OK), not raised.
 * The last result is memoised on the bit pattern of `par`: optim's fn(x); gr(x) pair (R/sde.R:694-696) costs ONE
 * device evaluation on the paths where the gradient rides along with the value at no extra memory traffic (shared-
 * covariance and direct kernels: an order-0 call evaluates order 1 there), and a repeated call costs none. */
int ssde_eval(ssde_handle *h, const double *par, int32_t n_par_full, int32_t order,
              double *value, double *grad);

/* Same evaluation WITHOUT the penalty and without synchronising: enqueues on
 * `stream` and leaves [nllk_data, grad..., window_check] (2 + n_par_full doubles) in
 * the HBM buffer `out_dev`.  Used by multi-GPU hosts: shard tracks, all-reduce
 * out_dev, then add ssde_penalty once.  window_check is the largest relative
 * disagreement between overlapping time windows of the register path (0 when the
 * evaluation ran as one sequential window): the caller must treat the result as
 * invalid when it exceeds 1e-11 (ssde_eval re-evaluates with a longer overlap by
 * itself; asynchronous callers do the same after ssde_widen_windows). */
int ssde_eval_device(ssde_handle *h, const double *par, int32_t n_par_full, int32_t order,
                     double *out_dev, void *stream);

/* Smoothing penalty and its gradient (host arithmetic, parameter-only). grad may be NULL;
 * otherwise it is ADDED into grad[n_par_full]. */
int ssde_penalty(ssde_handle *h, const double *par, int32_t n_par_full, double *value, double *grad);

/* One-step-ahead predicted states for every row: aest_all [n x sdim] column-major. */
int ssde_report(ssde_handle *h, const double *par, int32_t n_par_full, double *aest_all);

/* Fixed-interval smoother of the Kalman families at `par` (definitions: DESIGN.md §3.9).  Any output may be NULL, not all:
 *   a_smooth [n x sdim]        column-major, the aest_all layout: E[state at row i | the whole track]
 *   P_smooth [n x sdim x sdim] element (i, r, c) at i + n * (r + sdim * c): its covariance
 *   resid    [n x n_dim]       whitened one-step-ahead innovations C_i^-1 v_i (C_i the lower Cholesky factor of F_i)
 * NaN on rows that carry no state (a track's first row, one-row tracks) and, for resid, on rows without an update (those, NA
 * rows, detF <= 0).  SSDE_ERR_MODEL for the direct families and ESEAL_SSM (as ssde_report).  Leaves the memo, the window
 * state and every later ssde_eval result as they were; the per-row records live in a buffer of the call's own, capped by
 * SSDE_OPT_SMOOTH_BUDGET_MB (tracks are processed in chunks of whole wavefront groups; the result does not depend on it). */
int ssde_smooth(ssde_handle *h, const double *par, int32_t n_par_full, double *a_smooth, double *P_smooth, double *resid);

/* Leave-one-out (deletion) residuals and predictive densities of the Kalman families at `par` (definitions: DESIGN.md §3.20): what
 * every OTHER fix of the track says about fix j, from the smoother's own records and backward recursion -- no refit, no new forward
 * pass.  With r, N the smoother's backward quantities BEFORE row j is folded in, w_j = F_j^-1 v_j - K_j' r and
 * M_j = F_j^-1 + K_j' N K_j (at a track's last state row F_j^-1 v_j and F_j^-1), y_j | y_-j ~ N(y_j - D_j w_j, D_j) with D_j = M_j^-1
 * (de Jong 1989).  A SERVED row is a state row whose record took an update (resid of ssde_smooth is not NaN) and whose M_j is
 * positive definite.  Per-row outputs, each may be NULL, indexed by the caller's row:
 *   loo_mean  [n x n_dim]          column-major: E[y_j | every other fix of the track]
 *   loo_cov   [n x n_dim x n_dim]  element (i, r, c) at i + n * (r + n_dim * c): D_j, symmetrised
 *   loo_resid [n x n_dim]          z_j = C_j^-1 (y_j - loo_mean_j), C_j the lower Cholesky factor of D_j (resid's convention).  N(0, I)
 *                                  under the model at every row, but -- unlike resid -- NOT independent between rows: two deletion
 *                                  residuals of one track share all the other fixes
 *   lpd       [n]                  log p(y_j | y_-j) = -(n_dim log 2 pi + log det D_j + q_j) / 2, q_j = z_j' z_j
 * NaN on every row that is not served (a track's first row, one-row tracks, NA rows, detF <= 0); where only the Cholesky factor of
 * D_j fails (a pivot <= 0 or not finite) loo_mean and loo_cov are kept, loo_resid and lpd are NaN and the row enters no statistic.
 *   stats [n_tracks x n_stat], element (t, k) at t + n_tracks * k, n_stat = 4 + n_thr, t the ID segment's ordinal in the caller's
 *   data, or NULL:  0 the served rows; 1 the sum of lpd_j (the track's leave-one-out score); 2 max q_j; 3 the caller's 0-based row
 *   attaining it (the smallest of a tie: ssde_path_speed's convention); 4 + r the served rows with q_j > thr[r].  A track without a
 *   served row: 0, 0, NaN, NaN and zero counts.
 *   thr [n_thr] host memory, every entry finite and >= 0, on the q scale (the caller's chi-square_{n_dim} quantiles).
 * Every handle layout ssde_smooth serves is served.  An uncoupled wide response (column pairs) serves loo_mean, loo_cov (cross-pair
 * blocks exactly 0) and loo_resid; lpd and stats need a per-row sum across the pair handles there: SSDE_ERR_MODEL.  SSDE_ERR_MODEL
 * for the direct families and ESEAL_SSM.  SSDE_ERR_ARG: all five outputs NULL, n_thr outside 0 .. SSDE_LOO_MAX_THR, thr NULL with
 * n_thr > 0, a threshold that is not finite or < 0, n_thr > 0 without stats, flags != 0.  Isolation, chunking and buffers as
 * ssde_smooth; the result is bitwise independent of the chunking and of the devices. */
#define SSDE_LOO_MAX_THR 8
int ssde_smooth_loo(ssde_handle *h, const double *par, int32_t n_par_full,
                    double *loo_mean, double *loo_cov, double *loo_resid, double *lpd,
                    const double *thr, int32_t n_thr, double *stats, uint32_t flags);

/* Multi-step-ahead forecast errors and scores of the Kalman families at `par` (definitions: DESIGN.md §3.21).  For a horizon k >= 1
 * and a target row t of a track whose rows are first .. last, with t - k >= first, the forecast of row t from the data through row
 * t - k is the one-step prediction of row r = t - k + 1 (the smoother's forward record of that row) pushed through the rows
 * r .. t - 1 as the filter pushes it through NA rows -- a <- T_i a + drift, P <- T_i P T_i' + Q_i with row i's own parameters and the
 * interval the handle holds for row i; the data of those rows are ignored -- then m = Z a, S = Z P Z' + H_t (sigma_obs^2 I or row
 * t's H_array slice).  k = 1 is the filter's own innovation.  A target (t, k) is SCORED when y_t is not NA (the handle's na_mode), m
 * and S are finite and the lower Cholesky factor C of the symmetrised S has finite, positive pivots; then z = C^-1 (y_t - m),
 * q = z'z, lpd = -(n_dim log 2 pi + log det S + q) / 2: ssde_smooth_loo's conventions.  Horizons count the caller's rows: on a
 * lattice-padded handle the chain steps through the padded rows, which are never starts or targets.
 *   horizon   [n_h] host memory, strictly increasing, each 1 .. SSDE_AHEAD_MAX_STEP; n_h in 1 .. SSDE_AHEAD_MAX_H
 *   z_ahead   [n x n_dim x n_h]  element (t, c, j) at t + n * (c + n_dim * j); NaN where (t, horizon[j]) is not scored
 *   lpd_ahead [n x n_h]          NaN likewise
 *   thr       [n_thr] host memory, on the q scale: finite, >= 0; n_thr in 0 .. SSDE_AHEAD_MAX_THR
 *   stats     [n_tracks x n_stat x n_h], n_stat = 5 + n_thr, element (track, s, j) at track + n_tracks * (s + n_stat * j), track the ID
 *             segment's ordinal in the caller's data: 0 the scored targets; 1 the sum of lpd; 2 of q; 3 of |y_t - m|^2; 4 of the lead
 *             time (the handle's intervals of rows t - k .. t - 1 added up); 5 + r the scored targets with q > thr[r].  A track without
 *             a scored target at that horizon: 0 in every slot.
 * Any of the three outputs may be NULL, not all of them.  An uncoupled wide response (column pairs) serves z_ahead only (lpd_ahead
 * and stats need a per-row sum across the pair handles: SSDE_ERR_MODEL, as ssde_smooth_loo); one coupled filter of three or more
 * columns, the direct families and ESEAL_SSM: SSDE_ERR_MODEL.  SSDE_ERR_ARG, before anything touches the device: NULL h / par /
 * horizon, n_h outside 1 .. SSDE_AHEAD_MAX_H, a horizon out of range or not strictly increasing, n_thr outside
 * 0 .. SSDE_AHEAD_MAX_THR, thr NULL with n_thr > 0, a threshold that is not finite or < 0, n_thr > 0 without stats, all outputs NULL,
 * flags != 0.  Isolation, chunking and buffers as ssde_smooth; the result is bitwise independent of the budget, of the devices, of
 * repeated calls and of which outputs are asked for. */
#define SSDE_AHEAD_MAX_H     8     /* horizons per call */
#define SSDE_AHEAD_MAX_STEP 64     /* largest horizon */
#define SSDE_AHEAD_MAX_THR   8
int ssde_forecast_scores(ssde_handle *h, const double *par, int32_t n_par_full,
                         const int32_t *horizon, int32_t n_h,
                         double *z_ahead, double *lpd_ahead,
                         const double *thr, int32_t n_thr, double *stats, uint32_t flags);

/* Joint posterior draws of the whole state path at `par` (definitions: DESIGN.md §3.10): backward sampling over the smoother's own
 * forward records, so a draw carries the dependence BETWEEN rows that the row-wise a_smooth / P_smooth leave out.
 *   draws [n x sdim x n_draws]: element (i, c, k) at i + n * (c + sdim * k) -- draw k is one aest_all-layout matrix; it is draw number
 *   draw0 + k of the stream `seed`.  NaN on rows without a state.  flags: SSDE_DRAWS_DEVICE_OUT (1) = `draws` is an HBM pointer on the
 *   handle's device (single-device handles; nothing is copied to the host).
 * Every deviate is a pure function of (seed, the track's ordinal in the caller's data, the state row's position in the track as the
 * handle holds it -- the lattice position on a lattice-padded handle --, draw number, state column): Philox4x32-10 + Box-Muller as
 * ssde_simulate.  The result does not depend on SSDE_OPT_SMOOTH_BUDGET_MB, on the devices or on how the draws are cut over calls.
 * SSDE_ERR_MODEL for the direct families and ESEAL_SSM (as ssde_smooth) and for a handle whose response runs as ONE coupled filter of
 * three or more columns (a per-row H_array or P0 that couples them); uncoupled wide responses run as column pairs and ARE served.
 * SSDE_ERR_ARG for n_draws < 1, draw0 < 0, draw0 + n_draws >= 2^28, NULL pointers, an unknown flag, and SSDE_DRAWS_DEVICE_OUT on a
 * multi-device handle.  Leaves the memo, the window state, the TV records and every later ssde_eval result as they were. */
#define SSDE_DRAWS_DEVICE_OUT 1u
int ssde_smooth_draws(ssde_handle *h, const double *par, int32_t n_par_full, uint64_t seed, int64_t draw0, int32_t n_draws,
                      double *draws, uint32_t flags);

/* The smoothed state at any time from the smoother's records at `par` (definitions: DESIGN.md §3.11).  Query k is (q_row[k], q_off[k]):
 * a caller's row (0-based) and an offset >= 0 past its time stamp; the answer is the smoothed state of a NA row inserted there that
 * carries row q_row[k]'s covariates.  An offset inside the row's interval interpolates; past a track's last row it forecasts.
 *   a_pred [n_query x sdim]        column-major: E[state at the query time | the whole track]
 *   P_pred [n_query x sdim x sdim] element (k, r, c) at k + n_query * (r + sdim * c): its covariance; may be NULL
 * Queries may come in any order, repeat and share intervals.  NaN in every output of a query, with status SSDE_OK, where the row is a
 * track's first row (or a one-row track), where the offset passes the next fix of the track by more than rounding, and where the row
 * attempted an update and rejected it (det F <= 0); a NA row is served.  SSDE_ERR_ARG for NULL q_row / q_off / a_pred, n_query < 1, a
 * row outside [0, n), an offset that is negative or not finite; SSDE_ERR_MODEL exactly where ssde_smooth_draws gives it.  Multi-device
 * handles and column pairs are served (cross-pair covariance blocks are exactly 0).  Leaves the memo, the window state, the TV
 * records and every later ssde_eval / ssde_smooth / ssde_smooth_draws result as they were; its buffers are its own, chunked by whole
 * wavefront groups under SSDE_OPT_SMOOTH_BUDGET_MB, and the result does not depend on the chunking. */
int ssde_predict(ssde_handle *h, const double *par, int32_t n_par_full, const int64_t *q_row, const double *q_off, int64_t n_query,
                 double *a_pred, double *P_pred);

/* Joint posterior draws of the state at any time at `par` (definitions: DESIGN.md §3.14).  Queries are ssde_predict's: query k is
 * (q_row[k], q_off[k]), a caller's row (0-based) and an offset >= 0 past its time stamp; they may come in any order, repeat and share
 * intervals.  Draw q is draw number draw0 + q of the stream `seed` and it is THE SAME PATH ssde_smooth_draws, ssde_path_stats and
 * ssde_path_occupancy use for that seed and draw number: the states at the rows are theirs (offset 0 returns the row's draw and an
 * offset equal to the interval the next row's, bitwise), and the call adds the states between them -- a Gaussian bridge between the
 * draw's states at the two rows around the query, with row q_row[k]'s covariates -- and after a track's last row.
 *   draws_at [n_query x sdim x n_draws]: element (k, c, q) at k + n_query * (c + sdim * q); columns as in a_pred.
 * The offsets of one interval must go into ONE call to be jointly distributed: an answer is a pure function of the seed, the track,
 * the row, the draw number and the SET of distinct offsets of its interval in this call (each offset is drawn given the one below
 * it).  It does not depend on the order of the queries, their duplicates, the other intervals' queries, SSDE_OPT_SMOOTH_BUDGET_MB,
 * how the draws are batched or cut over calls, the devices or the column pairs.
 * NaN in every column of a query, with status SSDE_OK, exactly where ssde_predict gives NaN, and wherever the draw itself is NaN at an
 * end the answer depends on.  SSDE_ERR_ARG as for ssde_predict's query arguments and ssde_smooth_draws' draw arguments, for
 * flags != 0, and for a handle with 2^32 or more tracks or an interval with 2^32 or more distinct offsets; SSDE_ERR_MODEL exactly where
 * ssde_smooth_draws gives it.  Multi-device handles, column pairs, lattice-padded handles and row-varying parameters are served.
 * Leaves the memo, the window state, the TV records, n_evals / n_memo_hits and every later result of the other calls as they were. */
int ssde_predict_draws(ssde_handle *h, const double *par, int32_t n_par_full, const int64_t *q_row, const double *q_off, int64_t n_query,
                       uint64_t seed, int64_t draw0, int32_t n_draws, double *draws_at, uint32_t flags);

/* Summaries of posterior state paths at `par`, reduced on the device (definitions: DESIGN.md §3.12).  Draw q is draw number draw0 + q
 * of the stream `seed`: exactly the path ssde_smooth_draws returns for it.  A track's state rows are the CALLER's rows first + 1 ..
 * last (a lattice-padded handle samples its padded rows, which take part in no statistic); the position columns are state column 2a
 * of response column a for a CTCRW and state column a for OU_SSM / BM_SSM.
 *   stats [n_tracks x n_stat x n_draws], n_stat = 2 + n_regions: element (t, k, q) at t + n_tracks * (k + n_stat * q), t the ID
 *   segment's ordinal in the caller's data.
 *     k = 0      path length: the sum over consecutive state rows of the Euclidean distance between their positions (0 for one row)
 *     k = 1      net displacement: the distance between the positions at the last and the first state row
 *     k = 2 + r  the sum over state rows j of w_j 1[lo_c <= p_jc < hi_c for every position column c] of region r
 *   regions [n_regions x 4] row-major: lo_1, hi_1, lo_2, hi_2 (the second pair is not read for n_dim = 1); +-inf bounds make half-planes.
 *   weight  [n] host memory, indexed by the caller's row, or NULL for w_j = 1.  Weights are not validated: a non-finite weight enters
 *   the sums it is added to.
 * NaN in every statistic of every draw of a track without a state row (a one-row track), and in every statistic of a (track, draw)
 * whose path has a non-finite position on a state row (the negative-P0 / det F <= 0 corner of §3.10).
 * SSDE_ERR_ARG for NULL par / stats, n_draws < 1, draw0 < 0, draw0 + n_draws >= 2^28, n_regions outside 0 .. SSDE_PATH_MAX_REGIONS,
 * regions NULL with n_regions > 0, a NaN bound or lo > hi, flags != 0.  SSDE_ERR_MODEL for the direct families and ESEAL_SSM (as
 * ssde_smooth) and for EVERY handle with n_dim > 2, column pairs and coupled filters alike: a distance needs the position columns in
 * one lane, and the pairs of a wide response sit in different handles.  Multi-device handles are served (shards own whole tracks).
 * Leaves the memo, the window state, the TV records, n_evals / n_memo_hits and every later ssde_eval / ssde_smooth / ssde_smooth_draws /
 * ssde_predict result as they were; its buffers are its own, chunked by whole wavefront groups under SSDE_OPT_SMOOTH_BUDGET_MB, and the
 * result does not depend on the chunking, on how the draws are cut over calls or on the devices. */
#define SSDE_PATH_MAX_REGIONS 8
int ssde_path_stats(ssde_handle *h, const double *par, int32_t n_par_full, uint64_t seed, int64_t draw0, int32_t n_draws,
                    const double *regions, int32_t n_regions, const double *weight, double *stats, uint32_t flags);

/* Speed along posterior state paths at `par`, reduced on the device (definitions: DESIGN.md §3.17).  Draws, state rows and weights are
 * exactly those of ssde_path_stats: draw q is draw number draw0 + q of the stream `seed`, the path ssde_smooth_draws returns; a track's
 * state rows are the CALLER's rows first + 1 .. last (a lattice-padded handle samples its padded rows, which take part in nothing);
 * weight [n] host memory by the caller's row, or NULL for w_j = 1, not validated.  A CTCRW only: v_a is state column 2a + 1 of response
 * column a, and the speed at a state row is s = |v_1| for n_dim = 1 and s = sqrt(v_1^2 + v_2^2) for n_dim = 2.
 *   stats [n_tracks x n_stat x n_draws], n_stat = 5 + n_thr: element (t, k, q) at t + n_tracks * (k + n_stat * q), t the ID segment's
 *   ordinal in the caller's data.
 *     k = 0      sum over state rows j of w_j s_j: with dt weights the integral of speed; divided by sum w_j the mean speed
 *     k = 1      max over j of s_j
 *     k = 2      the caller's row (0-based, as a double) that attains the maximum; a tie gives the smallest row
 *     k = 3, 4   the resultant sum over j of w_j v_jc / s_j for c = 1, 2; a row with s_j = 0 adds nothing; for n_dim = 1, k = 3 is
 *                sum w_j sign(v_j) and k = 4 is 0.  |resultant| / sum w_j is the usual measure of directional persistence
 *     k = 5 + r  sum over j of w_j 1[s_j <= thr[r]]
 *   row_below [n x n_thr] uint32: element (j, r) at j + n * r, j the caller's row: the number of the call's draws with a finite
 *   s_j <= thr[r]; 0 on rows without a state (a track's first row, one-row tracks).  The call overwrites it.  Counts of disjoint draw
 *   ranges add up exactly on the host.
 * Either output may be NULL, not both; row_below must be NULL when n_thr = 0.  thr [n_thr] host memory: each >= 0, +inf allowed, in
 * any order.
 * NaN in every statistic of every draw of a track without a state row, and in every statistic of a (track, draw) with a non-finite
 * velocity column on a state row; a non-finite s_j is counted in no row_below entry.
 * SSDE_ERR_ARG for NULL h / par, stats and row_below both NULL, n_draws < 1, draw0 < 0, draw0 + n_draws >= 2^28, n_thr outside
 * 0 .. SSDE_SPEED_MAX_THR, thr NULL with n_thr > 0, a threshold that is NaN or < 0, row_below non-NULL with n_thr = 0, flags != 0.
 * SSDE_ERR_MODEL for OU_SSM and BM_SSM (their state holds no velocity) and wherever ssde_path_stats gives it (the direct families,
 * ESEAL_SSM, n_dim > 2).  Every check runs before anything touches the device.  Multi-device handles, lattice-padded handles, PATH_TV
 * handles, SSDE_FLAG_FORCE_DENSE, per-row H_array and a general P0 are served.  Leaves the memo, the window state, the TV records,
 * n_evals / n_memo_hits and every later result of every other call as they were.  The result is bitwise independent of
 * SSDE_OPT_SMOOTH_BUDGET_MB, the devices, how the draws are batched and repeated calls; stats of a draw range cut over calls is bitwise
 * the whole range's, and stats / row_below are the same numbers whether asked for alone or together. */
#define SSDE_SPEED_MAX_THR 8
int ssde_path_speed(ssde_handle *h, const double *par, int32_t n_par_full, uint64_t seed, int64_t draw0, int32_t n_draws,
                    const double *thr, int32_t n_thr, const double *weight, double *stats, uint32_t *row_below, uint32_t flags);

/* Occupancy grids of posterior state paths at `par`, summed on the device (definitions: DESIGN.md §3.13).  Draws, state rows and
 * position columns are exactly those of ssde_path_stats: draw q is draw number draw0 + q of the stream `seed`, the path
 * ssde_smooth_draws returns; a lattice-padded handle samples its padded rows, which take part in nothing.
 *   grid     the cell of a position p is ix = floor((p_1 - x0) / dx), iy = floor((p_2 - y0) / dy) (IEEE divisions); it is inside the
 *            grid when 0 <= ix < nx and 0 <= iy < ny.  For n_dim = 1, ny must be 1 and y0, dy are neither read nor validated.  A
 *            non-finite coordinate is outside.
 *   occ      [nx x ny x n_groups], element (ix, iy, g) at ix + nx * (iy + ny * g): the sum of w_j over the n_draws draws, the tracks t
 *            with group[t] == g and their state rows j whose position lies in the cell.
 *   outside  [n_groups] or NULL: the same sum over the state rows that fall in no cell, so that per group the sum of occ plus outside
 *            is exactly n_draws times the sum of w_j over the group's state rows.
 *   group    [n_tracks] host memory, indexed by the ID segment's ordinal; -1: the track takes part in nothing.  NULL: every track is in
 *            group 0 (n_groups must be 1).
 *   weight   [n] host memory, indexed by the caller's row, or NULL for w_j = 1.  Validated: every entry finite and >= 0.
 * The sums are taken in fixed point.  With wmax the largest weight (1 for NULL), frexp(wmax) = (m, k) and b the bit length of
 * n * n_draws (n the rows of the whole handle's data), the quantum is 2^e, e = max(k + b - 52, -1074); w_j enters as the integer
 * nearbyint(ldexp(w_j, -e)) (ties to even), the integers are summed as unsigned 64-bit numbers, and an output is
 * ldexp((double)sum, e): every possible sum is below 2^52, so that conversion is exact.  wmax == 0 gives 0 everywhere.  Hence
 *   1. the result is bitwise independent of SSDE_OPT_SMOOTH_BUDGET_MB, of the devices, of the kernel form and of repeated calls;
 *   2. draw ranges add up bitwise over calls whenever the weights are whole numbers of both calls' quanta (NULL weights, dyadic dt);
 *   3. otherwise draw ranges add up to within hits * 2^(e - 1) per cell, e the coarser call's.
 * flags: SSDE_OCC_FORCE_GLOBAL runs every wavefront group in the global form (each lane adds straight into HBM) instead of the
 * LDS-tile form; the numbers are the same.  ssde_last_occupancy_form tells which ran.
 * SSDE_ERR_ARG for NULL h / par / grid / occ; n_draws < 1, draw0 < 0, draw0 + n_draws >= 2^28; nx or ny outside 1 ... 4096; ny != 1
 * for n_dim = 1; dx (and dy for n_dim = 2) not finite or <= 0, x0 / y0 not finite; n_groups < 1 or nx * ny * n_groups > 2^28; group ==
 * NULL with n_groups != 1, a group entry outside -1 ... n_groups - 1; a weight that is negative or not finite; an unknown flag.
 * SSDE_ERR_MODEL exactly where ssde_path_stats gives it.  Every check runs before anything touches the device.  Multi-device handles
 * are served.  Leaves the memo, the window state, the TV records, n_evals / n_memo_hits and every later ssde_eval / ssde_smooth /
 * ssde_smooth_draws / ssde_predict / ssde_path_stats result as they were. */
typedef struct ssde_occ_grid { double x0, dx, y0, dy; int32_t nx, ny; } ssde_occ_grid;
#define SSDE_OCC_FORCE_GLOBAL 1u
int ssde_path_occupancy(ssde_handle *h, const double *par, int32_t n_par_full, uint64_t seed, int64_t draw0, int32_t n_draws,
                        const ssde_occ_grid *grid, const double *weight, const int32_t *group, int32_t n_groups,
                        double *occ, double *outside, uint32_t flags);
/* The kernel forms of the handle's last ssde_path_occupancy: 0 none yet, 1 every wavefront group ran the LDS-tile form, 2 every group
 * the global form, 3 both ran.  A multi-device parent reports its first shard.  NULL gives -1. */
int ssde_last_occupancy_form(const ssde_handle *h);

/* Occupancy grids of posterior state paths refined between the fixes (definitions: DESIGN.md §3.15).  The grid, occ, outside, group,
 * weight, the draws, the position columns, the cell rule, the validation of the weights, SSDE_OCC_FORCE_GLOBAL and the quantum (the
 * same e: b is the bit length of n * n_draws, n the whole handle's caller rows) are ssde_path_occupancy's.  What is new is WHERE a
 * state row's weight goes:
 *   1. Slots and sub-steps.  A slot is a state row s of a track in the handle's resident layout (on a lattice-padded handle: a
 *      lattice row) that is not the track's last state row; Delta_s is the interval the handle holds for it (the lattice step on a
 *      lattice-padded handle) and m_s = min(SSDE_OCC_MAX_SUB, max(1, ceil(Delta_s / max_step))), an IEEE division, computed once on
 *      the host from the handle's data; max_step = +inf gives m = 1.  A track's last state row has one point, its own.
 *   2. Points.  A slot's points are the draw's state at row s and, for k = 1 .. m_s - 1, its state at the offset
 *      delta_k = (k * Delta_s) / m_s (the product first, then the quotient, in double): the state ssde_predict_draws returns for a
 *      call whose queries in that slot are exactly those m_s - 1 offsets (delta_k has rank k - 1, each point is drawn given the one
 *      below it, row s's parameters apply).  The two calls describe THE SAME PATH.
 *   3. Weights.  A caller's state row j with W_j quanta owns the N_j points of every resident slot from its own up to, not
 *      including, the next caller row's slot (one slot on an unpadded handle, the padded rows' points included on a lattice
 *      handle).  Every point gets W_j div N_j quanta and the row's own point W_j mod N_j more, so per group the sum of occ plus
 *      outside is still EXACTLY n_draws times the sum of w_j over the group's state rows, and with every m = 1 on an unpadded
 *      handle the result is bitwise ssde_path_occupancy's.
 *   4. Outside.  A point with a non-finite position coordinate is outside: a row that rejected its update (every inner point of its
 *      slot), a NaN end, a non-positive pivot of chol(S) (the larger offsets of that slot and draw only, as in ssde_predict_draws).
 *   5. The result is bitwise independent of SSDE_OPT_SMOOTH_BUDGET_MB, the devices, the kernel form, how the draws are batched
 *      inside a call and repeated calls.  Over draw RANGES cut over calls the guarantee is WEAKER than ssde_path_occupancy's rules 2
 *      and 3: a point's amount is the floor W_j div N_j, and the quantum depends on n_draws.  Two calls' ranges add up bitwise to
 *      the whole range's call only where every W_j is a whole multiple of N_j in the quanta of all the calls involved (w_j = N_j
 *      times a dyadic number, for instance; NULL weights and dyadic dt do NOT suffice once an m exceeds 1); otherwise they add up
 *      to within hits * 3 * N_max * 2^e per cell, hits the points of all the draws in the cell, N_max the largest N_j and e the
 *      coarsest call's.  With every m = 1 on an unpadded handle rules 2 and 3 of ssde_path_occupancy hold as they stand.
 * The call always runs its own kernels, also when every m is 1.  ssde_last_occupancy_form reports this call's forms too.
 * SSDE_ERR_ARG for every case of ssde_path_occupancy; max_step NaN or <= 0 (+inf is allowed); a handle with 2^32 or more tracks (the
 * bridge deviates' counter holds the ordinal's low word).  SSDE_ERR_MODEL exactly where ssde_path_occupancy gives it.  Every check
 * runs before anything touches the device.  Multi-device handles are served.  Leaves the memo, the window state, the TV records,
 * n_evals / n_memo_hits and every later result of every other call as they were. */
#define SSDE_OCC_MAX_SUB 64
int ssde_path_occupancy_fine(ssde_handle *h, const double *par, int32_t n_par_full, uint64_t seed, int64_t draw0, int32_t n_draws,
                             const ssde_occ_grid *grid, double max_step, const double *weight, const int32_t *group, int32_t n_groups,
                             double *occ, double *outside, uint32_t flags);
/* of the handle's last ssde_path_occupancy_fine: path points per draw that carried weight (the sum of N_j over the state rows of the
 * tracks that take part), and intervals of those tracks whose m was cut to the cap.  Either pointer may be NULL. */
int ssde_last_occupancy_points(const ssde_handle *h, int64_t *n_points, int64_t *n_capped);

/* Proximity of posterior paths between tracks (definitions: DESIGN.md §3.16).  Point i compares side A, the query (qa_row[i],
 * qa_off[i]), with side B, the query (qb_row[i], qb_off[i]); both are queries of ssde_predict_draws: a caller's row and an offset >= 0
 * past its stamp.  Pair p owns the points pair_ptr[p] .. pair_ptr[p + 1] - 1: a CSR list with pair_ptr[0] == 0, non-decreasing,
 * n_point = pair_ptr[n_pairs].  A pair may be empty.  Nothing requires the two sides to be different tracks or one side to stay on
 * one track: a pair is a set of points; the same track at two times is legal, and so are two identical sides.
 *   1. The states.  For draw number draw0 + q the two states of point i are exactly what ssde_predict_draws returns for ONE call
 *      whose 2 * n_point queries are all the A queries followed by all the B queries: they go through one plan, are jointly
 *      distributed inside an interval and lie on the path every other call uses for that seed and draw number.  Tracks are
 *      independent given par, so draw q of two tracks at one clock time is a joint draw.  The position columns are ssde_path_stats'
 *      and the distance is its Euclidean one (|difference| for n_dim = 1).
 *   2. stats [n_pairs x n_stat x n_draws], n_stat = 2 + n_radii, element (p, k, q) at p + n_pairs * (k + n_stat * q):
 *      k = 0 the smallest distance over the pair's points; k = 1 the index inside the pair (0-based, as a double) of the first point
 *      that attains it (a tie gives the smallest index); k = 2 + r the sum of w_i over the pair's points with dist_i <= radii[r].
 *   3. Fixed-point sums, by ssde_path_occupancy's rule with e taken for wmax (the largest weight; 1 without weights), n_point and
 *      ONE draw: every w_i enters as nearbyint(ldexp(w_i, -e)) quanta, the quanta are summed as unsigned 64-bit integers and the
 *      output is ldexp((double)sum, e).  The quantum does not depend on n_draws, so draw ranges cut over calls give the whole range's
 *      numbers back bitwise.  The minimum, its index and the sums do not depend on the order in which points are combined: the result
 *      is bitwise independent of SSDE_OPT_SMOOTH_BUDGET_MB, of the devices and of repeated calls.  weight: [n_point] in host memory, or
 *      NULL for 1.  wmax == 0 gives 0 in every sum.
 *   4. NaN.  Every statistic of a (pair, draw) is NaN if either side of any of its points has a position that is not finite (as in
 *      ssde_path_stats; a query on a track's first row is such a case), and every statistic of an empty pair is NaN.
 * SSDE_ERR_ARG for NULL h / par / a query array / pair_ptr / stats; n_pairs < 1; a pair_ptr that is not as described, or n_point <
 * 1; a row outside [0, n), an offset that is negative or not finite; n_draws < 1, draw0 < 0, draw0 + n_draws >= 2^28; n_radii outside
 * 0 ... SSDE_PROX_MAX_RADII, radii NULL with n_radii > 0, a radius that is NaN or < 0 (+inf is allowed); a weight that is negative or
 * not finite; flags != 0; the limits of ssde_predict_draws (2^32 tracks, 2^32 distinct offsets in an interval).  SSDE_ERR_MODEL exactly
 * where ssde_path_stats gives it.  Every check runs before anything touches the device.  Lattice-padded handles, PATH_TV handles,
 * row-varying parameters and multi-device handles (a pair may straddle shards) are served.  Leaves the memo, the window state, the TV
 * records, n_evals / n_memo_hits and every later result of every other call as they were. */
#define SSDE_PROX_MAX_RADII 8
int ssde_path_proximity(ssde_handle *h, const double *par, int32_t n_par_full, uint64_t seed, int64_t draw0, int32_t n_draws,
                        const int64_t *qa_row, const double *qa_off, const int64_t *qb_row, const double *qb_off,
                        const int64_t *pair_ptr, int32_t n_pairs, const double *weight,
                        const double *radii, int32_t n_radii, double *stats, uint32_t flags);
/* Of the handle's last ssde_path_proximity: the tiles (every pair is cut into tiles of 256 consecutive points; a tile never spans
 * pairs and an empty pair has none), the most tiles one pair was cut into, the batches of draws, and the route: 1 the positions never
 * left the device, 2 they were gathered from the shards of a multi-device handle.  All zero before any call.  Any pointer may be NULL;
 * SSDE_ERR_ARG for a NULL handle. */
int ssde_last_proximity_plan(const ssde_handle *h, int64_t *n_tiles, int64_t *tiles_max, int32_t *n_batches, int32_t *route);

/* Of the handle's last ssde_hess, where it ran the hyper-dual lanes over time windows (scope 3, ESEAL_SSM excepted): the warm-up rows
 * of the accepted attempt (0: one sequential window per track), the most windows a track was cut into, the attempts it took (a failed
 * hand-over check quadruples the warm-up; the fourth failure, or a warm-up no track holds twice, ends in one sequential window) and
 * the accepted hand-over check.  A sharded or companion-backed handle reports the largest of each over the engines that ran.  All
 * zero before any ssde_hess and after one that ran no windowed pass (direct families, drift coefficients, ESEAL_SSM).  Any pointer
 * may be NULL; SSDE_ERR_ARG for a NULL handle. */
int ssde_last_hess_plan(const ssde_handle *h, int32_t *warm_up, int32_t *windows_max, int32_t *attempts, double *check);

/* Multiply the warm-up overlap of the time windows by `factor` for all later evaluations
 * (factor <= 0: force one sequential window). */
int ssde_widen_windows(ssde_handle *h, int32_t factor);

/* Halve that multiplier again (never below 1).  ssde_eval does this by itself after 32 evaluations accepted at the
 * first try; asynchronous callers that re-evaluate after ssde_widen_windows use this for the same policy.  Every
 * evaluation is checked, so a narrower overlap that does not hold shows in window_check. */
int ssde_relax_windows(ssde_handle *h);

int ssde_info(const ssde_handle *h, ssde_info_t *info);

/* HIP-event duration (ms) of the dominant kernel launch of the last evaluation (== ssde_info().main_kernel_ms, without
 * filling the rest of the structure: cheap enough to be read after every timed step of a benchmark); 0 if unknown. */
double ssde_last_kernel_ms(const ssde_handle *h);

/* The same for the last n evaluations at once: ms[0] = the last one, ms[1] the one before, ... (0 where no stamp exists:
 * more than 64 evaluations ago, or an evaluation replayed from a hipGraph).  Every evaluation stamps its dominant kernel
 * with an event pair of its own, so a caller can time K <= 64 evaluations back to back and read their kernel durations
 * AFTER the timed region (bench.py) instead of querying events between them. */
int ssde_kernel_ms_history(const ssde_handle *h, double *ms, int32_t n);

/* Where the last SYNCHRONOUS ssde_eval spent its time, in milliseconds (single-device handle; valid after an evaluation made with
 * SSDE_OPT_KERNEL_STAMPS on, zeros otherwise).  GPU-side phases come from HIP events on the evaluation's stream:
 *   ms[0] host_total   wall time of the call
 *   ms[1] host_enqueue ... of which: planning, gain table, launches (the host side until everything was enqueued)
 *   ms[2] gpu_pre      first operation of the evaluation on the stream -> the dominant kernel's begin (uploads, launch gap)
 *   ms[3] kernel       the dominant kernel (== ssde_last_kernel_ms)
 *   ms[4] finalize     its end -> the end of the finalising launch (hand-over checks + fixed-order sums)
 *   ms[5] allreduce    ... -> the end of the ncclAllReduce behind it (0 without a communicator): wire time AND the wait for
 *                      the slowest rank
 *   ms[6] readback     host_total minus everything above (the blocking copy and what the runtime adds around it)
 *   ms[7] reserved (0)
 * Returns SSDE_ERR_ARG for a multi-device parent.  A measurement hook: bench.py gathers it per rank. */
int ssde_last_phase_ms(ssde_handle *h, double ms[8]);

/* Drop the memoised last result: the next ssde_eval runs on the device whatever its argument (determinism checks). */
int ssde_forget(ssde_handle *h);

/* fn / gr of the MARGINAL negative log-likelihood: coeff_re integrated out by the Laplace approximation, which is
 * what tmb_obj$fn / tmb_obj$gr are when SDE$setup passes random = "coeff_re" (R/sde.R:510-525, 656-658):
 *     f(theta) = g(theta, u^) + 1/2 log det H_uu(theta, u^) - n_u/2 log(2 pi),   u^ = argmin_u g(theta, u),
 * g = ssde_eval's joint penalised nllk, u = the coeff_re entries that are not fixed, theta = every other free entry
 * (log_sigma_obs, coeff_fe, log_lambda, log_decay).
 *   par     [n_par_full] IN/OUT: outer parameters and the starting values of coeff_re (warm start); on return the
 *           coeff_re entries hold u^ (TMB's par.random / env$last.par)
 *   order   0: *value;  1: also grad[n_par_full] = df/dtheta (zeros at coeff_re and at fixed entries)
 *   hess_uu NULL or [n_u x n_u] column-major: H_uu at u^ (the random-effect block of sdreport's jointPrecision)
 * Direct families BM / OU / BM_t / CIR: H_uu and H_u,theta are EXACT (ssde_hess), only 1/2 d log det H_uu / dtheta is a central
 * difference -- of exact Hessians, along the implicit-function tangent of u^.  Elsewhere H_uu comes from central
 * differences of the device gradient.  The inner problem is solved by Newton iterations; the gradient is the exact
 * dg/dtheta at u^ plus that log-determinant term (ssde_laplace.hip).  A joint nllk that has no minimum in u gives
 * *value = +Inf (a rejected step; `par` is then left untouched). */
typedef struct ssde_laplace_opts {
    double hess_step;      /* relative step of the Hessian differences   (<= 0: 1e-4) */
    double fd_step;        /* relative step of the log-determinant term  (<= 0: 1e-4) */
    double newton_tol;     /* inner convergence: largest step component  (<= 0: 1e-8) */
    int32_t max_newton;    /* inner iterations                           (<= 0: 30)   */
    int32_t reserved;
} ssde_laplace_opts;
int ssde_laplace_eval(ssde_handle *h, double *par, int32_t n_par_full, int32_t order, double *value, double *grad,
                      double *hess_uu, const ssde_laplace_opts *opts);

/* Second derivatives of the joint penalised nllk (ssde_eval's value) over the parameter entries idx[0 .. n_idx):
 * hess [n_idx x n_idx] column-major.  EXACT -- no differencing -- for the direct families "BM", "OU", "BM_t" and "CIR"
 * (tr_dens.hpp:32-67) with resident design columns (decaying ones and log_decay included): the SDE parameters are linear in coeff_fe /
 * coeff_re, so the data term's Hessian is X' D X with a closed-form per-row D, and the penalty is exp(log_lambda) times a
 * quadratic form (nllk_sde.hpp:91-124); and for the state-space families CTCRW / OU_SSM / BM_SSM on handles whose rows the
 * lane = direction filter holds (row-varying coefficients, ESEAL_SSM, or any handle created with SSDE_FLAG_EXACT_HESS):
 * second-order forward mode through the filter.  ssde_info.exact_hess_scope says which entries a handle covers.  idx may name coeff_fe,
 * coeff_re and log_lambda entries, fixed or free.  Where the scope does not cover idx (exact_hess_scope 0 or 1) the
 * call returns SSDE_ERR_MODEL: difference ssde_eval's gradient there, as ssde_laplace_eval does.  Works on single-device,
 * multi-device and communicator handles (the shards' / ranks' Hessians are summed). */
int ssde_hess(ssde_handle *h, const double *par, int32_t n_par_full, const int32_t *idx, int32_t n_idx, double *hess);

/* One process per GPU (torchrun / mpirun style hosts).  Rank 0 calls ssde_comm_unique_id (128 bytes, an
 * ncclUniqueId), the host ships it to the other ranks by its own means, then EVERY rank calls ssde_comm_init_rank
 * on its own single-device handle (collective call).  From then on ssde_eval / ssde_eval_device sum
 * [nllk_data, grad..., window_check] over the ranks with one ncclAllReduce (RCCL over xGMI) on the evaluation's
 * stream before anything is read back, so every rank returns the batch value; the penalty is added once, after
 * the sum.  Window retries are decided on the reduced check value, i.e. identically on every rank. */
#define SSDE_COMM_ID_BYTES 128
int ssde_comm_unique_id(void *id128);
int ssde_comm_init_rank(ssde_handle *h, int32_t n_ranks, int32_t rank, const void *id128);

/* Per-handle options.
 *   SSDE_OPT_KERNEL_STAMPS (default 1): every evaluation stamps its dominant kernel with a HIP event pair
 *       (ssde_last_kernel_ms / ssde_kernel_ms_history).  0 = plain launches: a few microseconds less per evaluation,
 *       which is what a fitting host wants; measurement passes switch it back on.
 *   SSDE_OPT_COMM_DEFER (default 0): 1 = ssde_eval_device leaves this rank's PARTIAL [nllk, grad..., check] in the caller's
 *       buffer and the caller sums it over the ranks itself (ssde_comm_allreduce) -- a host that evaluates several handles
 *       side by side packs their result vectors and issues one collective for all of them instead of one per handle on
 *       as many streams.  ssde_eval ignores it.
 *   SSDE_OPT_SMOOTH_BUDGET_MB (default 0 = a quarter of the device memory free when ssde_smooth is called): the largest record
 *       buffer ssde_smooth allocates, in MiB (one wavefront group always goes, whatever the cap).
 *   SSDE_OPT_LAG_EARLY: 1 = an evaluation on the lag-statistics path (CTCRW) may cut the bulk at the end of its covariance transient
 *       instead of at row 256: the streamed head is then one window per track, and the rows past the cut come from
 *       statistics built for that cut (every multiple of 16 from 32 to 128).  Setting it builds those statistics, synchronously, on a
 *       handle that holds the late ones and not yet these; a handle without lag statistics ignores it.  0 = the cut at row 256 only.
 *       Default: 1 exactly when ssde_create built the early cuts -- where its dispatch rule itself built the lag statistics and the response
 *       has two coordinates --, else 0 (with one coordinate the head of the late cut is the faster launch: DESIGN.md §3.3d).
 *   SSDE_OPT_LAG_HEAD_HOST: 1 = a synchronous single-device ssde_eval whose bulk is cut early forms the head's accumulators on the host,
 *       from Gram statistics of the first 128 rows of every track, and launches nothing (ssde_last_head_form).  Setting it
 *       builds those statistics, synchronously, on a handle that holds lag statistics and not yet these (CTCRW, two coordinates, every
 *       track at least 128 rows; any other handle ignores it).  0 = the head stays a launch.  Every other caller (ssde_eval_device, stamped
 *       evaluations, shards, a communicator) keeps the launch whatever the option says.  Default: 1 exactly when ssde_create built
 *       those statistics -- where it built the early cuts by its own dispatch rule --, else 0. */
enum { SSDE_OPT_KERNEL_STAMPS = 1, SSDE_OPT_COMM_DEFER = 2, SSDE_OPT_SMOOTH_BUDGET_MB = 3, SSDE_OPT_LAG_EARLY = 4, SSDE_OPT_LAG_HEAD_HOST = 5 };
int ssde_set_option(ssde_handle *h, int32_t option, int64_t value);

/* Sum buf_dev[0 .. count) (doubles, HBM) over the ranks of the communicator `h` joined, in place, on `stream` (enqueue only:
 * one ncclAllReduce).  SSDE_ERR_ARG if the handle has joined none. */
int ssde_comm_allreduce(ssde_handle *h, double *buf_dev, int64_t count, void *stream);

/* Synthetic track batches in HBM: the exact-transition simulator of SDE$simulate (R/sde.R:1434-1478: BM increments,
 * OU transition density, CTCRW joint (velocity, position) transition with CTCRW_cov of R/utility.R:188-196), one
 * wavefront lane per track, plus N(0, sigma_obs^2) observation error for the state-space families (BM_SSM, OU_SSM,
 * CTCRW).  Every normal deviate is a pure function of (seed, GLOBAL track index, row, dimension) -- Philox4x32-10
 * counters + Box-Muller --, so tracks [track0, track0 + n_tracks) of a batch are the same numbers whichever process
 * generates them: ranks of a multi-GPU run each generate their own shard of ONE batch.
 *   obs_dev   [n_rows x n_dim] column-major (HBM), the reference's DATA_MATRIX(obs) layout
 *   id_dev    NULL or [n_rows]: the global track index of every row (as doubles, like TMB's factor codes)
 *   times_dev NULL or [n_rows]: (row_offset + i + 1) * dt -- increasing over the whole batch (inst/example.R:17)
 * Rows: track m (local index) owns rows [m * n_steps, (m + 1) * n_steps), or [row0[m], row0[m + 1]) when the HBM
 * array row0 [n_tracks + 1] is given (ragged tracks; n_steps is then the longest track).  Enqueues on `stream` and
 * returns; ssde_last_error(NULL) holds the message of a failure. */
typedef struct ssde_sim_desc {
    int32_t  abi_version;     /* SSDE_ABI_VERSION */
    int32_t  model;           /* SSDE_MODEL_BM, _OU, _BM_SSM, _OU_SSM, _CTCRW (R/sde.R:1434-1478; the others: SSDE_ERR_MODEL) */
    int32_t  n_dim;           /* response columns, 1..8 */
    int32_t  n_steps;         /* rows per track (the longest track when row0 is given) */
    int64_t  track0;          /* global index of the first track generated by this call */
    int64_t  n_tracks;        /* tracks generated by this call */
    const int64_t *row0;      /* NULL, or HBM [n_tracks + 1] first local row of every track */
    int64_t  n_rows;          /* rows of the local long format (column stride of obs_dev) */
    int64_t  row_offset;      /* global index of local row 0 (only `times` uses it) */
    double   mu[8], z0[8];    /* drift / long-term mean and first value per dimension (simulate's z0, R/sde.R:1388) */
    double   tau, nu;         /* CTCRW (beta = 1 / tau, sigma = 2 nu / sqrt(pi tau): R/sde.R:1455-1458); OU: tau */
    double   kappa;           /* OU variance parameter (R/sde.R:1445) */
    double   sigma;           /* BM diffusion (R/sde.R:1437) */
    double   sigma_obs;       /* sd of the observation error (state-space families; 0 = none) */
    double   dt;              /* the regular time step */
    uint64_t seed;
    int32_t  device;          /* HIP device ordinal, -1 = current device */
    int32_t  reserved;
} ssde_sim_desc;
int ssde_simulate(const ssde_sim_desc *desc, double *id_dev, double *times_dev, double *obs_dev, void *stream);

/* Confidence bands of the SDE parameters (SDE$post_par / CI_pointwise / CI_simultaneous, R/sde.R:941-1180) from a table of
 * posterior coefficient draws, reduced on the device: the n x n_post matrix of a parameter's draws is never built.
 * A descriptor call like ssde_simulate: no handle.
 *   n rows and n_par parameters.  Parameter j has a fixed-effect block x_fe[j] (n x ncol_fe[j], column-major; NULL with
 *   ncol_fe[j] == 1 = a column of ones) and a random-effect block x_re[j] (n x ncol_re[j], NULL for 0 columns): the block
 *   convention of ssde_desc.  K_j = ncol_fe[j] + ncol_re[j], n_coef = sum_j K_j.
 *   coeff     [(1 + n_post) x n_coef] row-major, host memory: row 0 the point estimate, rows 1 .. n_post the draws; parameter j's
 *             K_j entries contiguous, fixed effects first
 *   link[j]   0 identity, 1 log.  level in (0, 1), alpha = (1 - level) / 2; z = the caller's qnorm((1 + level) / 2).
 * lp(i, j, k) = sum_c X_j[i, c] coeff[k, off_j + c], summed in column order (fixed-effect columns, then random-effect columns) as
 * one fma chain.  Q(x, p) is R's type-7 quantile of the sorted x[0 .. m): h = (m - 1) p, lo = floor(h), hi = min(lo + 1, m - 1),
 * Q = x[lo] + (h - lo)(x[hi] - x[lo]) (x[lo] itself where x[hi] == x[lo]); equal values count with their multiplicity.
 * Outputs, each n x n_par column-major, each may be NULL:
 *   est               lp(i, j, 0), through the inverse link when resp != 0
 *   pw_low, pw_upp    Q at alpha and 1 - alpha of {g(lp(i, j, k))}, k = 1 .. n_post; g the inverse link when resp != 0 (applied to
 *                     the two order statistics before the interpolation), else the identity
 *   sim_low, sim_upp  g(lp(i, j, 0) -+ crit[j] se(i, j)) with se = (lp(i, j, 0) - Q_lp(alpha)) / z on the link scale
 * and, always host memory, may be NULL:
 *   max_dev  [n_par x n_post] row-major: max_i |dev(i, j, k) / se(i, j)|, dev the dot product with coeff[k] - coeff[0]; 0 / 0 counts
 *            as 0, x / 0 = inf is kept (R/sde.R:1155-1159)
 *   crit     [n_par]: Q(max_dev[j, .], level), NaN -> 0
 * ONE table serves se and the deviations; the reference draws twice inside CI_simultaneous (R/sde.R:1112, 1119).
 * Where any lp(i, j, k), k = 0 .. n_post, is not finite every output of (i, j) is NaN and the row adds nothing to max_dev.
 * Each tail needs floor((n_post - 1) alpha) + 2 order statistics (the upper one the mirror count); both must be <=
 * SSDE_BANDS_MAX_TAIL.  With sim_low, sim_upp, crit and max_dev all NULL only the first pass runs.
 * Host blocks are uploaded in chunks of whole rows under budget_mb MiB (0 = a quarter of the free device memory); the result is
 * bitwise independent of the chunking.  Synchronous; one device.
 * SSDE_ERR_ARG -- before anything touches the device; the text through ssde_last_error(NULL) -- for a NULL desc, every output NULL,
 * a wrong abi_version, n < 1, n_par outside 1 .. SSDE_BANDS_MAX_PAR, a K_j outside 1 .. SSDE_BANDS_MAX_COLS, a NULL block that is
 * not the intercept case, a link other than 0 / 1, n_post < 2, level outside (0, 1), z not finite or <= 0, a tail over the cap, a
 * coeff entry that is not finite, an unknown flag. */
#define SSDE_BANDS_MAX_TAIL 64
#define SSDE_BANDS_MAX_COLS 64     /* K_j */
#define SSDE_BANDS_MAX_PAR  16     /* n_par */
#define SSDE_BANDS_DEVICE_DATA 1u  /* x_fe / x_re blocks are HBM pointers on `device` */
#define SSDE_BANDS_DEVICE_OUT  2u  /* the n x n_par outputs are HBM pointers; crit / max_dev are always host */
typedef struct ssde_bands_desc {
    int32_t  abi_version;     /* SSDE_ABI_VERSION */
    int32_t  n_par;
    int64_t  n;
    const int32_t *ncol_fe;
    const double *const *x_fe;
    const int32_t *ncol_re;
    const double *const *x_re;
    const uint8_t *link;
    const double *coeff;
    int32_t  n_post;
    int32_t  resp;
    double   level;
    double   z;
    int32_t  device;          /* HIP device ordinal, -1 = current device */
    int32_t  budget_mb;
    uint32_t flags;
    uint32_t reserved;
} ssde_bands_desc;
int ssde_par_bands(const ssde_bands_desc *d, double *est, double *pw_low, double *pw_upp,
                   double *sim_low, double *sim_upp, double *crit, double *max_dev);

/* Replicate data sets simulated on the data's own rows, and their check statistics (SDE$simulate / SDE$check_post,
 * R/sde.R:1395-1508, 1259-1306).  A descriptor call like ssde_par_bands: no handle, synchronous, one device.
 *   model     BM, OU, CTCRW, BM_SSM, OU_SSM; every other model is SSDE_ERR_MODEL with the reference's message (R/sde.R:1496) -- CIR
 *             too: the reference's CIR branch cannot run (an undefined `n` at R/sde.R:1487)
 *   n rows in n_tracks ID segments: track t owns rows [row0[t], row0[t + 1]), row0 [n_tracks + 1] in host memory, row0[0] == 0,
 *   non-decreasing, row0[n_tracks] == n; an empty track produces nothing.  times [n], host memory; inside a track every step
 *   dt_i = times[i] - times[i - 1] is finite and > 0.
 *   Parameter blocks as ssde_bands_desc's (a NULL fixed-effect block with ncol_fe == 1 = a column of ones; device pointers with
 *   SSDE_SIMROWS_DEVICE_DATA), the same fma chain.  The parameters are mu_1 .. mu_d, then sigma (BM, BM_SSM: n_par = n_dim + 1), tau
 *   and kappa (OU, OU_SSM) or tau and nu (CTCRW: n_par = n_dim + 2); parameter = g(lp), g = exp where link[j] == 1.
 *   coeff     [n_coeff_rows x n_coef] row-major, host, n_coeff_rows 1 or n_rep, every entry finite: replicate k of the call uses row k
 *             (row 0 with one row: the reference's posterior = FALSE); n_coef = sum_j K_j <= SSDE_SIMROWS_MAX_COEF
 *   sigma_obs NULL or [n_coeff_rows], host, finite and >= 0: the sd of an N(0, sigma^2) error added to every written observation of
 *             the replicate, whatever the model (the reference's simulator has none)
 *   z0[c]     the first value of every track in column c (finite); a CTCRW velocity starts at 0 (R/sde.R:1451)
 *   seed, rep0, n_rep: replicate k is replicate NUMBER rep0 + k of the stream `seed`; rep0 >= 0, n_rep >= 1, rep0 + n_rep < 2^28;
 *             n_tracks < 2^32 and every track shorter than 2^32 rows
 *   thr       [n_thr] host, n_thr in 0 .. SSDE_SIMROWS_MAX_THR, each >= 0 (+inf allowed)
 * The transition into row i of a track uses the parameters of row i - 1 and dt_i (sub_par[i - 1, ], R/sde.R:1434-1478); the exact
 * forms -- expm1 for 1 - e, a series for the CTCRW position variance at small dt / tau, every fma -- are csrc/ssde_simrows.hpp's.
 * Deviates: Philox4x32-10 + Box-Muller as in ssde_simulate with the counter (row position in the track, track ordinal, replicate
 * number, stream) and the key (seed low, seed high); stream 2c gives (transition, error) of column c, for a CTCRW (na, nb) and the
 * first deviate of stream 2c + 1 the error.  A replicate is a pure function of seed, track ordinal, row position, replicate number,
 * its coefficient row and its sigma_obs: not of n_rep, of rep0's cut over calls, of budget_mb, of the outputs asked for or of the
 * other tracks.
 * Outputs (either may be NULL, not both):
 *   obs_rep   [n x n_dim x n_rep], element (i, c, k) at i + n (c + n_dim k); host memory, or HBM with SSDE_SIMROWS_DEVICE_OUT
 *   stats     [n_tracks x n_stat x n_rep], element (t, s, k) at t + n_tracks (s + n_stat k), n_stat = 3 n_dim + 2 + n_thr; always
 *             host memory.  From the written observations y (error included), D_{i,c} = y_{i,c} - y_{i-1,c} over the track's rows
 *             from its second on, in row order: s = 3c sum D, 3c + 1 sum D^2, 3c + 2 sum D_i D_{i-1} (rows with both increments in
 *             the track); then with L_i = sqrt(sum_c D_{i,c}^2): sum L, max L, and per threshold the number of i with L_i <= thr[r]
 *             (a double).  NaN in every statistic of a track with fewer than two rows and of a (track, replicate) with a y or a
 *             parameter of a used row that is not finite.
 * Replicates run in batches under budget_mb MiB of staged outputs (0 = a quarter of the free device memory); both outputs are bitwise
 * independent of the batching.
 * SSDE_ERR_ARG -- before anything touches the device; the text through ssde_last_error with a NULL handle -- for every constraint
 * above, NULL pointers, a wrong abi_version, both outputs NULL, an n_par or n_coef that does not fit the model and the blocks, a
 * K_j outside 1 .. SSDE_BANDS_MAX_COLS, a link other than 0 / 1, an unknown flag. */
#define SSDE_SIMROWS_MAX_THR  8
#define SSDE_SIMROWS_MAX_COEF 128   /* n_coef: 64 lanes' rows are 64 KiB of LDS */
#define SSDE_SIMROWS_DEVICE_DATA 1u /* x_fe / x_re blocks are HBM pointers on `device` */
#define SSDE_SIMROWS_DEVICE_OUT  2u /* obs_rep is an HBM pointer on `device` */
typedef struct ssde_simrows_desc {
    int32_t  abi_version;     /* SSDE_ABI_VERSION */
    int32_t  device;          /* HIP device ordinal, -1 = current device */
    int32_t  budget_mb;
    uint32_t flags;
    uint32_t reserved;
    int32_t  model;           /* SSDE_MODEL_* */
    int32_t  n_dim;
    int32_t  n_par;
    int64_t  n;
    int64_t  n_tracks;
    const int64_t *row0;
    const double *times;
    const int32_t *ncol_fe;
    const double *const *x_fe;
    const int32_t *ncol_re;
    const double *const *x_re;
    const uint8_t *link;
    const double *coeff;
    int32_t  n_coeff_rows;
    int32_t  n_coef;
    const double *sigma_obs;
    double   z0[8];
    uint64_t seed;
    int64_t  rep0;
    int64_t  n_rep;
    const double *thr;
    int32_t  n_thr;
    int32_t  reserved2;
} ssde_simrows_desc;
int ssde_simulate_rows(const ssde_simrows_desc *d, double *obs_rep, double *stats);

void ssde_destroy(ssde_handle *h);

/* Message of the last failure on this handle (or of the last failed ssde_create when h == NULL). */
const char *ssde_last_error(const ssde_handle *h);

int ssde_abi_version(void);
/* The lag statistics ssde_create builds for a stationary batch, computed on the host track by track: the reference
   the device pass is checked against (through ssde_lagstats_read).  y: the tracks' rows one track after the other, rows[k] rows of d doubles each (row-major;
   row t of a track here is its tiled row t); M: n_taps x n_taps doubles, s: 2 x n_taps, n_bulk: one double.  With y == NULL only
   *n_taps and *first_row (the bulk's first row) are written.  Returns SSDE_OK, or SSDE_ERR_ARG for d outside 1..2. */
int ssde_lagstats_host(const double *y, const int64_t *rows, int64_t n_tracks, int d, double *M, double *s, double *n_bulk,
                       int32_t *n_taps, int32_t *first_row);
/* The lag statistics a handle built at create, read back from the device (M: n_taps x n_taps, s: 2 x n_taps, n_bulk: one double; the
   sizes of ssde_lagstats_host).  SSDE_ERR_ARG when the handle holds none (the dispatch rule did not build them, or a multi-device
   parent: ask its shards). */
int ssde_lagstats_read(const ssde_handle *h, double *M, double *s, double *n_bulk);
/* The bulk's forms of ONE evaluation, on the host: what an evaluation on the lag-statistics path computes from M, s and n_bulk
   (ssde_lagstats_host / ssde_lagstats_read) before its reducing launch, without a device.  CTCRW on a regular
   grid of step dt; theta = (log sigma_obs, mu_1 .. mu_d, log tau, log nu); p0 = (p11, p12, p22) the covariance recursion starts
   from, or NULL; K = the cut (16 .. n_taps - 1; the check's cut is K - 16); mask = the gradient directions wanted (1: sigma_obs,
   2: mu, 4: tau, 8: nu; < 0: all).  taps: 2 x n_taps doubles, the impulse responses of u and of r -- written (zero beyond K) when
   taps_given == 0, read as they are when taps_given != 0 (entries beyond K are never read).
   raw: 2 x 6 doubles, S, C_1, C_2, C_3, su_1, su_2 of the cut K and then of the cut K - 16; acc: the 4 + d accumulators
   [value | sigma_obs | mu_1 .. mu_d | tau | nu] of the cut K; chk: the largest difference between the raw sums of the two cuts,
   relative to max(|sum|, sqrt(|S| n_bulk)).  SSDE_ERR_ARG: a NULL pointer, d outside 1..2, K out of range, or a theta without
   a stationary regime. */
int ssde_lagforms_host(const double *M, const double *s, double n_bulk, int32_t d, const double *theta, double dt, const double *p0,
                       int32_t K, int32_t mask, int32_t taps_given, double *taps, double *raw, double *acc, double *chk);
/* ssde_lagforms_host on one build of its sums: isa 0 the baseline instruction set, 1 the AVX2 build (SSDE_ERR_ARG on a host without
   it, and for any other isa).  The two give the same bits; ssde_lagforms_host -- and an evaluation -- runs the wide one where the
   host has it. */
int ssde_lagforms_host_isa(int32_t isa, const double *M, const double *s, double n_bulk, int32_t d, const double *theta, double dt,
                           const double *p0, int32_t K, int32_t mask, int32_t taps_given, double *taps, double *raw, double *acc,
                           double *chk);
/* The same three for every model the lag-statistics path serves (SSDE_MODEL_CTCRW, SSDE_MODEL_OU_SSM, SSDE_MODEL_BM_SSM; DESIGN.md
   §3.3d).  CTCRW and BM_SSM take the statistics of the INCREMENTS y_t - y_{t-1} (ssde_lagstats_host_m returns bitwise what
   ssde_lagstats_host returns for them; ref is ignored); OU_SSM takes those of the LEVELS z_{a,t} = y_{a,t} - ref[a]:
   M_ik = sum z_{t-i} z_{t-k}, s_{a,i} = sum z_{a,t-i} over the bulk rows, with ref[a] (d doubles) a value near the data -- a handle
   keeps the one it chose at create (ssde_lagstats_read_m).  SSDE_ERR_ARG additionally for a model outside the three and, for OU_SSM
   with y != NULL, for ref == NULL. */
int ssde_lagstats_host_m(int32_t model, const double *y, const int64_t *rows, int64_t n_tracks, int d, const double *ref, double *M,
                         double *s, double *n_bulk, int32_t *n_taps, int32_t *first_row);
/* ssde_lagstats_read, and the handle's ref (2 doubles; zeros for a model whose statistics are those of the increments).
   SSDE_ERR_ARG where ssde_lagstats_read gives it, and for ref == NULL. */
int ssde_lagstats_read_m(const ssde_handle *h, double *M, double *s, double *n_bulk, double *ref);
/* ssde_lagforms_host for `model`.  theta: OU_SSM (log sigma_obs, mu_1 .. mu_d, log tau, log kappa), BM_SSM (log sigma_obs,
   mu_1 .. mu_d, log sigma); p0: one double (the variance the covariance recursion starts from) or NULL; ref: what the statistics
   were built with (d doubles, OU_SSM; ignored otherwise); mask bits: 1 sigma_obs, 2 mu, 4 par d, 8 par d + 1 (< 0: all).
   OU_SSM / BM_SSM: taps: 3 x n_taps doubles, the responses of u, A1 and A3 of the stationary lanes (ssde_tf.hpp: BasisScal) to a unit
   impulse in the level (OU_SSM) or a unit increment (BM_SSM), as read by the row's products (A3 == 0 for BM_SSM); raw: 2 x 5 doubles,
   S = sum u^2, S1 = sum u A1, S3 = sum u A3, su_1, su_2 (su_a = sum u_a) of the cut K and then of K - 16; acc, chk as above.
   With model == SSDE_MODEL_CTCRW the call is ssde_lagforms_host (taps 2 x n_taps, raw 2 x 6).  SSDE_ERR_ARG as there, and for a
   model outside the three or (OU_SSM) ref == NULL. */
int ssde_lagforms_host_m(int32_t model, const double *M, const double *s, double n_bulk, const double *ref, int32_t d, const double *theta,
                         double dt, const double *p0, int32_t K, int32_t mask, int32_t taps_given, double *taps, double *raw, double *acc,
                         double *chk);
/* The final sums of an evaluation whose head finished on the host, without a device: what a synchronous
   single-device ssde_eval forms from the records its workgroups stored, in the fixed order of the device's reduction -- bitwise the
   result of the finalize launch.  sums: [n_groups][n_windows][nacc] wave sums; group_chk: [n_groups] hand-over checks; lag_acc: the
   bulk's `nacc` accumulators, the entry after the last one, or NULL (lag_chk is then ignored); add / add_slot: 4 data-independent
   terms and the output slot each is added to (< 0: unused); map: [nacc - 1], accumulator k >= 1 -> output slot, or < 0 (slot 0 is
   accumulator 0).  out: n_out sums, then the check -- the largest of the groups' checks and lag_chk, not-a-number counting as
   infinity.  SSDE_ERR_ARG: a NULL pointer, a count < 1 or a slot >= n_out. */
int ssde_reduce_host(const double *sums, const double *group_chk, int32_t n_groups, int32_t n_windows, int32_t nacc, const double *lag_acc,
                     double lag_chk, const double *add, const int16_t *add_slot, const int16_t *map, int32_t n_out, double *out);
/* ssde_reduce_host where every record but group 0's is zero (the head formed from its statistics: nothing was launched), from that
   record alone: sums0 [n_windows][nacc], chk0 its check; the other arguments as above.  out equals (==) what ssde_reduce_host gives
   on the full array of n_groups records.  SSDE_ERR_ARG as there, and for more than 63 windows. */
int ssde_reduce_host_head(const double *sums0, double chk0, int32_t n_groups, int32_t n_windows, int32_t nacc, const double *lag_acc,
                          double lag_chk, const double *add, const int16_t *add_slot, const int16_t *map, int32_t n_out, double *out);
/* What finished the handle's last evaluation: 0 a finalize launch after the main one, 1 the main launch itself
   (SSDE_FUSED_FINALIZE=1), 2 the host.  A multi-device parent reports its first shard; -1 for NULL. */
int ssde_last_finish_form(const ssde_handle *h);
/* How the main launch of the handle's last evaluation got its gain table: 0 through a pinned slot and a copy on the stream, 1 by value
   in the launch's own argument block (the head of the lag-statistics path with one workgroup per track group, a table short enough
   to fit).  ssde_last_gain_rows: the rows of that table.  A multi-device parent reports its first shard; -1 for NULL. */
int ssde_last_gain_feed(const ssde_handle *h);
int ssde_last_gain_rows(const ssde_handle *h);
/* The lag statistics with the first bulk row `cut`: 256 -- ssde_lagstats_host / ssde_lagstats_read --, or an early cut,
   a multiple of 16 from 32 to 128 (CTCRW: the increments): M_ik = sum_{t = cut}^{n - 1} Dy_{t-i} Dy_{t-k} and s_{a,i} for the lags
   i, k < cut (the other entries are zero), n_bulk = the rows past the cut; a track of n <= cut rows contributes nothing.  The sizes
   are those of ssde_lagstats_host.  ssde_lagstats_host_cut: the host reference, track by track.  ssde_lagstats_read_cut: what the
   handle built on the device (at create, or at ssde_set_option(SSDE_OPT_LAG_EARLY, 1)).  SSDE_ERR_ARG: a NULL pointer, d outside
   1..2, a cut outside the list, a handle that holds no statistics for it (also a multi-device parent, as for ssde_lagstats_read: ask its
   shards). */
int ssde_lagstats_host_cut(const double *y, const int64_t *rows, int64_t n_tracks, int d, int32_t cut, double *M, double *s, double *n_bulk);
int ssde_lagstats_read_cut(const ssde_handle *h, int32_t cut, double *M, double *s, double *n_bulk);
/* The first bulk row of the handle's last evaluation: 256 or an early cut where rows came from the lag statistics, 0 where every row
   was streamed.  A multi-device parent reports its first shard; -1 for NULL. */
int ssde_last_lag_cut(const ssde_handle *h);
/* The Gram statistics of the head's rows (129 components, the count in *n_comp): per track and coordinate
   w = (x0 - y_0, v0, y_1 - y_0, .., y_127 - y_126) of the tiled rows y and the track's a0 row; G = sum w w' [129][129] over tracks and
   coordinates, s [2][129] = sum w per coordinate, n = the tracks.  ssde_headstats_host: the host reference, track by track (y:
   [track][row][coordinate], rows[track] rows each, one track after the other; a0: [track][2 d]); *built = 0 and nothing summed where a
   track has fewer than 128 rows; y == NULL: only *n_comp is written.  ssde_headstats_read: what the handle built on the device (at
   create, or at ssde_set_option(SSDE_OPT_LAG_HEAD_HOST, 1)); SSDE_ERR_ARG where it holds none (also a multi-device parent: ask its shards). */
int ssde_headstats_host(const double *y, const int64_t *rows, const double *a0, int64_t n_tracks, int d, double *G, double *s, double *n,
                        int32_t *built, int32_t *n_comp);
int ssde_headstats_read(const ssde_handle *h, double *G, double *s, double *n);
/* The head's 4 + d accumulators of one evaluation from those statistics, on the host (csrc/ssde_headforms.hpp): CTCRW, d = 2, on a regular
   grid of step dt at theta = (log sigma_obs, mu_1, mu_2, log tau, log nu), rows [0, cut) of every track, cut 1 .. 128; p0: the initial
   covariance (p11, p12, p22) or NULL for (1, 0, 1); mask: DIR_* bits of the directions wanted, < 0 for all; full_probes != 0: every column
   of the response by its own run instead of the shifted-column shortcut (the same numbers: a test).  acc: [6].  gain_out (or NULL):
   [cut][16] the gain row of every head row; trans_out (or NULL): e, t12, b1, b2, de, dt12 of the step; n_probe (or NULL): the columns
   that ran.  SSDE_ERR_ARG: a NULL pointer, d != 2, a cut outside the range, a table row that is not scored. */
int ssde_headforms_host(const double *G, const double *s, double n_tracks, int32_t d, const double *theta, double dt, const double *p0,
                        int32_t cut, int32_t mask, int32_t full_probes, double *acc, double *gain_out, double *trans_out, int32_t *n_probe);
/* The head of the handle's last evaluation: 0 a launch, 1 the statistics on the host (SSDE_OPT_LAG_HEAD_HOST).  A multi-device parent
   reports its first shard; -1 for NULL. */
int ssde_last_head_form(const ssde_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* SSDE_H */
