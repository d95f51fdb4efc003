// ssde_engine_bands.hip -- ssde_par_bands: confidence bands of the SDE parameters from a table of posterior coefficient draws
// (include/ssde.h; kernels k_par_bands.hip, lane math ssde_bands.hpp).  A descriptor call like ssde_simulate: no
// handle, every check before anything touches the device, errors through ssde_last_error(NULL).
//
// The rows are cut into chunks of whole rows so that a chunk's host blocks and host outputs fit the budget; per chunk pass 1 (the
// pointwise outputs, lp0 and se) and pass 2 (the chunk's maxima, max-ed into max_dev) run while the chunk's blocks are on the device.
// lp0 and se are kept for all n rows (2 n n_par doubles beside the budget); after the last chunk max_dev comes home, crit is its
// quantile on the host, and pass 3 runs over the rows again.  Rows are independent and max_dev is a maximum, so nothing depends on
// where the chunks are cut.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/ssde.h"
#include "ssde_bands.hpp"

namespace ssde_engine { extern thread_local std::string g_create_error; }   // what ssde_last_error(NULL) returns
#define g_bands_error ssde_engine::g_create_error

namespace ssde {
hipError_t launch_bands_rows(const BandsArgs& a, hipStream_t s);
hipError_t launch_bands_dev(const BandsArgs& a, hipStream_t s);
hipError_t launch_bands_sim(const BandsArgs& a, hipStream_t s);
}  // namespace ssde

namespace {

// device buffers of one call, freed on every way out
struct BandsBuffers {
    std::vector<void*> p;
    ~BandsBuffers() { for (void* q : p) (void)hipFree(q); }
    hipError_t get(double** out, int64_t doubles) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, (size_t)(doubles > 0 ? doubles : 1) * sizeof(double));
        if (e == hipSuccess) { p.push_back(q); *out = (double*)q; }
        return e;
    }
};

int bands_fail(int status, const char* what, hipError_t e) {
    g_bands_error = std::string("ssde_par_bands: ") + what + (e != hipSuccess ? std::string(": ") + hipGetErrorString(e) : std::string());
    return status;
}

// rows [r0, r0 + nc) of a column-major n x cols block: host -> device (leading dimension nc) or back
hipError_t bands_copy_rows(double* dst, int64_t ld_dst, const double* src, int64_t ld_src, int64_t nc, int cols, hipMemcpyKind kind) {
    for (int c = 0; c < cols; c++) {                     // (one plain copy per column: at most 64 of them, and no pitch to bound)
        const hipError_t e = hipMemcpy(dst + ld_dst * c, src + ld_src * c, (size_t)nc * sizeof(double), kind);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

extern "C" {

int ssde_par_bands(const ssde_bands_desc* d, double* est, double* pw_low, double* pw_upp, double* sim_low, double* sim_upp,
                   double* crit, double* max_dev) {
    using namespace ssde;
#define BANDS_ARG(msg) return bands_fail(SSDE_ERR_ARG, msg, hipSuccess)
    if (!d) BANDS_ARG("NULL descriptor");
    if (!est && !pw_low && !pw_upp && !sim_low && !sim_upp && !crit && !max_dev) BANDS_ARG("every output is NULL");
    if (d->abi_version != SSDE_ABI_VERSION) BANDS_ARG("descriptor built for another ABI version");
    if (d->n < 1) BANDS_ARG("n >= 1 is required");
    if (d->n_par < 1 || d->n_par > SSDE_BANDS_MAX_PAR) BANDS_ARG("n_par outside 1 .. SSDE_BANDS_MAX_PAR");
    if (d->flags & ~(SSDE_BANDS_DEVICE_DATA | SSDE_BANDS_DEVICE_OUT)) BANDS_ARG("unknown flag");
    if (!d->ncol_fe || !d->ncol_re || !d->x_fe || !d->x_re || !d->link || !d->coeff) BANDS_ARG("NULL ncol_fe / ncol_re / x_fe / x_re / link / coeff");
    const int q = d->n_par;
    int n_coef = 0;
    BandsArgs a{};
    for (int j = 0; j < q; j++) {
        const int kf = d->ncol_fe[j], kr = d->ncol_re[j];
        if (kf < 1 || kr < 0 || kf > SSDE_BANDS_MAX_COLS || kr > SSDE_BANDS_MAX_COLS || kf + kr > SSDE_BANDS_MAX_COLS)
            BANDS_ARG("ncol_fe >= 1, ncol_re >= 0 and ncol_fe + ncol_re <= SSDE_BANDS_MAX_COLS are required");
        if (!d->x_fe[j] && kf != 1) BANDS_ARG("a NULL fixed-effect block needs ncol_fe == 1 (the intercept)");
        if (!d->x_re[j] && kr != 0) BANDS_ARG("a NULL random-effect block needs ncol_re == 0");
        if (d->link[j] > 1) BANDS_ARG("link is 0 (identity) or 1 (log)");
        a.kf[j] = kf; a.kr[j] = kr; a.off[j] = n_coef; a.link[j] = d->link[j];
        n_coef += kf + kr;
    }
    if (d->n_post < 2) BANDS_ARG("n_post >= 2 is required");
    if (!(d->level > 0.0 && d->level < 1.0)) BANDS_ARG("level in (0, 1) is required");
    if (!(d->z > 0.0) || !std::isfinite(d->z)) BANDS_ARG("z > 0 and finite is required");
    const BandsPlan plan = bands_plan(d->n_post, d->level);
    if (plan.m_lo > SSDE_BANDS_MAX_TAIL || plan.m_up > SSDE_BANDS_MAX_TAIL)
        BANDS_ARG("the quantile needs more than SSDE_BANDS_MAX_TAIL order statistics of a tail: fewer draws or a higher level");
    const int64_t n_tab = (int64_t)(1 + d->n_post) * n_coef;
    for (int64_t e = 0; e < n_tab; e++)
        if (!std::isfinite(d->coeff[e])) BANDS_ARG("a coeff entry is not finite");
#undef BANDS_ARG
    const bool want_sim = sim_low || sim_upp || crit || max_dev;
    const bool dev_data = d->flags & SSDE_BANDS_DEVICE_DATA, dev_out = d->flags & SSDE_BANDS_DEVICE_OUT;
    const int64_t n = d->n;

    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return bands_fail(SSDE_ERR_NODEVICE, "no HIP device visible: there is no CPU fallback", hipSuccess);
    if (d->device >= 0 && hipSetDevice(d->device) != hipSuccess) return bands_fail(SSDE_ERR_HIP, "hipSetDevice failed", hipSuccess);
    hipError_t e;
#define BANDS_HIP(call, what) do { e = (call); if (e != hipSuccess) return bands_fail(e == hipErrorOutOfMemory ? SSDE_ERR_ALLOC : SSDE_ERR_HIP, what, e); } while (0)

    // the chunk: what one row costs in staged blocks and staged outputs, against the budget
    int64_t row_bytes = 0;
    if (!dev_data)
        for (int j = 0; j < q; j++) row_bytes += (int64_t)sizeof(double) * ((d->x_fe[j] ? a.kf[j] : 0) + a.kr[j]);
    const int n_row_out = (est ? 1 : 0) + (pw_low ? 1 : 0) + (pw_upp ? 1 : 0);
    const int n_stage_out = dev_out ? 0 : std::max(n_row_out, (sim_low ? 1 : 0) + (sim_upp ? 1 : 0));
    row_bytes += (int64_t)sizeof(double) * q * n_stage_out;
    int64_t chunk = n;
    if (row_bytes > 0) {
        int64_t budget = (int64_t)d->budget_mb << 20;
        if (d->budget_mb <= 0) {
            size_t fr = 0, tot = 0;
            BANDS_HIP(hipMemGetInfo(&fr, &tot), "hipMemGetInfo");
            budget = (int64_t)(fr / 4);
        }
        chunk = std::max<int64_t>(1, std::min<int64_t>(n, budget / row_bytes));
    }

    BandsBuffers buf;
    double *d_coeff = nullptr, *d_lp0 = nullptr, *d_se = nullptr, *d_md = nullptr, *d_part = nullptr, *d_x = nullptr, *d_out = nullptr;
    BANDS_HIP(buf.get(&d_coeff, n_tab), "hipMalloc (coeff)");
    BANDS_HIP(hipMemcpy(d_coeff, d->coeff, (size_t)n_tab * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy (coeff)");
    const int64_t rpb = bands_rows_per_block(chunk);
    if (want_sim) {
        BANDS_HIP(buf.get(&d_lp0, n * q), "hipMalloc (lp0)");
        BANDS_HIP(buf.get(&d_se, n * q), "hipMalloc (se)");
        BANDS_HIP(buf.get(&d_md, (int64_t)q * d->n_post), "hipMalloc (max_dev)");
        BANDS_HIP(hipMemset(d_md, 0, (size_t)q * d->n_post * sizeof(double)), "hipMemset (max_dev)");
        BANDS_HIP(buf.get(&d_part, ((chunk + rpb - 1) / rpb) * q * d->n_post), "hipMalloc (block maxima)");
    }
    int64_t x_cols = 0;
    if (!dev_data) {
        for (int j = 0; j < q; j++) x_cols += (d->x_fe[j] ? a.kf[j] : 0) + a.kr[j];
        if (x_cols) BANDS_HIP(buf.get(&d_x, chunk * x_cols), "hipMalloc (design chunk)");
    }
    if (n_stage_out) BANDS_HIP(buf.get(&d_out, chunk * q * n_stage_out), "hipMalloc (output chunk)");

    a.n_par = q; a.n_coef = n_coef; a.n_post = d->n_post; a.resp = d->resp ? 1 : 0;
    a.coeff = d_coeff; a.z = d->z; a.plan = plan;
    a.lds = n; a.rows_per_block = rpb; a.part = d_part; a.max_dev = d_md;
    hipStream_t s = nullptr;
    double* const row_out[3] = {est, pw_low, pw_upp};

    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nc = std::min(chunk, n - r0);
        a.n = nc;
        if (dev_data) {
            a.ldx = n;
            for (int j = 0; j < q; j++) { a.xf[j] = d->x_fe[j] ? d->x_fe[j] + r0 : nullptr; a.xr[j] = d->x_re[j] ? d->x_re[j] + r0 : nullptr; }
        } else {
            a.ldx = nc;
            double* w = d_x;
            for (int j = 0; j < q; j++) {
                a.xf[j] = nullptr; a.xr[j] = nullptr;
                if (d->x_fe[j]) {
                    BANDS_HIP(bands_copy_rows(w, nc, d->x_fe[j] + r0, n, nc, a.kf[j], hipMemcpyHostToDevice), "hipMemcpy (x_fe)");
                    a.xf[j] = w; w += nc * a.kf[j];
                }
                if (d->x_re[j]) {
                    BANDS_HIP(bands_copy_rows(w, nc, d->x_re[j] + r0, n, nc, a.kr[j], hipMemcpyHostToDevice), "hipMemcpy (x_re)");
                    a.xr[j] = w; w += nc * a.kr[j];
                }
            }
        }
        double* o[3] = {nullptr, nullptr, nullptr};
        if (dev_out) {
            a.ldo = n;
            for (int t = 0; t < 3; t++) o[t] = row_out[t] ? row_out[t] + r0 : nullptr;
        } else {
            a.ldo = nc;
            double* w = d_out;
            for (int t = 0; t < 3; t++)
                if (row_out[t]) { o[t] = w; w += nc * q; }
        }
        a.est = o[0]; a.pw_low = o[1]; a.pw_upp = o[2];
        a.lp0 = d_lp0 ? d_lp0 + r0 : nullptr; a.se = d_se ? d_se + r0 : nullptr;
        if (n_row_out || want_sim) BANDS_HIP(launch_bands_rows(a, s), "pass 1 launch");
        if (want_sim) BANDS_HIP(launch_bands_dev(a, s), "pass 2 launch");
        BANDS_HIP(hipStreamSynchronize(s), "pass 1 / 2");
        if (!dev_out)
            for (int t = 0; t < 3; t++)
                if (row_out[t]) BANDS_HIP(bands_copy_rows(row_out[t] + r0, n, o[t], nc, nc, q, hipMemcpyDeviceToHost), "hipMemcpy (outputs)");
    }
    if (!want_sim) return SSDE_OK;

    // crit: the level quantile of each parameter's maxima, on the host
    std::vector<double> md((size_t)q * d->n_post), sorted((size_t)d->n_post);
    BANDS_HIP(hipMemcpy(md.data(), d_md, md.size() * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy (max_dev)");
    const BandsQ Q = bands_q(d->n_post, d->level);
    for (int j = 0; j < q; j++) {
        std::copy(md.begin() + (size_t)j * d->n_post, md.begin() + (size_t)(j + 1) * d->n_post, sorted.begin());
        std::sort(sorted.begin(), sorted.end());
        const double c = bands_lerp(sorted[(size_t)Q.lo], sorted[(size_t)Q.hi], Q.frac);
        a.crit[j] = c == c ? c : 0.0;
        if (crit) crit[j] = a.crit[j];
    }
    if (max_dev) std::copy(md.begin(), md.end(), max_dev);
    if (!sim_low && !sim_upp) return SSDE_OK;

    // pass 3 over the rows again: straight into the caller's HBM, or chunk by chunk through the staging buffer
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nc = dev_out ? n : std::min(chunk, n - r0);
        a.n = nc; a.lp0 = d_lp0 + r0; a.se = d_se + r0;
        if (dev_out) {
            a.ldo = n; a.sim_low = sim_low; a.sim_upp = sim_upp;
        } else {
            a.ldo = nc; a.sim_low = sim_low ? d_out : nullptr; a.sim_upp = sim_upp ? d_out + (sim_low ? nc * q : 0) : nullptr;
        }
        BANDS_HIP(launch_bands_sim(a, s), "pass 3 launch");
        BANDS_HIP(hipStreamSynchronize(s), "pass 3");
        if (dev_out) break;
        if (sim_low) BANDS_HIP(bands_copy_rows(sim_low + r0, n, a.sim_low, nc, nc, q, hipMemcpyDeviceToHost), "hipMemcpy (sim_low)");
        if (sim_upp) BANDS_HIP(bands_copy_rows(sim_upp + r0, n, a.sim_upp, nc, nc, q, hipMemcpyDeviceToHost), "hipMemcpy (sim_upp)");
    }
#undef BANDS_HIP
    return SSDE_OK;
}

}  // extern "C"
