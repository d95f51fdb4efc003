// oracle/ref_capi.cpp -- C entry points over the REFERENCE's own likelihood sources (TEST INFRASTRUCTURE ONLY).
//
// This translation unit includes the reference's src/smoothSDE.cpp (and through it its five src/nllk/*.hpp) UNMODIFIED, from a
// checkout outside this repository (oracle/Makefile: REFERENCE), compiled against the stand-in <TMB.hpp> of oracle/tmb_shim/.
// It takes the same descriptor as oracle_eval (include/ssde.h), assembles `tmb_dat` / `tmb_par` from it the way the package's R
// side does (R/sde.R: SDE$make_mat and SDE$setup) and calls objective_function<Type>::operator():
//
//   ref_eval(desc, par, n_par_full, order, &value, grad, aest_all)        -> oracle/_ref/libssde_ref.so
//     value with Type = double; grad over the FULL parameter vector by forward-mode duals (oracle/dual.hpp) through the
//     reference's own templates, 0 for par_fixed entries; aest_all [n x sdim] column-major = REPORT(aest_all), or NULL
//   ref_eval_quad(desc, par, n_par_full, order, &value, grad, fd_step)    -> oracle/_ref/libssde_ref_quad.so (-DSSDE_REF_QUAD)
//     value with Type = IEEE binary128 (oracle/quad.hpp), rounded to double once; grad by central differences of that function
//
// Nothing of oracle/ssde_oracle.hpp is used.  What is NOT compiled reference text here, and so stays a restatement:
// the assembly of tmb_dat below (block-diagonal designs, sentinels, 1-based decay indices) and, where the descriptor leaves
// a0 / P0 to the default, r_side_defaults().
#include <cstdint>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../include/ssde.h"
#include "dual.hpp"
#ifdef SSDE_REF_QUAD
#include "quad.hpp"
#endif

#include "smoothSDE.cpp"   // the reference's source, found through -I $(REFERENCE)/src

namespace {

using tmb_shim::data_table;
using tmb_shim::datum;

datum dense(const std::vector<double>& v, std::vector<int> dim) {
    datum d;
    d.val = v;
    d.dim = std::move(dim);
    return d;
}
datum vec(const double* p, size_t n) { return dense(std::vector<double>(p, p + n), {(int)n}); }
datum scalar_vec(double x) { return dense({x}, {1}); }

// as_sparse(bdiag(blocks)): block b is n_rows[b] x n_cols[b], column-major, or NULL = a column of ones; zeros are dropped
datum block_diagonal(const std::vector<const double*>& blocks, const std::vector<int>& n_rows, const std::vector<int>& n_cols) {
    datum d;
    d.sparse = true;
    int R = 0, Cc = 0;
    d.colptr.push_back(0);
    for (size_t b = 0; b < blocks.size(); b++) {
        for (int c = 0; c < n_cols[b]; c++) {
            for (int i = 0; i < n_rows[b]; i++) {
                const double x = blocks[b] ? blocks[b][(size_t)i + (size_t)c * n_rows[b]] : 1.0;
                if (x != 0.0) { d.rowidx.push_back(R + i); d.val.push_back(x); }
            }
            d.colptr.push_back((int)d.rowidx.size());
        }
        R += n_rows[b];
        Cc += n_cols[b];
    }
    d.dim = {R, Cc};
    return d;
}
datum sparse_zeros(int rows, int cols) {
    datum d;
    d.sparse = true;
    d.dim = {rows, cols};
    d.colptr.assign((size_t)cols + 1, 0);
    return d;
}

const char* type_name(int model) {
    switch (model) {
        case SSDE_MODEL_BM: return "BM";
        case SSDE_MODEL_OU: return "OU";
        case SSDE_MODEL_BM_SSM: return "BM_SSM";
        case SSDE_MODEL_OU_SSM: return "OU_SSM";
        case SSDE_MODEL_CTCRW: return "CTCRW";
        case SSDE_MODEL_BM_T: return "BM_t";
        case SSDE_MODEL_ESEAL_SSM: return "ESEAL_SSM";
        case SSDE_MODEL_CIR: return "CIR";
    }
    return "?";
}
bool is_ssm(int m) { return m == SSDE_MODEL_BM_SSM || m == SSDE_MODEL_OU_SSM || m == SSDE_MODEL_CTCRW; }
bool is_direct(int m) { return m == SSDE_MODEL_BM || m == SSDE_MODEL_OU || m == SSDE_MODEL_BM_T || m == SSDE_MODEL_CIR; }
int state_dim(const ssde_desc* d) {
    if (d->model == SSDE_MODEL_CTCRW) return 2 * d->n_dim;
    if (d->model == SSDE_MODEL_ESEAL_SSM) return 2;
    return is_ssm(d->model) ? d->n_dim : 0;
}

// ==== RESTATEMENT OF R CODE, NOT COMPILED REFERENCE TEXT (stays unpinned) =====================================================
// The a0 / P0 that SDE$setup builds when the user gives none: first observation of every ID segment as the initial state
// (BM_SSM / OU_SSM), (x1, 0, y1, 0, ...) for CTCRW; P0 = diag(10, ...) resp. diag(1, 10, 1, 10, ...), diag(0, 10) for ESEAL_SSM.
void r_side_defaults(const ssde_desc* d, const std::vector<int64_t>& seg_start, std::vector<double>* a0, std::vector<double>* p0) {
    const int sdim = state_dim(d);
    const size_t n_seg = seg_start.size();
    if (a0) {
        a0->assign(n_seg * (size_t)sdim, 0.0);
        for (size_t k = 0; k < n_seg; k++)
            for (int a = 0; a < d->n_dim; a++) {
                const int comp = d->model == SSDE_MODEL_CTCRW ? 2 * a : a;
                (*a0)[k + (size_t)comp * n_seg] = d->obs[seg_start[k] + (int64_t)a * d->n];
            }
    }
    if (p0) {
        p0->assign((size_t)sdim * sdim, 0.0);
        for (int i = 0; i < sdim; i++) {
            double v = 10.0;
            if (d->model == SSDE_MODEL_CTCRW) v = (i % 2 == 0) ? 1.0 : 10.0;
            if (d->model == SSDE_MODEL_ESEAL_SSM) v = (i == 0) ? 0.0 : 10.0;
            (*p0)[(size_t)i + (size_t)i * sdim] = v;
        }
    }
}
// ==============================================================================================================================

// where each block of the template's parameter list sits in the full vector (include/ssde.h: PARAMETER VECTOR)
struct Layout {
    int n_lead = 0, n_fe = 0, n_lambda = 0, n_decay = 0, n_re = 0;
    int off_fe = 0, off_lambda = 0, off_decay = 0, off_re = 0, n_par_full = 0;
};
Layout layout_of(const ssde_desc* d) {
    Layout L;
    L.n_lead = is_ssm(d->model) ? 1 : (d->model == SSDE_MODEL_ESEAL_SSM ? 3 : 0);
    for (int j = 0; j < d->n_par; j++) {
        L.n_fe += d->ncol_fe[j];
        L.n_re += d->ncol_re ? d->ncol_re[j] : 0;
    }
    L.n_lambda = d->n_smooth;
    L.n_decay = (is_direct(d->model) && d->n_decay > 0) ? d->n_decay : 0;
    L.off_fe = L.n_lead;
    L.off_lambda = L.off_fe + L.n_fe;
    L.off_decay = L.off_lambda + L.n_lambda;
    L.off_re = L.off_decay + L.n_decay;
    L.n_par_full = L.off_re + L.n_re;
    return L;
}

// tmb_dat of R/sde.R (SDE$setup), from the descriptor
data_table make_tmb_dat(const ssde_desc* d, const Layout& L) {
    data_table t;
    const int64_t n = d->n;
    const int q = d->n_par, nd = d->n_dim;
    t["type"].str = type_name(d->model);
    t["ID"] = vec(d->id, (size_t)n);
    t["times"] = vec(d->times, (size_t)n);
    {
        datum obs = dense(std::vector<double>(d->obs, d->obs + (size_t)n * nd), {(int)n, nd});
        if (d->na_mode == SSDE_NA_ANY_NAN) {
            // a host that marks missing values with any NaN: hand them to the reference as R's NA_real_, the only NaN it tests for
            const uint64_t na_bits = 0x7FF00000000007A2ull;
            double na;
            std::memcpy(&na, &na_bits, 8);
            for (double& x : obs.val)
                if (x != x) x = na;
        }
        t["obs"] = obs;
    }
    // X_fe, X_re: block-diagonal over the SDE parameters (make_mat: bdiag_check(X_list_fe) / (X_list_re))
    std::vector<const double*> bf, br;
    std::vector<int> rows, cf, cr;
    for (int j = 0; j < q; j++) {
        bf.push_back(d->x_fe ? d->x_fe[j] : nullptr);
        cf.push_back(d->ncol_fe[j]);
        const int k = d->ncol_re ? d->ncol_re[j] : 0;
        br.push_back(k > 0 ? d->x_re[j] : nullptr);
        cr.push_back(k);
        rows.push_back((int)n);
    }
    t["X_fe"] = block_diagonal(bf, rows, cf);
    if (d->n_smooth > 0) {
        t["X_re"] = block_diagonal(br, rows, cr);
        std::vector<const double*> sb;
        std::vector<int> sn;
        std::vector<double> ncol;
        const double* p = d->s_blocks;
        for (int s = 0; s < d->n_smooth; s++) {
            sb.push_back(p);
            sn.push_back(d->smooth_ncol[s]);
            ncol.push_back((double)d->smooth_ncol[s]);
            p += (size_t)d->smooth_ncol[s] * d->smooth_ncol[s];
        }
        t["S"] = block_diagonal(sb, sn, sn);
        t["ncol_re"] = dense(ncol, {(int)ncol.size()});
    } else {
        // no random effects: S = 0 (1 x 1), ncol_re = 0, X_re = one column of zeros (SDE$setup, is.null(S) branch)
        t["X_re"] = sparse_zeros((int)n * q, 1);
        t["S"] = sparse_zeros(1, 1);
        t["ncol_re"] = scalar_vec(0.0);
    }
    t["include_penalty"] = scalar_vec((double)d->include_penalty);

    std::vector<int64_t> seg_start;
    for (int64_t i = 0; i < n; i++)
        if (i == 0 || d->id[i] != d->id[i - 1]) seg_start.push_back(i);   // i0 of SDE$setup
    const int sdim = state_dim(d);
    if (is_ssm(d->model) || d->model == SSDE_MODEL_ESEAL_SSM) {
        std::vector<double> a0, p0;
        r_side_defaults(d, seg_start, d->a0 ? nullptr : &a0, d->p0 ? nullptr : &p0);
        if (d->a0) a0.assign(d->a0, d->a0 + (size_t)d->n_seg * sdim);
        if (d->p0) p0.assign(d->p0, d->p0 + (size_t)sdim * sdim);
        t["a0"] = dense(a0, {(int)(d->a0 ? d->n_seg : (int64_t)seg_start.size()), sdim});
        t["P0"] = dense(p0, {sdim, sdim});
    }
    if (is_ssm(d->model)) {
        if (d->h_array)
            t["H_array"] = dense(std::vector<double>(d->h_array, d->h_array + (size_t)nd * nd * n), {nd, nd, (int)n});
        else
            t["H_array"] = scalar_vec(0.0);                                 // array(0)
    }
    if (d->model == SSDE_MODEL_ESEAL_SSM) {
        t["h"] = vec(d->eseal_h, (size_t)n);
        t["R"] = vec(d->eseal_R, (size_t)n);
    }
    if (is_direct(d->model)) {
        if (d->other_data && d->n_other_data > 0) t["other_data"] = vec(d->other_data, (size_t)d->n_other_data);
        else t["other_data"] = scalar_vec(0.0);
        if (L.n_decay > 0) {
            t["t_decay"] = vec(d->t_decay, (size_t)q * n);
            std::vector<double> col, ind;
            for (int c = 0; c < d->n_decay_cols; c++) {
                col.push_back((double)d->col_decay[c] + 1.0);               // R indices are 1-based
                ind.push_back((double)d->ind_decay[c] + 1.0);
            }
            t["col_decay"] = dense(col, {(int)col.size()});
            t["ind_decay"] = dense(ind, {(int)ind.size()});
        } else {
            t["t_decay"] = scalar_vec(0.0);
            t["col_decay"] = scalar_vec(0.0);
            t["ind_decay"] = scalar_vec(0.0);
        }
    }
    return t;
}

// tmb_par of SDE$setup, from the full parameter vector
template <class Type>
void make_tmb_par(const ssde_desc* d, const Layout& L, const Type* par, objective_function<Type>* obj) {
    auto slice = [&](int off, int len) { return std::vector<Type>(par + off, par + off + len); };
    if (is_ssm(d->model)) obj->par["log_sigma_obs"] = slice(0, 1);
    if (d->model == SSDE_MODEL_ESEAL_SSM) {
        obj->par["log_tau"] = slice(0, 1);
        obj->par["a1"] = slice(1, 1);
        obj->par["log_a2"] = slice(2, 1);
    }
    obj->par["coeff_fe"] = slice(L.off_fe, L.n_fe);
    // without random effects log_lambda and coeff_re are the mapped dummies 0 of SDE$setup
    obj->par["log_lambda"] = L.n_lambda > 0 ? slice(L.off_lambda, L.n_lambda) : std::vector<Type>(1, Type(0.0));
    obj->par["coeff_re"] = L.n_lambda > 0 ? slice(L.off_re, L.n_re) : std::vector<Type>(1, Type(0.0));
    if (is_direct(d->model))
        obj->par["log_decay"] = L.n_decay > 0 ? slice(L.off_decay, L.n_decay) : std::vector<Type>(1, Type(0.0));
}

template <class Type>
Type run(const ssde_desc* d, const Layout& L, const data_table& dat, const Type* par, double* aest_all) {
    objective_function<Type> obj;
    obj.data = &dat;
    make_tmb_par(d, L, par, &obj);
    Type v = obj();
    if (aest_all) {
        auto it = obj.reports.find("aest_all");
        if (it != obj.reports.end())
            for (size_t k = 0; k < it->second.d_.size(); k++) aest_all[k] = asDouble(it->second.d_[k]);
    }
    return v;
}

}  // namespace

extern "C" {

int ref_n_par_full(const ssde_desc* d) { return layout_of(d).n_par_full; }

// 1 if REPORT(aest_all) exists for this model (the three state-space families; ESEAL_SSM reports nothing)
int ref_has_report(const ssde_desc* d) { return is_ssm(d->model) ? 1 : 0; }

#ifndef SSDE_REF_QUAD

int ref_eval(const ssde_desc* d, const double* par, int n_par_full, int order, double* value, double* grad, double* aest_all) {
    try {
        const Layout L = layout_of(d);
        if (n_par_full != L.n_par_full) return 1;
        if (d->model == SSDE_MODEL_ESEAL_SSM && !d->a0) return 1;   // its a0 comes from a data column (dep_fat), never from obs
        const data_table dat = make_tmb_dat(d, L);
        *value = run<double>(d, L, dat, par, aest_all);
        if (order < 1 || !grad) return 0;
        constexpr int NB = 8;   // dual directions per pass
        typedef ssde_oracle::Dual<NB> D;
        std::vector<int> free_idx;
        for (int k = 0; k < L.n_par_full; k++) {
            grad[k] = 0.0;
            if (!(d->par_fixed && d->par_fixed[k])) free_idx.push_back(k);
        }
        for (size_t b0 = 0; b0 < free_idx.size(); b0 += NB) {
            const size_t nb = free_idx.size() - b0 < (size_t)NB ? free_idx.size() - b0 : (size_t)NB;
            std::vector<D> dp((size_t)L.n_par_full);
            for (int k = 0; k < L.n_par_full; k++) dp[k] = D(par[k]);
            for (size_t j = 0; j < nb; j++) dp[free_idx[b0 + j]].d[j] = 1.0;
            const D tot = run<D>(d, L, dat, dp.data(), nullptr);
            for (size_t j = 0; j < nb; j++) grad[free_idx[b0 + j]] = tot.d[j];
        }
        return 0;
    } catch (const std::exception&) {
        return 2;
    }
}

#else

int ref_eval_quad(const ssde_desc* d, const double* par, int n_par_full, int order, double* value, double* grad, double fd_step) {
    typedef ssde_oracle::Quad Q;
    try {
        const Layout L = layout_of(d);
        if (n_par_full != L.n_par_full) return 1;
        if (d->model == SSDE_MODEL_ESEAL_SSM && !d->a0) return 1;
        const data_table dat = make_tmb_dat(d, L);
        std::vector<Q> x((size_t)L.n_par_full);
        for (int k = 0; k < L.n_par_full; k++) x[k] = Q(par[k]);
        *value = asDouble(run<Q>(d, L, dat, x.data(), nullptr));
        if (order < 1 || !grad) return 0;
        const __float128 h = fd_step > 0.0 ? (__float128)fd_step : (__float128)1e-10;
        for (int k = 0; k < L.n_par_full; k++) {
            grad[k] = 0.0;
            if (d->par_fixed && d->par_fixed[k]) continue;
            const Q keep = x[k];
            x[k] = ssde_oracle::q128(keep.v + h);
            const Q fp = run<Q>(d, L, dat, x.data(), nullptr);
            x[k] = ssde_oracle::q128(keep.v - h);
            const Q fm = run<Q>(d, L, dat, x.data(), nullptr);
            x[k] = keep;
            grad[k] = (double)((fp.v - fm.v) / (2 * h));
        }
        return 0;
    } catch (const std::exception&) {
        return 2;
    }
}

#endif

}  // extern "C"
