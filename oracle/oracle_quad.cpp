// oracle/oracle_quad.cpp -- the restated nllk templates evaluated in IEEE binary128 (liboracle_quad.so).
//
// TEST INFRASTRUCTURE ONLY (tools/extreme_triage.py, tests/test_oracle_quad.py).  Same templates as liboracle.so
// (ssde_oracle.hpp, every function citing /root/reference/src/nllk/*.hpp), instantiated with ssde_oracle::Quad:
//
//   oracle_eval_quad(desc, par, order, &value, grad, fd_step)
//     value = nllk + penalty of the double-precision inputs, evaluated with a 113-bit mantissa, rounded to double once
//     grad  = central differences of that binary128 function with step fd_step (default 1e-10): truncation error
//             O(step^2) ~ 1e-20 relative, rounding 1e-34 / step ~ 1e-24 -- far below any double-precision question.
//             No dual numbers: nothing of the gradient path of liboracle.so is shared.
//
//   oracle_hess_quad(desc, par, idx, n_idx, H, fd_step, n_threads)
//     H (n_idx x n_idx, symmetric) = second central differences of the same binary128 function over the full-parameter indices
//             idx[], step fd_step (default 1e-8): the diagonal by the three-point form (f(+h) - 2 f + f(-h)) / h^2, a mixed entry
//             by the four-point form (f(++) - f(+-) - f(-+) + f(--)) / (4 h^2).  Truncation O(h^2) ~ 1e-16 relative, rounding
//             1e-34 / h^2 ~ 1e-18; rounded to double once per entry.  par_fixed is not consulted: every entry of idx is
//             differentiated.  The pairs are independent and are dealt to n_threads std::threads.
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "quad.hpp"
#include "ssde_oracle.hpp"

using namespace ssde_oracle;

namespace {
Quad total(const Problem& p, const std::vector<Quad>& par) {
    return nllk_data<Quad>(p, par.data(), nullptr) + penalty<Quad>(p, par.data());
}
}  // namespace

extern "C" int oracle_eval_quad(const ssde_desc* d, const double* par, int order, double* value, double* grad,
                                double fd_step) {
    Problem p = make_problem(d);
    const int np = p.n_par_full;
    std::vector<Quad> x(np);
    for (int k = 0; k < np; k++) x[k] = Quad(par[k]);
    *value = asDouble(total(p, x));
    if (order < 1 || !grad) return 0;
    const __float128 h = fd_step > 0.0 ? (__float128)fd_step : (__float128)1e-10;
    for (int k = 0; k < np; k++) {
        grad[k] = 0.0;
        if (d->par_fixed && d->par_fixed[k]) continue;
        const Quad keep = x[k];
        x[k] = q128(keep.v + h);
        const Quad fp = total(p, x);
        x[k] = q128(keep.v - h);
        const Quad fm = total(p, x);
        x[k] = keep;
        grad[k] = (double)((fp.v - fm.v) / (2 * h));
    }
    return 0;
}

extern "C" int oracle_hess_quad(const ssde_desc* d, const double* par, const int32_t* idx, int n_idx, double* H, double fd_step,
                                int n_threads) {
    const Problem p = make_problem(d);
    const int np = p.n_par_full;
    if (!par || !idx || !H || n_idx < 1) return 1;
    for (int k = 0; k < n_idx; k++) if (idx[k] < 0 || idx[k] >= np) return 1;
    std::vector<Quad> x0(np);
    for (int k = 0; k < np; k++) x0[k] = Quad(par[k]);
    const __float128 h = fd_step > 0.0 ? (__float128)fd_step : (__float128)1e-8;
    const Quad f0 = total(p, x0);
    std::vector<std::pair<int, int>> pairs;
    for (int a = 0; a < n_idx; a++) for (int b = a; b < n_idx; b++) pairs.push_back({a, b});
    std::atomic<size_t> next{0};
    auto work = [&]() {
        std::vector<Quad> x(x0);
        for (size_t k = next++; k < pairs.size(); k = next++) {
            const int a = pairs[k].first, b = pairs[k].second, ia = idx[a], ib = idx[b];
            auto at = [&](int sa, int sb) {
                x[ia] = q128(x0[ia].v + sa * h);
                if (ib != ia) x[ib] = q128(x0[ib].v + sb * h);
                const Quad f = total(p, x);
                x[ia] = x0[ia]; x[ib] = x0[ib];
                return f.v;
            };
            __float128 v;
            if (ia == ib) v = (at(1, 1) - 2 * f0.v + at(-1, -1)) / (h * h);
            else v = (at(1, 1) - at(1, -1) - at(-1, 1) + at(-1, -1)) / (4 * h * h);
            H[a + (size_t)b * n_idx] = H[b + (size_t)a * n_idx] = (double)v;
        }
    };
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, n_threads), pairs.size()));
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    return 0;
}

// arbiter mode of the restatement (ssde_oracle.hpp: keep_P_symmetric): 0 = the literal recursion (default), 1 = P <- (P + P') / 2
extern "C" void ssde_oracle_keep_P_symmetric(int on) { ssde_oracle::keep_P_symmetric() = on != 0; }

