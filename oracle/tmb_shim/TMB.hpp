// oracle/tmb_shim/TMB.hpp -- a stand-in for <TMB.hpp>, written for this project (TEST INFRASTRUCTURE ONLY).
//
// The reference's likelihood sources (src/smoothSDE.cpp and src/nllk/*.hpp of smoothSDE) include <TMB.hpp> and use a small,
// enumerable slice of the TMB / Eigen surface.  This header provides exactly that slice, so that those sources compile
// UNMODIFIED against it (oracle/Makefile, target `ref`; oracle/ref_capi.cpp is the entry point).  Nothing here is taken from
// TMB, Eigen, CppAD or the reference, and nothing here includes oracle/ssde_oracle.hpp: the point is a second, independent
// route from the reference's program text to a number.
//
// What is a restatement in this file (oracle/README.md lists it as still unpinned):
//   vector<Type>   array semantics: `*` and `/` are elementwise, exp / log / sqrt map; matrix * vector is the matrix product
//   matrix<Type>   dynamic, column-major; row / col / block are assignable views; inverse() is a partial-pivot LU solve of I
//   array<Type>    carries its dimensions: col(i) drops the last one, matrix() reshapes a 2-d array
//   dnorm, dt      TMB's published log-densities;  atomic::logdet = sum log|diag(LU)|;  atomic::matinvpd = inverse and
//                  log-determinant of a positive definite matrix (LDL');  density::GMRF(Q).Quadform(x) = x'Qx
//   besselI        ascending series of the modified Bessel function of the first kind (unscaled: overflows like R's)
//   R_IsNA         a NaN whose low 32-bit word is 1954
//   DATA_* / PARAMETER* / REPORT   look a name up in tables the entry point fills (objective_function<Type>)
// Every scalar operation is left to the scalar type: double, ssde_oracle::Dual<N> (oracle/dual.hpp) and ssde_oracle::Quad
// (oracle/quad.hpp) all instantiate.
#ifndef SSDE_TMB_SHIM_HPP
#define SSDE_TMB_SHIM_HPP

#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

inline double asDouble(double x) { return x; }

inline bool R_IsNA(double x) {
    if (!(x != x)) return false;
    uint64_t bits;
    std::memcpy(&bits, &x, 8);
    return (uint32_t)(bits & 0xffffffffu) == 1954u;
}

inline void error(const char* msg) { throw std::runtime_error(msg); }

template <class T> struct vector;
template <class T> struct matrix;
namespace Eigen { template <class T> struct SparseMatrix; }

namespace tmb_shim {
template <class T, class S>
using scalar_arg = typename std::enable_if<std::is_arithmetic<S>::value || std::is_same<S, T>::value, int>::type;
template <class T> struct row_view;
template <class T> struct col_view;
template <class T> struct block_view;
}  // namespace tmb_shim

// ---------------------------------------------------------------------------------------------------------------------------
// vector<Type>: a one-dimensional ARRAY (tmbutils::vector derives from Eigen::Array)
// ---------------------------------------------------------------------------------------------------------------------------
template <class T>
struct vector {
    std::vector<T> d_;
    vector() {}
    explicit vector(int n) : d_((size_t)n) {}
    vector(const std::vector<T>& v) : d_(v) {}
    int size() const { return (int)d_.size(); }
    T& operator()(int i) { return d_[(size_t)i]; }
    const T& operator()(int i) const { return d_[(size_t)i]; }
    T& operator[](int i) { return d_[(size_t)i]; }
    const T& operator[](int i) const { return d_[(size_t)i]; }
    void setZero() { for (auto& x : d_) x = T(0); }
    vector segment(int start, int n) const {
        vector r(n);
        for (int i = 0; i < n; i++) r.d_[i] = d_[(size_t)(start + i)];
        return r;
    }
    T sum() const {
        T s = T(0);
        for (const auto& x : d_) s = s + x;
        return s;
    }
    vector array() const { return *this; }
    vector matrix() const { return *this; }
    vector transpose() const { return *this; }
};

#define TMB_SHIM_VEC_OP(OP)                                                                              \
    template <class T> vector<T> operator OP(const vector<T>& a, const vector<T>& b) {                   \
        vector<T> r(a.size());                                                                           \
        for (int i = 0; i < a.size(); i++) r[i] = a[i] OP b[i];                                          \
        return r;                                                                                        \
    }                                                                                                    \
    template <class T, class S, tmb_shim::scalar_arg<T, S> = 0> vector<T> operator OP(const S& s, const vector<T>& b) { \
        vector<T> r(b.size());                                                                           \
        for (int i = 0; i < b.size(); i++) r[i] = T(s) OP b[i];                                          \
        return r;                                                                                        \
    }                                                                                                    \
    template <class T, class S, tmb_shim::scalar_arg<T, S> = 0> vector<T> operator OP(const vector<T>& a, const S& s) { \
        vector<T> r(a.size());                                                                           \
        for (int i = 0; i < a.size(); i++) r[i] = a[i] OP T(s);                                          \
        return r;                                                                                        \
    }
TMB_SHIM_VEC_OP(+)
TMB_SHIM_VEC_OP(-)
TMB_SHIM_VEC_OP(*)
TMB_SHIM_VEC_OP(/)
#undef TMB_SHIM_VEC_OP

template <class T> vector<T> operator-(const vector<T>& a) {
    vector<T> r(a.size());
    for (int i = 0; i < a.size(); i++) r[i] = -a[i];
    return r;
}
template <class T> vector<T> exp(const vector<T>& a) {
    vector<T> r(a.size());
    for (int i = 0; i < a.size(); i++) r[i] = exp(a[i]);
    return r;
}
template <class T> vector<T> log(const vector<T>& a) {
    vector<T> r(a.size());
    for (int i = 0; i < a.size(); i++) r[i] = log(a[i]);
    return r;
}
template <class T> vector<T> sqrt(const vector<T>& a) {
    vector<T> r(a.size());
    for (int i = 0; i < a.size(); i++) r[i] = sqrt(a[i]);
    return r;
}
template <class T> vector<T> diff(const vector<T>& a) {
    vector<T> r(a.size() > 0 ? a.size() - 1 : 0);
    for (int i = 0; i + 1 < a.size(); i++) r[i] = a[i + 1] - a[i];
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// matrix<Type>: dynamic, column-major
// ---------------------------------------------------------------------------------------------------------------------------
template <class T>
struct matrix {
    int r_, c_;
    std::vector<T> d_;
    matrix() : r_(0), c_(0) {}
    matrix(int r, int c) : r_(r), c_(c), d_((size_t)r * (size_t)c) {}
    matrix(const Eigen::SparseMatrix<T>& s);
    matrix(const tmb_shim::block_view<T>& b);
    int rows() const { return r_; }
    int cols() const { return c_; }
    int size() const { return r_ * c_; }
    T& operator()(int i, int j) { return d_[(size_t)i + (size_t)j * r_]; }
    const T& operator()(int i, int j) const { return d_[(size_t)i + (size_t)j * r_]; }
    void setZero() { for (auto& x : d_) x = T(0); }
    void setIdentity() {
        setZero();
        for (int i = 0; i < r_ && i < c_; i++) (*this)(i, i) = T(1);
    }
    tmb_shim::row_view<T> row(int i) const { return tmb_shim::row_view<T>{const_cast<matrix*>(this), i}; }
    tmb_shim::col_view<T> col(int j) const { return tmb_shim::col_view<T>{const_cast<matrix*>(this), j}; }
    tmb_shim::block_view<T> block(int i, int j, int nr, int nc) const {
        return tmb_shim::block_view<T>{const_cast<matrix*>(this), i, j, nr, nc};
    }
    matrix transpose() const {
        matrix r(c_, r_);
        for (int j = 0; j < c_; j++)
            for (int i = 0; i < r_; i++) r(j, i) = (*this)(i, j);
        return r;
    }
    matrix array() const { return *this; }
    matrix inverse() const;
    T sum() const {
        T s = T(0);
        for (const auto& x : d_) s = s + x;
        return s;
    }
};

namespace tmb_shim {

template <class T>
struct row_view {
    ::matrix<T>* m;
    int i;
    int size() const { return m->cols(); }
    operator ::vector<T>() const {
        ::vector<T> r(m->cols());
        for (int j = 0; j < m->cols(); j++) r[j] = (*m)(i, j);
        return r;
    }
    ::vector<T> transpose() const { return *this; }
    ::vector<T> array() const { return *this; }
    row_view& operator=(const ::vector<T>& v) {
        for (int j = 0; j < m->cols(); j++) (*m)(i, j) = v[j];
        return *this;
    }
    row_view& operator=(const row_view& o) { return *this = (::vector<T>)o; }
};

template <class T>
struct col_view {
    ::matrix<T>* m;
    int j;
    int size() const { return m->rows(); }
    operator ::vector<T>() const {
        ::vector<T> r(m->rows());
        for (int i = 0; i < m->rows(); i++) r[i] = (*m)(i, j);
        return r;
    }
    ::vector<T> transpose() const { return *this; }
    ::vector<T> array() const { return *this; }
    col_view& operator=(const ::vector<T>& v) {
        for (int i = 0; i < m->rows(); i++) (*m)(i, j) = v[i];
        return *this;
    }
    col_view& operator=(const col_view& o) { return *this = (::vector<T>)o; }
};

template <class T>
struct block_view {
    ::matrix<T>* m;
    int i0, j0, nr, nc;
    ::matrix<T> eval() const {
        ::matrix<T> r(nr, nc);
        for (int j = 0; j < nc; j++)
            for (int i = 0; i < nr; i++) r(i, j) = (*m)(i0 + i, j0 + j);
        return r;
    }
    ::matrix<T> array() const { return eval(); }
    ::matrix<T> matrix() const { return eval(); }
    block_view& operator=(const ::matrix<T>& v) {
        for (int j = 0; j < nc; j++)
            for (int i = 0; i < nr; i++) (*m)(i0 + i, j0 + j) = v(i, j);
        return *this;
    }
    block_view& operator=(const block_view& o) { return *this = o.eval(); }
};

// a row or a column scaled by a scalar (nllk_bm_ssm's drift)
template <class T> ::vector<T> operator*(const row_view<T>& a, const T& s) { return (::vector<T>)a * s; }
template <class T> ::vector<T> operator*(const T& s, const row_view<T>& a) { return s * (::vector<T>)a; }
template <class T> ::vector<T> operator*(const col_view<T>& a, const T& s) { return (::vector<T>)a * s; }
template <class T> ::vector<T> operator*(const T& s, const col_view<T>& a) { return s * (::vector<T>)a; }

// partial-pivot LU of a square matrix: rows of `lu` permuted as perm says, unit lower factor below the diagonal
template <class T>
struct pivoted_lu {
    ::matrix<T> lu;
    std::vector<int> perm;
    explicit pivoted_lu(const ::matrix<T>& a) : lu(a), perm((size_t)a.rows()) {
        const int n = a.rows();
        for (int i = 0; i < n; i++) perm[i] = i;
        for (int k = 0; k < n; k++) {
            int piv = k;
            double best = std::fabs(asDouble(lu(k, k)));
            for (int i = k + 1; i < n; i++) {
                const double v = std::fabs(asDouble(lu(i, k)));
                if (v > best) { best = v; piv = i; }
            }
            if (piv != k) {
                for (int j = 0; j < n; j++) std::swap(lu(k, j), lu(piv, j));
                std::swap(perm[k], perm[piv]);
            }
            for (int i = k + 1; i < n; i++) {
                lu(i, k) = lu(i, k) / lu(k, k);
                for (int j = k + 1; j < n; j++) lu(i, j) = lu(i, j) - lu(i, k) * lu(k, j);
            }
        }
    }
    ::matrix<T> solve_identity() const {
        const int n = lu.rows();
        ::matrix<T> x(n, n);
        std::vector<T> y((size_t)n);
        for (int c = 0; c < n; c++) {
            for (int i = 0; i < n; i++) {
                T s = (perm[i] == c) ? T(1) : T(0);
                for (int j = 0; j < i; j++) s = s - lu(i, j) * y[j];
                y[i] = s;
            }
            for (int i = n - 1; i >= 0; i--) {
                T s = y[i];
                for (int j = i + 1; j < n; j++) s = s - lu(i, j) * x(j, c);
                x(i, c) = s / lu(i, i);
            }
        }
        return x;
    }
};

}  // namespace tmb_shim

template <class T> matrix<T>::matrix(const tmb_shim::block_view<T>& b) { *this = b.eval(); }
template <class T> matrix<T> matrix<T>::inverse() const { return tmb_shim::pivoted_lu<T>(*this).solve_identity(); }

template <class T> matrix<T> operator*(const matrix<T>& a, const matrix<T>& b) {
    matrix<T> r(a.rows(), b.cols());
    r.setZero();
    for (int j = 0; j < b.cols(); j++)
        for (int k = 0; k < a.cols(); k++)
            for (int i = 0; i < a.rows(); i++) r(i, j) = r(i, j) + a(i, k) * b(k, j);
    return r;
}
template <class T> matrix<T> operator+(const matrix<T>& a, const matrix<T>& b) {
    matrix<T> r(a.rows(), a.cols());
    for (size_t i = 0; i < r.d_.size(); i++) r.d_[i] = a.d_[i] + b.d_[i];
    return r;
}
template <class T> matrix<T> operator-(const matrix<T>& a, const matrix<T>& b) {
    matrix<T> r(a.rows(), a.cols());
    for (size_t i = 0; i < r.d_.size(); i++) r.d_[i] = a.d_[i] - b.d_[i];
    return r;
}
// matrix * vector: the matrix-vector product, returned as a vector (tmbutils)
template <class T> vector<T> operator*(const matrix<T>& a, const vector<T>& x) {
    vector<T> r(a.rows());
    r.setZero();
    for (int k = 0; k < a.cols(); k++)
        for (int i = 0; i < a.rows(); i++) r[i] = r[i] + a(i, k) * x[k];
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// array<Type>: values with their dimensions (column-major, like R)
// ---------------------------------------------------------------------------------------------------------------------------
template <class T>
struct array {
    std::vector<int> dim;
    std::vector<T> d_;
    int size() const { return (int)d_.size(); }
    // the i-th slice along the LAST dimension
    array col(int i) const {
        array r;
        size_t len = 1;
        for (size_t k = 0; k + 1 < dim.size(); k++) { r.dim.push_back(dim[k]); len *= (size_t)dim[k]; }
        r.d_.assign(d_.begin() + (ptrdiff_t)(len * (size_t)i), d_.begin() + (ptrdiff_t)(len * (size_t)(i + 1)));
        return r;
    }
    ::matrix<T> matrix() const {
        const int r = dim.size() > 0 ? dim[0] : 0, c = dim.size() > 1 ? dim[1] : 1;
        ::matrix<T> m(r, c);
        for (size_t k = 0; k < m.d_.size(); k++) m.d_[k] = d_[k];
        return m;
    }
};

// ---------------------------------------------------------------------------------------------------------------------------
// Eigen::SparseMatrix<Type>: compressed columns
// ---------------------------------------------------------------------------------------------------------------------------
namespace Eigen {
template <class T>
struct SparseMatrix {
    int r_ = 0, c_ = 0;
    std::vector<int> colptr{0}, rowidx;
    std::vector<T> val;
    int rows() const { return r_; }
    int cols() const { return c_; }
    SparseMatrix block(int i0, int j0, int nr, int nc) const {
        SparseMatrix b;
        b.r_ = nr; b.c_ = nc;
        b.colptr.assign(1, 0);
        for (int j = 0; j < nc; j++) {
            for (int p = colptr[(size_t)(j0 + j)]; p < colptr[(size_t)(j0 + j + 1)]; p++)
                if (rowidx[(size_t)p] >= i0 && rowidx[(size_t)p] < i0 + nr) {
                    b.rowidx.push_back(rowidx[(size_t)p] - i0);
                    b.val.push_back(val[(size_t)p]);
                }
            b.colptr.push_back((int)b.rowidx.size());
        }
        return b;
    }
    ::vector<T> col(int j) const {
        ::vector<T> r(r_);
        r.setZero();
        for (int p = colptr[(size_t)j]; p < colptr[(size_t)j + 1]; p++) r[rowidx[(size_t)p]] = val[(size_t)p];
        return r;
    }
};
}  // namespace Eigen

template <class T> matrix<T>::matrix(const Eigen::SparseMatrix<T>& s) : r_(s.rows()), c_(s.cols()), d_((size_t)s.rows() * (size_t)s.cols()) {
    setZero();
    for (int j = 0; j < c_; j++)
        for (int p = s.colptr[(size_t)j]; p < s.colptr[(size_t)j + 1]; p++) (*this)(s.rowidx[(size_t)p], j) = s.val[(size_t)p];
}
template <class T> vector<T> operator*(const Eigen::SparseMatrix<T>& a, const vector<T>& x) {
    vector<T> r(a.rows());
    r.setZero();
    for (int j = 0; j < a.cols(); j++)
        for (int p = a.colptr[(size_t)j]; p < a.colptr[(size_t)j + 1]; p++)
            r[a.rowidx[(size_t)p]] = r[a.rowidx[(size_t)p]] + a.val[(size_t)p] * x[j];
    return r;
}
// explicit zeros are dropped, as a conversion to a sparse class does
template <class T> Eigen::SparseMatrix<T> asSparseMatrix(const matrix<T>& m) {
    Eigen::SparseMatrix<T> s;
    s.r_ = m.rows(); s.c_ = m.cols();
    s.colptr.assign(1, 0);
    for (int j = 0; j < m.cols(); j++) {
        for (int i = 0; i < m.rows(); i++)
            if (asDouble(m(i, j)) != 0.0) { s.rowidx.push_back(i); s.val.push_back(m(i, j)); }
        s.colptr.push_back((int)s.rowidx.size());
    }
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// densities and special functions
// ---------------------------------------------------------------------------------------------------------------------------
template <class T> T dnorm(T x, T mean, T sd, int give_log = 0) {
    T resid = (x - mean) / sd;
    T logans = T(-std::log(std::sqrt(2.0 * M_PI))) - log(sd) - T(0.5) * resid * resid;
    return give_log ? logans : exp(logans);
}
// Student's t density with df degrees of freedom
template <class T> T dt(T x, T df, int give_log = 0) {
    T logres = lgamma((df + 1) / 2) - T(1) / 2 * log(df * M_PI) - lgamma(df / 2) - (df + 1) / 2 * log(1 + x * x / df);
    return give_log ? logres : exp(logres);
}
// I_nu(x) = sum_k (x/2)^(2k+nu) / (k! Gamma(k+nu+1)), x >= 0, nu > -1: every term is positive.  Unscaled, so it overflows where the
// scalar type does (x beyond ~700 in double), like R's besselI(x, nu) behind TMB's.
template <class T> T besselI(T x, T nu) {
    T y = x * x / 4;
    T t = exp(nu * log(x / 2) - lgamma(nu + 1));
    T s = t;
    for (int k = 1; k < 2000000; k++) {
        t = t * y / (T(k) * (T(k) + nu));
        s = s + t;
        if (!(asDouble(t) > 1e-40 * asDouble(s))) break;
    }
    return s;
}

namespace atomic {
// log|det| from the diagonal of a partial-pivot LU
template <class T> T logdet(const matrix<T>& m) {
    tmb_shim::pivoted_lu<T> f(m);
    T s = T(0);
    for (int i = 0; i < m.rows(); i++) s = s + log(fabs(f.lu(i, i)));
    return s;
}
// inverse of a positive definite matrix; its log-determinant is returned through `logdet` (sum of log D of S = L D L')
template <class T> matrix<T> matinvpd(const matrix<T>& m, T& logdet) {
    const int n = m.rows();
    matrix<T> l(n, n);
    l.setZero();
    std::vector<T> dg((size_t)n);
    logdet = T(0);
    for (int j = 0; j < n; j++) {
        T dj = m(j, j);
        for (int k = 0; k < j; k++) dj = dj - l(j, k) * l(j, k) * dg[k];
        dg[j] = dj;
        l(j, j) = T(1);
        for (int i = j + 1; i < n; i++) {
            T s = m(i, j);
            for (int k = 0; k < j; k++) s = s - l(i, k) * l(j, k) * dg[k];
            l(i, j) = s / dj;
        }
        logdet = logdet + log(dj);
    }
    return m.inverse();
}
}  // namespace atomic

namespace density {
template <class T>
struct GMRF_t {
    Eigen::SparseMatrix<T> Q;
    T Quadform(const vector<T>& x) const { return (x * (Q * x)).sum(); }
};
template <class T> GMRF_t<T> GMRF(const Eigen::SparseMatrix<T>& Q) { return GMRF_t<T>{Q}; }
}  // namespace density

namespace R_inla {}

// ---------------------------------------------------------------------------------------------------------------------------
// objective_function<Type>: data and parameters by name
// ---------------------------------------------------------------------------------------------------------------------------
namespace tmb_shim {
struct datum {
    std::string str;                 // DATA_STRING
    std::vector<double> val;         // values, column-major (dense), or the stored entries (sparse)
    std::vector<int> dim;            // dimensions
    bool sparse = false;
    std::vector<int> colptr, rowidx; // compressed columns (sparse)
};
typedef std::map<std::string, datum> data_table;
}  // namespace tmb_shim

template <class Type>
class objective_function {
public:
    const tmb_shim::data_table* data = nullptr;
    std::map<std::string, std::vector<Type> > par;
    std::map<std::string, matrix<Type> > reports;

    Type operator()();   // defined by the model source

    const tmb_shim::datum& shim_get(const char* name) const {
        auto it = data->find(name);
        if (it == data->end()) throw std::runtime_error(std::string("tmb_shim: no data object named ") + name);
        return it->second;
    }
    std::string shim_string(const char* name) const { return shim_get(name).str; }
    int shim_integer(const char* name) const { return (int)shim_get(name).val.at(0); }
    vector<Type> shim_vector(const char* name) const {
        const tmb_shim::datum& d = shim_get(name);
        vector<Type> v((int)d.val.size());
        for (size_t i = 0; i < d.val.size(); i++) v.d_[i] = Type(d.val[i]);
        return v;
    }
    vector<int> shim_ivector(const char* name) const {
        const tmb_shim::datum& d = shim_get(name);
        vector<int> v((int)d.val.size());
        for (size_t i = 0; i < d.val.size(); i++) v.d_[i] = (int)d.val[i];
        return v;
    }
    matrix<Type> shim_matrix(const char* name) const {
        const tmb_shim::datum& d = shim_get(name);
        matrix<Type> m(d.dim.at(0), d.dim.at(1));
        for (size_t i = 0; i < d.val.size(); i++) m.d_[i] = Type(d.val[i]);
        return m;
    }
    array<Type> shim_array(const char* name) const {
        const tmb_shim::datum& d = shim_get(name);
        array<Type> a;
        a.dim = d.dim;
        a.d_.resize(d.val.size());
        for (size_t i = 0; i < d.val.size(); i++) a.d_[i] = Type(d.val[i]);
        return a;
    }
    Eigen::SparseMatrix<Type> shim_sparse(const char* name) const {
        const tmb_shim::datum& d = shim_get(name);
        if (!d.sparse) throw std::runtime_error(std::string("tmb_shim: not a sparse matrix: ") + name);
        Eigen::SparseMatrix<Type> s;
        s.r_ = d.dim.at(0); s.c_ = d.dim.at(1);
        s.colptr = d.colptr; s.rowidx = d.rowidx;
        s.val.resize(d.val.size());
        for (size_t i = 0; i < d.val.size(); i++) s.val[i] = Type(d.val[i]);
        return s;
    }
    vector<Type> shim_par(const char* name) const {
        auto it = par.find(name);
        if (it == par.end()) throw std::runtime_error(std::string("tmb_shim: no parameter named ") + name);
        return vector<Type>(it->second);
    }
    void shim_report(const char* name, const matrix<Type>& m) { reports[name] = m; }
};

#define TMB_OBJECTIVE_PTR this
#define DATA_STRING(name) std::string name = TMB_OBJECTIVE_PTR->shim_string(#name);
#define DATA_INTEGER(name) int name = TMB_OBJECTIVE_PTR->shim_integer(#name);
#define DATA_VECTOR(name) vector<Type> name = TMB_OBJECTIVE_PTR->shim_vector(#name);
#define DATA_IVECTOR(name) vector<int> name = TMB_OBJECTIVE_PTR->shim_ivector(#name);
#define DATA_MATRIX(name) matrix<Type> name = TMB_OBJECTIVE_PTR->shim_matrix(#name);
#define DATA_ARRAY(name) array<Type> name = TMB_OBJECTIVE_PTR->shim_array(#name);
#define DATA_SPARSE_MATRIX(name) Eigen::SparseMatrix<Type> name = TMB_OBJECTIVE_PTR->shim_sparse(#name);
#define PARAMETER(name) Type name = TMB_OBJECTIVE_PTR->shim_par(#name)(0);
#define PARAMETER_VECTOR(name) vector<Type> name = TMB_OBJECTIVE_PTR->shim_par(#name);
#define REPORT(name) TMB_OBJECTIVE_PTR->shim_report(#name, name);

#endif
