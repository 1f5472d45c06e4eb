// SPD model: exponential map, logarithm, geodesic and the RiemannianSGD step along the geodesic, per-row
// arithmetic compiled by hipcc (spd_expmap.hip, one row / pair per lane) and by g++ (tests/hostsim/hostsim_spd_expmap.cpp).
// PARITY UNPINNED like every spd entry (geoopt is absent); pinned by 100-digit mpmath evaluations of the textbook definitions
// through x^(1/2) (tools/make_golden_spd_expmap_exact.py).
//
// x = L L^T, and for a symmetric W:  A = L^-1 W L^-T = V diag(a) V^T.  Every map is  (x +) L V diag(f(a)) V^T L^T:
//   expmap(x, u)      = x + L V diag(expm1(a)) V^T L^T,                W = sym(u)
//   logmap(x, y)      =     L V diag(log1p(a)) V^T L^T,                W = y - x
//   geodesic(t, x, y) = x + L V diag(expm1(t log1p(a))) V^T L^T,       W = y - x
//   RSGD step         : x <- x + L V diag(expm1(-lr c)) V^T L^T,       L^T S L = V diag(c) V^T,  S = coef sym(g) + wd x
// (the step is expmap(x, -lr x S x): L^-1 (x S x) L^-T = L^T S L, a factor, two triangular products, no solve).  The "x +" forms
// return x bit for bit at u = 0, t = 0, lr = 0 (f = +-0, the whole congruence an exact zero) and keep the relative accuracy of a
// tiny u; y == x gives W = 0 exactly and an exact zero logarithm.  Outputs are symmetric bit for bit (the upper triangle is
// computed and mirrored).  The maps read x and y as their upper triangles (sym_at), the step reads sym(x), sym(g) like spd_row_rsgd.
#pragma once

#include <cmath>

#include "spd_math_bwd.hpp"

namespace sympa {

constexpr int SPD_MAP_EXP = 0, SPD_MAP_LOG = 1, SPD_MAP_GEODESIC = 2;

struct SpdExpWork {
    double l[SPD_MAX_N * SPD_MAX_N];   // Cholesky factor of x (lower)
    double a[SPD_MAX_N * SPD_MAX_N];   // W, then A (destroyed by the QL), then L P
    double v[SPD_MAX_N * SPD_MAX_N];   // eigenvectors (columns)
    double p[SPD_MAX_N * SPD_MAX_N];   // scratch of a product, then P = V diag(f) V^T
    double rd[SPD_MAX_N], lam[SPD_MAX_N], f[SPD_MAX_N], e[SPD_MAX_N];
};

// (L, a, V) from (x, W):  w.a holds the full symmetric W on entry;  A = L^-1 W L^-T (product == false) or L^T W L (true);
// w.l / w.rd = the factor of x (xs: full storage, upper triangle read), w.lam = a, w.v = V.  Returns "x is positive definite".
SYMPA_HD bool spd_exp_spectrum(SpdExpWork& w, const double* __restrict__ xs, int n, bool product, int& status) {
    const bool ok = spd_cholesky(xs, n, w.l, w.rd);
    if (product) {
        for (int i = 0; i < n; ++i)                       // p = W L
            for (int j = 0; j < n; ++j) {
                double t = 0.0;
                for (int k = j; k < n; ++k) t += w.a[i * n + k] * w.l[k * n + j];
                w.p[i * n + j] = t;
            }
        for (int i = 0; i < n; ++i)                       // a = L^T p
            for (int j = 0; j < n; ++j) {
                double t = 0.0;
                for (int k = i; k < n; ++k) t += w.l[k * n + i] * w.p[k * n + j];
                w.a[i * n + j] = t;
            }
    } else {
        spd_congruence_inv(w.a, w.l, w.rd, n);
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) { const double t = 0.5 * (w.a[i * n + j] + w.a[j * n + i]); w.a[i * n + j] = t; w.a[j * n + i] = t; }
    const bool conv = spd_eigh_ql(w.a, w.v, w.lam, w.e, n);
    if (!ok) status |= ST_NOT_PD;
    if (!conv) status |= ST_NO_CONVERGENCE;
    return ok;
}

// out = (xs +) L V diag(w.f) V^T L^T, symmetric bit for bit; xs == nullptr: no first term (the logarithm)
SYMPA_HD void spd_exp_apply(SpdExpWork& w, const double* __restrict__ xs, int n, double* __restrict__ out) {
    for (int i = 0; i < n; ++i)                           // P = V diag(f) V^T
        for (int j = i; j < n; ++j) {
            double t = 0.0;
            for (int k = 0; k < n; ++k) t += w.v[i * n + k] * w.f[k] * w.v[j * n + k];
            w.p[i * n + j] = t;
            w.p[j * n + i] = t;
        }
    for (int i = 0; i < n; ++i)                           // a = L P
        for (int j = 0; j < n; ++j) {
            double t = 0.0;
            for (int k = 0; k <= i; ++k) t += w.l[i * n + k] * w.p[k * n + j];
            w.a[i * n + j] = t;
        }
    for (int i = 0; i < n; ++i)                           // (L P) L^T, upper triangle, mirrored
        for (int j = i; j < n; ++j) {
            double t = 0.0;
            for (int k = 0; k <= j; ++k) t += w.a[i * n + k] * w.l[j * n + k];
            const double val = (xs != nullptr) ? sym_at(xs, n, i, j) + t : t;
            out[i * n + j] = val;
            out[j * n + i] = val;
        }
}

SYMPA_HD void spd_exp_nan_row(double* __restrict__ out, int n) {
    for (int k = 0; k < n * n; ++k) out[k] = __builtin_nan("");
}

// One map of one pair: kind = SPD_MAP_EXP (p2 = u), SPD_MAP_LOG / SPD_MAP_GEODESIC (p2 = y).  out must not alias the inputs.
// A row whose x does not factor (or, for log / geodesic, whose y is not positive definite against x: a <= -1) is NaN + ST_NOT_PD.
SYMPA_HD void spd_map_row(SpdExpWork& w, int kind, const double* __restrict__ px, const double* __restrict__ p2, double t, int n,
                          double* __restrict__ out, int& status) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            w.a[i * n + j] = (kind == SPD_MAP_EXP) ? 0.5 * (p2[i * n + j] + p2[j * n + i]) : sym_at(p2, n, i, j) - sym_at(px, n, i, j);
    bool ok = spd_exp_spectrum(w, px, n, false, status);
    bool fin = true;
    for (int k = 0; k < n; ++k) {
        const double a = w.lam[k];
        if (kind == SPD_MAP_EXP) {
            w.f[k] = std::expm1(a);
        } else {
            ok = ok && (a > -1.0);
            const double lg = d_log1p_signed(a);
            w.f[k] = (kind == SPD_MAP_LOG) ? lg : std::expm1(t * lg);
        }
        fin = fin && d_finite(w.f[k]);
    }
    if (!ok) status |= ST_NOT_PD;
    if (ok && !fin) status |= ST_NONFINITE;
    if (!ok) { spd_exp_nan_row(out, n); return; }
    spd_exp_apply(w, kind == SPD_MAP_LOG ? nullptr : px, n, out);
}

// x <- expmap(x, -lr x S x) in place, S = coef sym(g) + wd x.  xs: n * n doubles of working storage for sym(x).
SYMPA_HD void spd_row_rsgd_exp(SpdExpWork& w, double* __restrict__ xs, double* __restrict__ px, const double* __restrict__ pg, int n,
                               double lr, double wd, double coef, int& status) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            xs[i * n + j] = 0.5 * (px[i * n + j] + px[j * n + i]);
            w.a[i * n + j] = 0.5 * coef * (pg[i * n + j] + pg[j * n + i]);
        }
    if (wd != 0.0)
        for (int k = 0; k < n * n; ++k) w.a[k] = d_fma(wd, xs[k], w.a[k]);
    const bool ok = spd_exp_spectrum(w, xs, n, true, status);
    bool fin = true;
    for (int k = 0; k < n; ++k) {
        w.f[k] = std::expm1(-lr * w.lam[k]);
        fin = fin && d_finite(w.f[k]);
    }
    if (ok && !fin) status |= ST_NONFINITE;
    if (!ok) { spd_exp_nan_row(px, n); return; }
    spd_exp_apply(w, xs, n, px);
}

}  // namespace sympa
