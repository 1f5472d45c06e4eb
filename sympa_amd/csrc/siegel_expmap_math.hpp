// Per-row arithmetic of the exponential and logarithm maps of the upper and bounded Siegel models and of the RiemannianSGD
// step that moves along the geodesic, compiled by hipcc (kernels: siegel_expmap_kernel.hpp) and by g++ (tests/hostsim), like
// siegel_table_math.hpp.  The reference leaves both maps empty (sympa/manifolds/siegel_manifold.py:156-162, "We might not need
// it") and retracts linearly ("Simple retraction: x + u. Correct retraction: exp_map(u)", siegel_manifold.py:74-87).
//
// The maps belong to the invariant metric of the model; the `riem` distance measures c times that metric's length, c = 1
// (upper), c = 2 (bounded):   dist(x, expmap(x, u)) = c |u|_x.   upper: |u|_x^2 = inner(x, u, u) = tangent_sqnorm<N, MODEL_UPPER>;
// bounded: |u|_x^2 = |C^-1 u C^-T|_F^2 = inner(x, conj u, conj u), NOT inner(x, u, u) (see below, after the solve route).
// Tangent vectors are complex symmetric; both maps act on sym(u).
//
// Spectral functions  h(t) = tanh(sqrt t) / sqrt t,  g(t) = atanh(sqrt t) / sqrt t  of a Hermitian matrix through its
// eigendecomposition (matrix functions: the arbitrary basis inside a cluster of eigenvalues does not matter).
//
// upper,  Z = X + iY,  Y = L L^T:
//   exp:  S = L^-1 U L^-T / (2i),  V = h(S S^H) S  (complex symmetric, ||V|| = tanh sigma_max(S) < 1),
//         expmap = X + L [i (I + V)(I - V)^-1] L^T = Z + L [2i (I - V)^-1 V] L^T
//         (the second form: u = 0 returns Z bit for bit, and a small u keeps its relative accuracy)
//   log:  D' = L1^-1 (Z2 - Z1) L1^-T,  V = D' (D' + 2i I)^-1  (= L1^-1 (Z2 - Z1)(Z2 - conj Z1)^-1 L1; an exact 0 for Z2 = Z1),
//         logmap = L1 [2i g(V V^H) V] L1^T
// bounded,  A = I - W0 conj(W0) = C C^H,  Wt = C^-1 W0 conj(C)  (complex symmetric, the singular values of W0):
//   exp:  S = C^-1 U C^-T,  V = h(S S^H) S,
//         expmap = (I + P conj W0)^-1 (P + W0),  P = C V conj(C)^-1
//                = W0 + C [(I + V conj Wt)^-1 V] C^T
//         (same point: I + P conj(W0) = C (I + V conj Wt) C^-1,  P + W0 = C (V + Wt) conj(C)^-1,  I - conj(Wt) Wt = C^T conj(C);
//          u = 0 returns W0 bit for bit, conj(C)^-1 is never applied)
//   log:  V = C1^-1 (W - W0)(I - conj(W0) W)^-1 conj(C1),  logmap = C1 [g(V V^H) V] C1^T
// g at far pairs needs 1 - t for t -> 1.  V V^H = G (I + G)^-1 with G = E E^H / 4 (upper) or E E^H (bounded), E = L1^-1 (Z2 - Z1)
// L2^-T the forward's own matrix: g is evaluated from the eigenvalues gamma of G as asinh(sqrt gamma) sqrt(1 + gamma) / sqrt gamma
// (= (v / 2) / tanh(v / 2), v = 2 asinh sqrt gamma), with the relative accuracy the forward has, and applied through the
// eigenvectors of E E^H.
//
// General complex solves: Gaussian elimination WITHOUT pivoting (csolve_nopivot), on matrices whose Hermitian part is positive
// definite -- for those every pivot has a positive real part and the factors are bounded by
// || |L||U| ||_F <= n (||T|| + ||K T^-1 K||), T / K the Hermitian / skew-Hermitian part (Golub & Van Loan, Matrix Computations,
// section 4.2 on unsymmetric positive definite systems; Mathias 1992 for the complex case):
//   I - V,  I + V conj(Wt),  I - W conj(W0):   I + (a contraction): T >= 1 - ||.|| > 0, ||K|| < 1;
//   (D' + 2i I) / i = (Im D' + 2 I) - i Re D':   T = L1^-1 Y2 L1^-T + I >= I,  K = -i Re D'.
// A tangent so long that tanh(sigma) rounds to 1 (sigma > 19) makes I - V singular: ST_NOT_PD / ST_NONFINITE.
// The metric: |u|^2 = inner(x, u, u) for upper; for bounded |C^-1 u C^-T|_F^2 = inner(x, conj u, conj u) -- the reference's bounded
// inner has its two inverses the other way round (tangent_sqnorm<N, MODEL_BOUNDED>, left as it is).
// DESIGN.md section 24 has the error bounds with their measured constants.
#pragma once

#include "siegel_table_math.hpp"

namespace sympa {

// h(t) = tanh(sqrt t) / sqrt t, t >= 0 (a rounding-negative t counts as 0); below 1e-4 the series (next term 2e-18)
SYMPA_HD double spec_tanh_ratio(double t) {
    t = fmax(t, 0.0);
    const bool small = t < 1e-4;
    const double series = d_fma(t, d_fma(t, d_fma(t, -17.0 / 315.0, 2.0 / 15.0), -1.0 / 3.0), 1.0);
    const double x = small ? 1.0 : d_sqrt(t);
    return small ? series : std::tanh(x) / x;
}

// g as a function of gamma = t / (1 - t) = sinh^2(v / 2):  asinh(s) sqrt(1 + gamma) / s, s = sqrt gamma
SYMPA_HD double spec_atanh_ratio_gamma(double gamma) {
    gamma = fmax(gamma, 0.0);
    const bool small = gamma < 1e-4;
    const double series = d_fma(gamma, d_fma(gamma, d_fma(gamma, -15.0 / 336.0, 3.0 / 40.0), -1.0 / 6.0), 1.0);
    const double s = small ? 1.0 : d_sqrt(gamma);
    return (small ? series : std::asinh(s) / s) * d_sqrt(1.0 + gamma);
}

template <int N, bool COMPLEX>
SYMPA_HD void tri_diag(const Tri<N, COMPLEX>& l, double (&diag)[N]) {
SYMPA_UNROLL
    for (int i = 0; i < N; ++i) diag[i] = d_rcp(l.rdiag[i]);
}

// x <- L x  (rows from the bottom: row i reads the rows above it)
template <int N, bool COMPLEX>
SYMPA_HD void tri_mul_left(const Tri<N, COMPLEX>& l, const double (&diag)[N], CMat<N>& x) {
SYMPA_UNROLL
    for (int c = 0; c < N; ++c) {
SYMPA_UNROLL
        for (int i = N - 1; i >= 0; --i) {
            double tr = diag[i] * x.re[i][c], ti = diag[i] * x.im[i][c];
SYMPA_UNROLL
            for (int k = 0; k < i; ++k) {
                tr = d_fma(l.re[i][k], x.re[k][c], tr);
                ti = d_fma(l.re[i][k], x.im[k][c], ti);
                if (COMPLEX) {
                    tr = d_fma(-l.im[i][k], x.im[k][c], tr);
                    ti = d_fma(l.im[i][k], x.re[k][c], ti);
                }
            }
            x.re[i][c] = tr;
            x.im[i][c] = ti;
        }
    }
}

// x <- x L^T  (plain transpose; columns from the right)
template <int N, bool COMPLEX>
SYMPA_HD void tri_mul_right_t(const Tri<N, COMPLEX>& l, const double (&diag)[N], CMat<N>& x) {
SYMPA_UNROLL
    for (int r = 0; r < N; ++r) {
SYMPA_UNROLL
        for (int j = N - 1; j >= 0; --j) {
            double tr = diag[j] * x.re[r][j], ti = diag[j] * x.im[r][j];
SYMPA_UNROLL
            for (int k = 0; k < j; ++k) {
                tr = d_fma(x.re[r][k], l.re[j][k], tr);
                ti = d_fma(x.im[r][k], l.re[j][k], ti);
                if (COMPLEX) {
                    tr = d_fma(-x.im[r][k], l.im[j][k], tr);
                    ti = d_fma(x.re[r][k], l.im[j][k], ti);
                }
            }
            x.re[r][j] = tr;
            x.im[r][j] = ti;
        }
    }
}

// x <- x conj(L)  (columns from the left)
template <int N>
SYMPA_HD void tri_mul_right_conj(const Tri<N, true>& l, const double (&diag)[N], CMat<N>& x) {
SYMPA_UNROLL
    for (int r = 0; r < N; ++r) {
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) {
            double tr = diag[j] * x.re[r][j], ti = diag[j] * x.im[r][j];
SYMPA_UNROLL
            for (int k = j + 1; k < N; ++k) {       // x_rk conj(L_kj)
                tr = d_fma(x.re[r][k], l.re[k][j], tr);
                tr = d_fma(x.im[r][k], l.im[k][j], tr);
                ti = d_fma(x.im[r][k], l.re[k][j], ti);
                ti = d_fma(-x.re[r][k], l.im[k][j], ti);
            }
            x.re[r][j] = tr;
            x.im[r][j] = ti;
        }
    }
}

// b <- a^-1 b by Gaussian elimination without pivoting (a is destroyed); for matrices with a positive definite Hermitian part
// (header comment).  Returns false when a pivot's real part is not positive (the argument left the domain, or is not finite).
template <int N>
SYMPA_HD bool csolve_nopivot(CMat<N>& a, CMat<N>& b) {
    bool ok = true;
SYMPA_UNROLL
    for (int k = 0; k < N; ++k) {
        const double pr = a.re[k][k], pi = a.im[k][k];
        ok = ok && (pr > 0.0);
        const double inv = d_rcp(d_fma(pr, pr, pi * pi));
        const double ir = pr * inv, ii = -(pi * inv);                  // 1 / pivot
SYMPA_UNROLL
        for (int j = k + 1; j < N; ++j) {
            const double xr = a.re[k][j], xi = a.im[k][j];
            a.re[k][j] = d_fma(xr, ir, -(xi * ii));
            a.im[k][j] = d_fma(xr, ii, xi * ir);
        }
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) {
            const double xr = b.re[k][j], xi = b.im[k][j];
            b.re[k][j] = d_fma(xr, ir, -(xi * ii));
            b.im[k][j] = d_fma(xr, ii, xi * ir);
        }
SYMPA_UNROLL
        for (int i = k + 1; i < N; ++i) {
            const double fr = a.re[i][k], fi = a.im[i][k];
SYMPA_UNROLL
            for (int j = k + 1; j < N; ++j) {
                a.re[i][j] = d_fma(-fr, a.re[k][j], d_fma(fi, a.im[k][j], a.re[i][j]));
                a.im[i][j] = d_fma(-fr, a.im[k][j], d_fma(-fi, a.re[k][j], a.im[i][j]));
            }
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) {
                b.re[i][j] = d_fma(-fr, b.re[k][j], d_fma(fi, b.im[k][j], b.re[i][j]));
                b.im[i][j] = d_fma(-fr, b.im[k][j], d_fma(-fi, b.re[k][j], b.im[i][j]));
            }
        }
    }
    // unit upper triangle left in a: back substitution
SYMPA_UNROLL
    for (int k = N - 1; k > 0; --k) {
SYMPA_UNROLL
        for (int i = 0; i < k; ++i) {
            const double fr = a.re[i][k], fi = a.im[i][k];
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) {
                b.re[i][j] = d_fma(-fr, b.re[k][j], d_fma(fi, b.im[k][j], b.re[i][j]));
                b.im[i][j] = d_fma(-fr, b.im[k][j], d_fma(-fi, b.re[k][j], b.im[i][j]));
            }
        }
    }
    return ok;
}

// H = E E^H (gram<N> forms E^H E)
template <int N>
SYMPA_HD void gram_rows(const CMat<N>& e, Herm<N>& h) {
SYMPA_UNROLL
    for (int j = 0; j < N; ++j) {
        double s = 0.0;
SYMPA_UNROLL
        for (int i = 0; i < N; ++i) {
            s = d_fma(e.re[j][i], e.re[j][i], s);
            s = d_fma(e.im[j][i], e.im[j][i], s);
        }
        h.d[j] = s;
SYMPA_UNROLL
        for (int k = j + 1; k < N; ++k) {
            double tr = 0.0, ti = 0.0;   // sum_i e_ji conj(e_ki)
SYMPA_UNROLL
            for (int i = 0; i < N; ++i) {
                tr = d_fma(e.re[j][i], e.re[k][i], tr);
                tr = d_fma(e.im[j][i], e.im[k][i], tr);
                ti = d_fma(e.im[j][i], e.re[k][i], ti);
                ti = d_fma(-e.re[j][i], e.im[k][i], ti);
            }
            h.re[j][k] = tr;
            h.im[j][k] = ti;
        }
    }
}

// eigenvalues into h.d, eigenvectors into the columns of q: Jacobi up to n = 4, tridiagonal QL above (as the backward)
template <int N>
SYMPA_HD bool herm_eig(Herm<N>& h, CMat<N>& q) {
    if constexpr (N >= 5) return herm_eigen_vectors_ql<N>(h, q);
    else return herm_eigen_vectors<N>(h, q);
}

template <int N>
SYMPA_HD bool cmat_finite(const CMat<N>& z) {
    bool f = true;
SYMPA_UNROLL
    for (int i = 0; i < N; ++i)
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) f = f && d_finite(z.re[i][j]) && d_finite(z.im[i][j]);
    return f;
}

// v <- h(s s^H) s for a complex symmetric s (v comes out symmetrised)
template <int N>
SYMPA_HD bool tanh_ratio_apply(const CMat<N>& s, CMat<N>& v) {
    Herm<N> h;
    gram_rows<N>(s, h);
    CMat<N> q, m;
    const bool conv = herm_eig<N>(h, q);
    double f[N];
SYMPA_UNROLL
    for (int i = 0; i < N; ++i) f[i] = spec_tanh_ratio(h.d[i]);
    herm_from_eig<N>(q, f, m);
    cmatmul<N>(m, s, 1.0, v);
    symmetrise<N>(v);
    return conv;
}

// out = expmap_z(u) on sym(z), sym(u); u is used as workspace.  Pure: no clamp.
template <int N, int MODEL>
SYMPA_HD void expmap_row(const CMat<N>& z, CMat<N>& u, CMat<N>& out, int& status) {
    static_assert(MODEL == MODEL_UPPER || MODEL == MODEL_BOUNDED, "the compact dual has no inner product (compact_dual.py:96)");
    constexpr bool CPLX = (MODEL == MODEL_BOUNDED);
    out = z;
    symmetrise<N>(out);
    symmetrise<N>(u);
    Tri<N, CPLX> l;
    bool ok;
    if constexpr (CPLX) ok = chol_id_minus_wwh<N>(out, l);
    else ok = chol_real<N>(out.im, l);
    double diag[N];
    tri_diag<N, CPLX>(l, diag);
    solve_left<N, CPLX>(l, u);
    solve_right_t<N, CPLX>(l, u);
    CMat<N> s, v, a;
    if constexpr (CPLX) {
        s = u;
    } else {
SYMPA_UNROLL
        for (int i = 0; i < N; ++i)
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) { s.re[i][j] = 0.5 * u.im[i][j]; s.im[i][j] = -0.5 * u.re[i][j]; }      // T / (2i)
    }
    symmetrise<N>(s);
    const bool conv = tanh_ratio_apply<N>(s, v);
    if constexpr (CPLX) {
        // Wt = C^-1 W0 conj(C);  a = I + V conj(Wt) = I + V Wt^H  (Wt symmetric)
        CMat<N> wt = out;
        solve_left<N, true>(l, wt);
        tri_mul_right_conj<N>(l, diag, wt);
        symmetrise<N>(wt);
        cmatmul_bh<N>(v, wt, 1.0, a);
    } else {
SYMPA_UNROLL
        for (int i = 0; i < N; ++i)
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) { a.re[i][j] = -v.re[i][j]; a.im[i][j] = -v.im[i][j]; }                  // I - V
    }
SYMPA_UNROLL
    for (int i = 0; i < N; ++i) a.re[i][i] += 1.0;
    ok = csolve_nopivot<N>(a, v) && ok;
    if constexpr (!CPLX) {
SYMPA_UNROLL
        for (int i = 0; i < N; ++i)
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) {                                                                       // times 2i
                const double r = v.re[i][j];
                v.re[i][j] = -2.0 * v.im[i][j];
                v.im[i][j] = 2.0 * r;
            }
    }
    tri_mul_left<N, CPLX>(l, diag, v);
    tri_mul_right_t<N, CPLX>(l, diag, v);
SYMPA_UNROLL
    for (int i = 0; i < N; ++i)
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) { out.re[i][j] += v.re[i][j]; out.im[i][j] += v.im[i][j]; }
    symmetrise<N>(out);
    if (!ok) status |= ST_NOT_PD;
    if (!conv) status |= ST_NO_CONVERGENCE;
    if (!cmat_finite<N>(out)) status |= ST_NONFINITE;
}

// out = logmap_z1(z2) on sym(z1), sym(z2): the tangent vector at z1 whose geodesic reaches z2 at time 1
template <int N, int MODEL>
SYMPA_HD void logmap_pair(const CMat<N>& z1, const CMat<N>& z2, CMat<N>& out, int& status) {
    static_assert(MODEL == MODEL_UPPER || MODEL == MODEL_BOUNDED, "the compact dual has no inner product (compact_dual.py:96)");
    constexpr bool CPLX = (MODEL == MODEL_BOUNDED);
    CMat<N> x1 = z1, x2 = z2;
    symmetrise<N>(x1);
    symmetrise<N>(x2);
    Tri<N, CPLX> l1, l2;
    bool ok;
    if constexpr (CPLX) {
        ok = chol_id_minus_wwh<N>(x1, l1);
        ok = chol_id_minus_wwh<N>(x2, l2) && ok;
    } else {
        ok = chol_real<N>(x1.im, l1);
        ok = chol_real<N>(x2.im, l2) && ok;
    }
    double diag[N];
    tri_diag<N, CPLX>(l1, diag);
    CMat<N> d, e, v;
SYMPA_UNROLL
    for (int i = 0; i < N; ++i)
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) {
            d.re[i][j] = x2.re[i][j] - x1.re[i][j];
            d.im[i][j] = x2.im[i][j] - x1.im[i][j];
        }
    e = d;
    solve_left<N, CPLX>(l1, e);
    if constexpr (CPLX) {
        // K = (I - W conj(W0))^-1 (W - W0);  V = C1^-1 K^T conj(C1)
        CMat<N> a;
        cmatmul_bh<N>(x2, x1, -1.0, a);              // -W W0^H = -W conj(W0)  (W0 symmetric)
SYMPA_UNROLL
        for (int i = 0; i < N; ++i) a.re[i][i] += 1.0;
        ok = csolve_nopivot<N>(a, d) && ok;
SYMPA_UNROLL
        for (int i = 0; i < N; ++i)
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) { v.re[i][j] = d.re[j][i]; v.im[i][j] = d.im[j][i]; }
        solve_left<N, true>(l1, v);
        tri_mul_right_conj<N>(l1, diag, v);
    } else {
        // D' = L1^-1 (Z2 - Z1) L1^-T;  V = D' (D' + 2i I)^-1 = [((Im D' + 2 I) - i Re D')^-1 (Im D' - i Re D')]^T
        CMat<N> a;
        d = e;
        solve_right_t<N, false>(l1, d);
        symmetrise<N>(d);
SYMPA_UNROLL
        for (int i = 0; i < N; ++i)
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) {
                a.re[i][j] = d.im[i][j] + ((i == j) ? 2.0 : 0.0);
                a.im[i][j] = -d.re[i][j];
                v.re[i][j] = d.im[i][j];
                v.im[i][j] = -d.re[i][j];
            }
        ok = csolve_nopivot<N>(a, v) && ok;
    }
    symmetrise<N>(v);                                // V is symmetric: the transpose of the solve is taken here
    solve_right_t<N, CPLX>(l2, e);                   // E, the forward's matrix
    Herm<N> h;
    gram_rows<N>(e, h);
    CMat<N> q, m;
    const bool conv = herm_eig<N>(h, q);
    if constexpr (N >= 5) {
        // Rayleigh quotients lambda_i = ||E^H q_i||^2: relative accuracy for the small eigenvalues (as the backward does)
SYMPA_UNROLL
        for (int c = 0; c < N; ++c) {
            double acc = 0.0;
SYMPA_UNROLL
            for (int r = 0; r < N; ++r) {
                double tr = 0.0, ti = 0.0;           // sum_k conj(e_kr) q_kc
SYMPA_UNROLL
                for (int k = 0; k < N; ++k) {
                    tr = d_fma(e.re[k][r], q.re[k][c], d_fma(e.im[k][r], q.im[k][c], tr));
                    ti = d_fma(e.re[k][r], q.im[k][c], d_fma(-e.im[k][r], q.re[k][c], ti));
                }
                acc = d_fma(tr, tr, d_fma(ti, ti, acc));
            }
            h.d[c] = acc;
        }
    }
    double f[N];
SYMPA_UNROLL
    for (int i = 0; i < N; ++i) f[i] = spec_atanh_ratio_gamma(CPLX ? h.d[i] : 0.25 * h.d[i]);
    herm_from_eig<N>(q, f, m);
    cmatmul<N>(m, v, 1.0, out);
    if constexpr (!CPLX) {
SYMPA_UNROLL
        for (int i = 0; i < N; ++i)
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) {                                                                       // times 2i
                const double r = out.re[i][j];
                out.re[i][j] = -2.0 * out.im[i][j];
                out.im[i][j] = 2.0 * r;
            }
    }
    tri_mul_left<N, CPLX>(l1, diag, out);
    tri_mul_right_t<N, CPLX>(l1, diag, out);
    symmetrise<N>(out);
    if (!ok) status |= ST_NOT_PD;
    if (!conv) status |= ST_NO_CONVERGENCE;
    if (!cmat_finite<N>(out)) status |= ST_NONFINITE;
}

// One RiemannianSGD step along the geodesic:  x <- projx(expmap(x, -lr * egrad2rgrad(x, grad + wd x))).
// Returns true when projx moved the point (the exponential map stays inside the domain; the clamp keeps the eps-interior).
template <int N, int MODEL>
SYMPA_HD bool rsgd_exp_row(CMat<N>& z, const CMat<N>& grad, double lr, double weight_decay, double eps, int& status) {
    CMat<N> g, r;
SYMPA_UNROLL
    for (int i = 0; i < N; ++i)
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) {
            g.re[i][j] = d_fma(weight_decay, z.re[i][j], grad.re[i][j]);
            g.im[i][j] = d_fma(weight_decay, z.im[i][j], grad.im[i][j]);
        }
    egrad2rgrad<N, MODEL>(z, g, r);
SYMPA_UNROLL
    for (int i = 0; i < N; ++i)
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) { r.re[i][j] *= -lr; r.im[i][j] *= -lr; }
    expmap_row<N, MODEL>(z, r, g, status);
    z = g;
    return projx<N, MODEL>(z, eps, status);
}

}  // namespace sympa
