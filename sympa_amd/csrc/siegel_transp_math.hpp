// Per-row arithmetic of the parallel transport along geodesics of the upper and bounded Siegel models, compiled by hipcc
// (kernels: siegel_transp_kernel.hpp) and by g++ (tests/hostsim), on top of siegel_expmap_math.hpp, whose functions are used as
// they are.  The reference approximates: "The formula for the parallel transport is very complicated so we approximate it with
// the Euclidean parallel transport" (sympa/manifolds/siegel_manifold.py:142-154); SiegelManifold.transp keeps that identity.
//
// Transport of v from x along t -> expmap(x, t u) to y = expmap(x, u) is one congruence  v' = G v G^T  (both tangents
// symmetrised).  With the notation of siegel_expmap_math.hpp, h(t) = tanh(sqrt t) / sqrt t, M = sqrt(S S^H):
//   upper,   Im x = L L^T:          S = L^-1 u L^-T / (2i),  V = h(S S^H) S,  G = L (I - V)^-1 sech(M) L^-1
//   bounded, I - x conj x = C C^H:  S = C^-1 u C^-T,  V = h(S S^H) S,  Wt = C^-1 x conj(C),  G = C (I + V conj Wt)^-1 sech(M) C^-1
// (at the origin of the disc the transvection along S is [[cosh M, sinh(M) M^-1 S], [conj, conj]], its differential at 0 is
// dW -> sech(M) dW sech(M)^T; the rest is the differential, taken at V, of the isometry that carries 0 (upper: iI) to x; the
// Cayley factors 2i cancel).
//
// Evaluation.  expmap_row solves once, X = (I - V)^-1 V resp. (I + V conj Wt)^-1 V, and returns y = x + L [2i X] L^T resp.
// x + C X C^T.  The inverse itself follows from that X:  (I - V)^-1 = I + X,  (I + V conj Wt)^-1 = I - X conj(Wt).  So with
//   B = -X (upper),  B = X conj(Wt) (bounded),   G = L (I - B) sech(M) L^-1,   w = L^-1 v L^-T,
// one factor, one eigendecomposition and one solve serve y and v' together.  Two forms of the last step, chosen per row:
//   short step (every eigenvalue of S S^H below TRANSP_SHORT = 1/4, i.e. sigma_max < 1/2):
//       E = sech(M) - I (spectral),   K = E - B (I + E),   v' = v + L [K w + (K w)^T + (K w) K^T] L^T
//     u = 0 gives E = 0, X = 0, K = 0 and v' = sym(v) bit for bit, as expmap returns x, and a short step keeps the relative
//     accuracy of v' - v.  sech(s) - 1 = -2 sinh^2(s / 2) / cosh(s), below t = s^2 = 1e-4 the series.
//   long step:   Gh = (I - B) sech(M),   v' = L [Gh w Gh^T] L^T
//     -- along a long step G contracts some directions like exp(-sigma), and v + (v' - v) would cancel ||v|| / ||v'|| ~
//     exp(2 sigma) of its digits (measured: 7e4 eps kappa at |u| = 6, n = 1, bounded).
// Both are  A = F - B S,  T = A w,  v' = base + L [T A^T + extra] L^T  with (F, S, base, extra) = (E, I + E, sym v, T + T^T) for
// a short step and (sech, sech, 0, 0) for a long one: the same operations, a few selects.
//
// Between two points y is given, so X needs no solve: X = L^-1 (y - x) L^-T / (2i) resp. C^-1 (y - x) C^-T, which is the
// D' / (2i) of logmap_pair's V = D' (D' + 2i I)^-1.  sech(M) = (I - V V^H)^(1/2) = (I + G_)^(-1/2), G_ = E_ E_^H / 4 (upper) or
// E_ E_^H (bounded), E_ = L1^-1 (y - x) L2^-T the forward's matrix: sech = 1 / r, E = -gamma / (r (1 + r)), r = sqrt(1 + gamma),
// from the eigenvalues gamma of G_ and applied through its eigenvectors, as logmap_pair applies g; a short step is gamma < 1/4
// throughout.  No 1 - t, no atanh; y = x gives an exact 0.
//
// A tangent so long that tanh(sigma_max) rounds to 1 (sigma_max > 19.07) puts y on the boundary in fp64: ST_NOT_PD, set from
// the eigenvalue itself (I - V need not come out singular for a complex symmetric V of norm 1), next to what the solve reports.
// DESIGN.md section 25 has the error bounds with their measured constants.
#pragma once

#include "siegel_expmap_math.hpp"

namespace sympa {

// sech(sqrt t) - 1, t >= 0 (a rounding-negative t counts as 0); below 1e-4 the series (next term 1.4e-2 t^5: 3e-18 of the first)
SYMPA_HD double spec_sech_m1(double t) {
    t = fmax(t, 0.0);
    const bool small = t < 1e-4;
    const double series = t * d_fma(t, d_fma(t, d_fma(t, 277.0 / 8064.0, -61.0 / 720.0), 5.0 / 24.0), -0.5);
    const double x = small ? 1.0 : d_sqrt(t);
    const double sh = std::sinh(0.5 * x);
    return small ? series : -2.0 * sh * sh / std::cosh(x);
}

// the same as a function of gamma = sinh^2(M): (1 + gamma)^(-1/2) - 1
SYMPA_HD double spec_sech_m1_gamma(double gamma) {
    gamma = fmax(gamma, 0.0);
    const double r = d_sqrt(1.0 + gamma);
    return -gamma / (r * (1.0 + r));
}

// a step is short when every eigenvalue (of S S^H, or gamma = sinh^2 of it) is below this: sigma_max < 1/2 (header comment)
constexpr double TRANSP_SHORT = 0.25;

// tanh(s) = 1 in fp64 from s = 19.07 on (2 exp(-2 s) < 2^-54): t = s^2
constexpr double TRANSP_TANH_ONE = 363.6;

template <int N>
SYMPA_HD bool transp_short_step(const double (&lam)[N]) {
    bool s = true;
SYMPA_UNROLL
    for (int i = 0; i < N; ++i) s = s && (lam[i] < TRANSP_SHORT);
    return s;
}

// c = a * b^T (plain transpose)
template <int N>
SYMPA_HD void cmatmul_bt(const CMat<N>& a, const CMat<N>& b, CMat<N>& c) {
SYMPA_UNROLL
    for (int i = 0; i < N; ++i)
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) {
            double tr = 0.0, ti = 0.0;
SYMPA_UNROLL
            for (int k = 0; k < N; ++k) {
                tr = d_fma(a.re[i][k], b.re[j][k], tr);
                tr = d_fma(-a.im[i][k], b.im[j][k], tr);
                ti = d_fma(a.re[i][k], b.im[j][k], ti);
                ti = d_fma(a.im[i][k], b.re[j][k], ti);
            }
            c.re[i][j] = tr;
            c.im[i][j] = ti;
        }
}

// a = F - B S,  S = F + I for a short step (F = E, a = K) and S = F for a long one (F = sech, a = Gh)  (header comment)
template <int N>
SYMPA_HD void transp_generator(const CMat<N>& f, const CMat<N>& b, const bool short_step, CMat<N>& a) {
    CMat<N> sech = f;
SYMPA_UNROLL
    for (int i = 0; i < N; ++i) sech.re[i][i] += short_step ? 1.0 : 0.0;
    cmatmul<N>(b, sech, -1.0, a);
SYMPA_UNROLL
    for (int i = 0; i < N; ++i)
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) { a.re[i][j] += f.re[i][j]; a.im[i][j] += f.im[i][j]; }
}

// out = base + L [T A^T + extra] L^T,  T = A w,  w = L^-1 sym(v) L^-T;  (base, extra) = (sym v, T + T^T) for a short step, where
// a = K, and (0, 0) for a long one, where a = Gh:  (L G L^-1) sym(v) (L G L^-1)^T either way
template <int N, bool CPLX>
SYMPA_HD void transp_congruence(const Tri<N, CPLX>& l, const double (&diag)[N], const CMat<N>& a, const bool short_step,
                                const CMat<N>& v, CMat<N>& out) {
    out = v;
    symmetrise<N>(out);
    CMat<N> w = out, t, p;
    solve_left<N, CPLX>(l, w);
    solve_right_t<N, CPLX>(l, w);
    symmetrise<N>(w);
    cmatmul<N>(a, w, 1.0, t);
    cmatmul_bt<N>(t, a, p);
    const double keep = short_step ? 1.0 : 0.0;
SYMPA_UNROLL
    for (int i = 0; i < N; ++i)
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) {
            p.re[i][j] += keep * (t.re[i][j] + t.re[j][i]);
            p.im[i][j] += keep * (t.im[i][j] + t.im[j][i]);
        }
    symmetrise<N>(p);
    tri_mul_left<N, CPLX>(l, diag, p);
    tri_mul_right_t<N, CPLX>(l, diag, p);
SYMPA_UNROLL
    for (int i = 0; i < N; ++i)
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) {
            out.re[i][j] = (short_step ? out.re[i][j] : 0.0) + p.re[i][j];
            out.im[i][j] = (short_step ? out.im[i][j] : 0.0) + p.im[i][j];
        }
    symmetrise<N>(out);
}

// Wt = C^-1 W0 conj(C) of a symmetric point of the bounded model
template <int N>
SYMPA_HD void bounded_wt(const Tri<N, true>& l, const double (&diag)[N], const CMat<N>& w0, CMat<N>& wt) {
    wt = w0;
    solve_left<N, true>(l, wt);
    tri_mul_right_conj<N>(l, diag, wt);
    symmetrise<N>(wt);
}

// The shared body of the two tangent forms.  out_v = the transport of sym(v) along sym(u); WITH_Y: out_y = expmap_z(u), by the
// operations of expmap_row in their order.  u is used as workspace.
template <int N, int MODEL, bool WITH_Y>
SYMPA_HD void transp_exp_body(const CMat<N>& z, CMat<N>& u, const CMat<N>& v, CMat<N>& out_y, CMat<N>& out_v, int& status) {
    static_assert(MODEL == MODEL_UPPER || MODEL == MODEL_BOUNDED, "the compact dual has no inner product (compact_dual.py:96)");
    constexpr bool CPLX = (MODEL == MODEL_BOUNDED);
    CMat<N> x = z;
    symmetrise<N>(x);
    symmetrise<N>(u);
    Tri<N, CPLX> l;
    bool ok;
    if constexpr (CPLX) ok = chol_id_minus_wwh<N>(x, l);
    else ok = chol_real<N>(x.im, l);
    double diag[N];
    tri_diag<N, CPLX>(l, diag);
    solve_left<N, CPLX>(l, u);
    solve_right_t<N, CPLX>(l, u);
    CMat<N> s, xs, a, e, k;
    if constexpr (CPLX) {
        s = u;
    } else {
SYMPA_UNROLL
        for (int i = 0; i < N; ++i)
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) { s.re[i][j] = 0.5 * u.im[i][j]; s.im[i][j] = -0.5 * u.re[i][j]; }      // T / (2i)
    }
    symmetrise<N>(s);
    bool conv, short_step;
    {
        // V = h(S S^H) S and E = sech(M) - I (a long step: sech(M)) from one eigendecomposition
        Herm<N> h;
        gram_rows<N>(s, h);
        CMat<N> q, m;
        conv = herm_eig<N>(h, q);
        double f[N], g[N];
        short_step = transp_short_step<N>(h.d);
SYMPA_UNROLL
        for (int i = 0; i < N; ++i) {
            f[i] = spec_tanh_ratio(h.d[i]);
            ok = ok && (h.d[i] < TRANSP_TANH_ONE);
            g[i] = short_step ? spec_sech_m1(h.d[i]) : 1.0 / std::cosh(d_sqrt(fmax(h.d[i], 0.0)));
        }
        herm_from_eig<N>(q, f, m);
        cmatmul<N>(m, s, 1.0, xs);
        symmetrise<N>(xs);
        herm_from_eig<N>(q, g, e);
    }
    CMat<N> wt;
    if constexpr (CPLX) {
        bounded_wt<N>(l, diag, x, wt);
        cmatmul_bh<N>(xs, wt, 1.0, a);                                   // V conj(Wt) = V Wt^H  (Wt symmetric)
    } else {
SYMPA_UNROLL
        for (int i = 0; i < N; ++i)
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) { a.re[i][j] = -xs.re[i][j]; a.im[i][j] = -xs.im[i][j]; }                // I - V
    }
SYMPA_UNROLL
    for (int i = 0; i < N; ++i) a.re[i][i] += 1.0;
    ok = csolve_nopivot<N>(a, xs) && ok;                                 // X
    if constexpr (CPLX) {
        cmatmul_bh<N>(xs, wt, 1.0, a);                                   // B = X conj(Wt)
    } else {
SYMPA_UNROLL
        for (int i = 0; i < N; ++i)
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) { a.re[i][j] = -xs.re[i][j]; a.im[i][j] = -xs.im[i][j]; }                // B = -X
    }
    transp_generator<N>(e, a, short_step, k);
    transp_congruence<N, CPLX>(l, diag, k, short_step, v, out_v);
    bool finite = cmat_finite<N>(out_v);
    if constexpr (WITH_Y) {
        if constexpr (!CPLX) {
SYMPA_UNROLL
            for (int i = 0; i < N; ++i)
SYMPA_UNROLL
                for (int j = 0; j < N; ++j) {                                                                   // times 2i
                    const double r = xs.re[i][j];
                    xs.re[i][j] = -2.0 * xs.im[i][j];
                    xs.im[i][j] = 2.0 * r;
                }
        }
        tri_mul_left<N, CPLX>(l, diag, xs);
        tri_mul_right_t<N, CPLX>(l, diag, xs);
SYMPA_UNROLL
        for (int i = 0; i < N; ++i)
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) { out_y.re[i][j] = x.re[i][j] + xs.re[i][j]; out_y.im[i][j] = x.im[i][j] + xs.im[i][j]; }
        symmetrise<N>(out_y);
        finite = finite && cmat_finite<N>(out_y);
    }
    if (!ok) status |= ST_NOT_PD;
    if (!conv) status |= ST_NO_CONVERGENCE;
    if (!finite) status |= ST_NONFINITE;
}

// out_v = sym(v) transported from z along t -> expmap(z, t u) to expmap(z, u); u is used as workspace
template <int N, int MODEL>
SYMPA_HD void transp_exp_row(const CMat<N>& z, CMat<N>& u, const CMat<N>& v, CMat<N>& out_v, int& status) {
    transp_exp_body<N, MODEL, false>(z, u, v, out_v, out_v, status);
}

// the same, and out_y = expmap(z, u): factor, eigendecomposition and solve are those of the transport
template <int N, int MODEL>
SYMPA_HD void expmap_transp_row(const CMat<N>& z, CMat<N>& u, const CMat<N>& v, CMat<N>& out_y, CMat<N>& out_v, int& status) {
    transp_exp_body<N, MODEL, true>(z, u, v, out_y, out_v, status);
}

// out_v = sym(v) transported from z1 to z2 along the geodesic between them
template <int N, int MODEL>
SYMPA_HD void transp_pair(const CMat<N>& z1, const CMat<N>& z2, const CMat<N>& v, CMat<N>& out_v, int& status) {
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
    CMat<N> e, xs, b, em, k;
SYMPA_UNROLL
    for (int i = 0; i < N; ++i)
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) {
            e.re[i][j] = x2.re[i][j] - x1.re[i][j];
            e.im[i][j] = x2.im[i][j] - x1.im[i][j];
        }
    solve_left<N, CPLX>(l1, e);
    xs = e;
    solve_right_t<N, CPLX>(l1, xs);
    symmetrise<N>(xs);                               // D' = L1^-1 (z2 - z1) L1^-T
    if constexpr (CPLX) {
        CMat<N> wt;
        bounded_wt<N>(l1, diag, x1, wt);
        cmatmul_bh<N>(xs, wt, 1.0, b);               // B = X conj(Wt),  X = D'
    } else {
SYMPA_UNROLL
        for (int i = 0; i < N; ++i)
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) { b.re[i][j] = -0.5 * xs.im[i][j]; b.im[i][j] = 0.5 * xs.re[i][j]; }    // B = -X,  X = D' / (2i)
    }
    solve_right_t<N, CPLX>(l2, e);                   // E_, the forward's matrix
    Herm<N> h;
    gram_rows<N>(e, h);
    CMat<N> q;
    const bool conv = herm_eig<N>(h, q);
    if constexpr (N >= 5) {
        // Rayleigh quotients lambda_i = ||E_^H q_i||^2, as logmap_pair takes them
SYMPA_UNROLL
        for (int c = 0; c < N; ++c) {
            double acc = 0.0;
SYMPA_UNROLL
            for (int r = 0; r < N; ++r) {
                double tr = 0.0, ti = 0.0;           // sum_k conj(e_kr) q_kc
SYMPA_UNROLL
                for (int kk = 0; kk < N; ++kk) {
                    tr = d_fma(e.re[kk][r], q.re[kk][c], d_fma(e.im[kk][r], q.im[kk][c], tr));
                    ti = d_fma(e.re[kk][r], q.im[kk][c], d_fma(-e.im[kk][r], q.re[kk][c], ti));
                }
                acc = d_fma(tr, tr, d_fma(ti, ti, acc));
            }
            h.d[c] = acc;
        }
    }
    double g[N];
SYMPA_UNROLL
    for (int i = 0; i < N; ++i) g[i] = CPLX ? h.d[i] : 0.25 * h.d[i];
    const bool short_step = transp_short_step<N>(g);
SYMPA_UNROLL
    for (int i = 0; i < N; ++i) g[i] = short_step ? spec_sech_m1_gamma(g[i]) : d_rsqrt(1.0 + fmax(g[i], 0.0));
    herm_from_eig<N>(q, g, em);
    transp_generator<N>(em, b, short_step, k);
    transp_congruence<N, CPLX>(l1, diag, k, short_step, v, out_v);
    if (!ok) status |= ST_NOT_PD;
    if (!conv) status |= ST_NO_CONVERGENCE;
    if (!cmat_finite<N>(out_v)) status |= ST_NONFINITE;
}

}  // namespace sympa
