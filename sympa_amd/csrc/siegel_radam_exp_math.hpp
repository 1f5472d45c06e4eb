// Per-row arithmetic of the RiemannianAdam step that moves along the geodesic and carries exp_avg by the parallel transport,
// upper and bounded Siegel models, compiled by hipcc (kernels: siegel_radam_exp_kernel.hpp) and by g++ (tests/hostsim), on top
// of siegel_transp_math.hpp, whose functions are used as they are:
//     g     = sym(egrad2rgrad(x, coef * grad + wd x))          (the bounded A G A is not symmetric; the maps act on symmetric tangents)
//     m1    = b1 sym(m) + (1 - b1) g
//     s1    = b2 s + (1 - b2) |g|_x^2                          (one s per row)
//     alpha = lr / ((1 - b1^t) (sqrt(s1 / (1 - b2^t)) + eps_adam))
//     (y, m') = expmap_transp_row(x, -alpha m1, m1)            (one factor, one eigendecomposition and one solve serve both)
//     x <- projx(y, eps),   exp_avg <- m',   exp_avg_sq <- s1
// |.|_x is the INVARIANT norm, the one the maps and the transport belong to (siegel_expmap_math.hpp): upper |L^-1 g L^-T|_F^2
// = tangent_sqnorm<N, MODEL_UPPER>; bounded |C^-1 g C^-T|_F^2, which is NOT tangent_sqnorm<N, MODEL_BOUNDED> (that one is the norm
// of conj g).  With it the first step has the invariant length lr |g|_x / (|g|_x + eps_adam): Adam's unit step.
// When projx moves the row, m' stays as transported to y: the tangent spaces of the open domain are one vector space.
// The velocity is parallel to the transported vector; no form special to that case is taken, and the norm factors the point
// on its own (a shared factor would have to leave every bit of expmap_transp_row alone; the factor is a small part of the row).
// grad = 0 on m = 0, s = 0: alpha = lr / ((1 - b1^t) eps_adam) is finite, u = 0 takes the short form: sym(x) bit for bit, m' = 0,
// s1 = 0.  lr = 0: sym(x) and m1 bit for bit.  DESIGN.md section 26 has the error bounds with their measured constants.
#pragma once

#include "siegel_transp_math.hpp"

namespace sympa {

// |g|_x^2 of the invariant metric for a symmetric tangent g (header comment)
template <int N, int MODEL>
SYMPA_HD double invariant_sqnorm(const CMat<N>& x, const CMat<N>& g, int& status) {
    static_assert(MODEL == MODEL_UPPER || MODEL == MODEL_BOUNDED, "the compact dual has no inner product (compact_dual.py:96)");
    if constexpr (MODEL == MODEL_UPPER) {
        return tangent_sqnorm<N, MODEL_UPPER>(x, g, status);
    } else {
        Tri<N, true> c;
        const bool ok = chol_id_minus_wwh<N>(x, c);
        CMat<N> e = g;
        solve_left<N, true>(c, e);
        solve_right_t<N, true>(c, e);
        double acc = 0.0;
SYMPA_UNROLL
        for (int i = 0; i < N; ++i)
SYMPA_UNROLL
            for (int j = 0; j < N; ++j) acc = d_fma(e.re[i][j], e.re[i][j], d_fma(e.im[i][j], e.im[i][j], acc));
        if (!ok) status |= ST_NOT_PD;
        return acc;
    }
}

// In: x = the point, g = the Euclidean gradient row, m = exp_avg, s_old = exp_avg_sq.  Out: x = the new point, g = the new
// exp_avg, s_new = the new exp_avg_sq; returns true when projx moved the point.  pow1 = b1^t, pow2 = b2^t, coef = the clip factor.
template <int N, int MODEL>
SYMPA_HD bool radam_exp_row(CMat<N>& x, CMat<N>& g, const CMat<N>& m, const double s_old, double& s_new, double lr, double b1,
                            double b2, double eps_adam, double wd, double pow1, double pow2, double coef, double eps, int& status) {
    CMat<N> r, m1, u, y;
SYMPA_UNROLL
    for (int i = 0; i < N; ++i)
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) {
            g.re[i][j] = d_fma(wd, x.re[i][j], coef * g.re[i][j]);
            g.im[i][j] = d_fma(wd, x.im[i][j], coef * g.im[i][j]);
        }
    egrad2rgrad<N, MODEL>(x, g, r);
    symmetrise<N>(r);
    const double sq = invariant_sqnorm<N, MODEL>(x, r, status);
    s_new = d_fma(b2, s_old, (1.0 - b2) * sq);
    const double bc1 = 1.0 - pow1, bc2 = 1.0 - pow2;
    const double alpha = lr / (bc1 * (sqrt(s_new / bc2) + eps_adam));
    m1 = m;
    symmetrise<N>(m1);
SYMPA_UNROLL
    for (int i = 0; i < N; ++i)
SYMPA_UNROLL
        for (int j = 0; j < N; ++j) {
            m1.re[i][j] = d_fma(b1, m1.re[i][j], (1.0 - b1) * r.re[i][j]);
            m1.im[i][j] = d_fma(b1, m1.im[i][j], (1.0 - b1) * r.im[i][j]);
            u.re[i][j] = -alpha * m1.re[i][j];
            u.im[i][j] = -alpha * m1.im[i][j];
        }
    expmap_transp_row<N, MODEL>(x, u, m1, y, g, status);
    x = y;
    return projx<N, MODEL>(x, eps, status);
}

}  // namespace sympa
