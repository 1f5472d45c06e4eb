// Arithmetic of the vector models: euclidean, poincare, lorentz, sphere and the four products of two
// of them, and their RiemannianAdam row (section 20).  Compiles under hipcc (vector_models.hip) and under g++
// (tests/hostsim/hostsim_vector.cpp, tests/hostsim/hostsim_vector_radam.cpp), like the other *_math.hpp headers.  A point is a row of `dims` doubles split into one or two factors; every kernel is
//     per-lane sums over the lane's coordinates  ->  fixed xor butterfly over the G lanes of the pair / row
//     ->  scalar epilogue (the only place where the geometry is looked at)  ->  per-coordinate output.
// The pieces below are those four; the butterfly itself belongs to the caller (shuffles on the device, a loop on the host).
#pragma once
#include <cmath>
#include <cstdint>

#include "siegel_math.hpp"     // SYMPA_HD, d_fma, the status bits

namespace sympa {

constexpr int VEC_MAX_DIMS = 1024;
constexpr int VEC_MAX_FACTORS = 2;
constexpr double VEC_BALL_EPS = 1e-5;      // config.EPS[float64]: projx keeps Poincare points at norm <= 1 - 1e-5

enum VecGeom : int { VG_E = 0, VG_P = 1, VG_L = 2, VG_S = 3 };
// ops.VECTOR_MODEL_IDS, in the order of the reference's ManifoldFactory (sympa/embeddings.py:130-158)
enum VecModel : int { VM_EUCLIDEAN = 0, VM_POINCARE = 1, VM_LORENTZ = 2, VM_SPHERE = 3, VM_PROD_HYSPH = 4, VM_PROD_HYHY = 5,
                      VM_PROD_HYEU = 6, VM_PROD_SPHSPH = 7, VM_COUNT = 8 };
enum VecRowOp : int { VR_PROJX = 0, VR_RSGD = 1, VR_EGRAD2RGRAD = 2 };

// Factor f covers the coordinates [begin[f], begin[f] + count[f]).
struct VecLayout {
    int nf;
    int geom[VEC_MAX_FACTORS];
    int begin[VEC_MAX_FACTORS];
    int count[VEC_MAX_FACTORS];
};

// false: the model id is unknown, a product has odd dims, or an S / L factor has fewer than two coordinates.
SYMPA_HD bool vec_layout(int model, int dims, VecLayout& L) {
    if (dims < 1 || model < 0 || model >= VM_COUNT) return false;
    int g0 = VG_E, g1 = -1;
    switch (model) {
        case VM_EUCLIDEAN: g0 = VG_E; break;
        case VM_POINCARE: g0 = VG_P; break;
        case VM_LORENTZ: g0 = VG_L; break;
        case VM_SPHERE: g0 = VG_S; break;
        case VM_PROD_HYSPH: g0 = VG_P; g1 = VG_S; break;
        case VM_PROD_HYHY: g0 = VG_P; g1 = VG_P; break;
        case VM_PROD_HYEU: g0 = VG_P; g1 = VG_E; break;
        default: g0 = VG_S; g1 = VG_S; break;
    }
    if (g1 < 0) {
        L.nf = 1;
        L.geom[0] = g0; L.begin[0] = 0; L.count[0] = dims;
        L.geom[1] = VG_E; L.begin[1] = dims; L.count[1] = 0;
    } else {
        if (dims % 2 != 0) return false;
        L.nf = 2;
        L.geom[0] = g0; L.begin[0] = 0; L.count[0] = dims / 2;
        L.geom[1] = g1; L.begin[1] = dims / 2; L.count[1] = dims / 2;
    }
    for (int f = 0; f < L.nf; ++f)
        if ((L.geom[f] == VG_S || L.geom[f] == VG_L) && L.count[f] < 2) return false;
    return true;
}

// Lanes per pair / per row: the smallest power of two that leaves a lane at most four coordinates, at most 64 (dims > 256: a
// lane loops).
SYMPA_HD int vec_lanes(int dims) {
    int g = 1;
    while (g < 64 && 4 * g < dims) g *= 2;
    return g;
}

// Coordinate i of the row: its factor, and J_i (-1 for the time-like coordinate of an L factor, else 1).
SYMPA_HD int vec_factor_of(const VecLayout& L, int i) { return (L.nf == 2 && i >= L.begin[1]) ? 1 : 0; }
// (selects, not indexed loads: a layout indexed by a runtime factor would be copied out of the kernel arguments)
SYMPA_HD int vec_geom(const VecLayout& L, int f) { return f ? L.geom[1] : L.geom[0]; }
SYMPA_HD int vec_begin(const VecLayout& L, int f) { return f ? L.begin[1] : L.begin[0]; }
SYMPA_HD double vec_sign(const VecLayout& L, int f, int i) { return (vec_geom(L, f) == VG_L && i == vec_begin(L, f)) ? -1.0 : 1.0; }

// Lane `lane` of G owns the coordinate pairs (2c, 2c + 1), c = lane, lane + G, ...: consecutive lanes read consecutive 16 bytes.
// The assignment does not depend on how the coordinates are loaded, so a pair's sums are the same bits in every entry point.
struct VecPairSums {
    double dd[VEC_MAX_FACTORS], xx[VEC_MAX_FACTORS], yy[VEC_MAX_FACTORS];
};

SYMPA_HD void vec_pair_sums_zero(VecPairSums& s) {
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) { s.dd[f] = 0.0; s.xx[f] = 0.0; s.yy[f] = 0.0; }
}

SYMPA_HD void vec_pair_accumulate(const VecLayout& L, int i, double x, double y, VecPairSums& s) {
    const int f = vec_factor_of(L, i);
    const double t = x - y;
    const double jt = vec_sign(L, f, i) * t;
    // (selects, not indexed stores: the sums stay in registers)
    const double dd = d_fma(jt, t, f ? s.dd[1] : s.dd[0]);
    const double xx = d_fma(x, x, f ? s.xx[1] : s.xx[0]);
    const double yy = d_fma(y, y, f ? s.yy[1] : s.yy[0]);
    if (f) { s.dd[1] = dd; s.xx[1] = xx; s.yy[1] = yy; } else { s.dd[0] = dd; s.xx[0] = xx; s.yy[0] = yy; }
}

SYMPA_HD void vec_pair_lane_sums(const VecLayout& L, int dims, int G, int lane, const double* __restrict__ x,
                                 const double* __restrict__ y, VecPairSums& s) {
    vec_pair_sums_zero(s);
    for (int i = 2 * lane; i < dims; i += 2 * G) {
        vec_pair_accumulate(L, i, x[i], y[i], s);
        if (i + 1 < dims) vec_pair_accumulate(L, i + 1, x[i + 1], y[i + 1], s);
    }
}

// ---- forward epilogue: the distance of one factor from its sums; q is kept for the backward
SYMPA_HD double vec_factor_dist(int geom, double dd, double xx, double yy, double& q, int& st) {
    double d;
    if (geom == VG_E) {
        q = dd;
        d = std::sqrt(dd);
    } else if (geom == VG_P) {
        const double a = 1.0 - xx, b = 1.0 - yy;
        q = dd / (a * b);
        d = 2.0 * std::asinh(std::sqrt(q));
        if (!(a > 0.0) || !(b > 0.0)) { st |= ST_NOT_PD; d = __builtin_nan(""); }      // a point on or outside the unit sphere
    } else if (geom == VG_L) {
        q = 0.25 * (dd > 0.0 ? dd : (dd == dd ? 0.0 : dd));
        d = 2.0 * std::asinh(std::sqrt(q));
    } else {
        const double h = 0.25 * dd;
        q = h < 1.0 ? h : (h == h ? 1.0 : h);
        d = 2.0 * std::asin(std::sqrt(q));
    }
    if (!(d - d == 0.0)) { st |= ST_NONFINITE; d = __builtin_nan(""); }
    return d;
}

SYMPA_HD double vec_combine(int nf, double d0, double d1) { return nf == 1 ? d0 : std::sqrt(d_fma(d0, d0, d1 * d1)); }

SYMPA_HD double vec_pair_dist(const VecLayout& L, const VecPairSums& s, double (&df)[VEC_MAX_FACTORS], double (&q)[VEC_MAX_FACTORS],
                              int& st) {
    df[1] = 0.0; q[1] = 0.0;
    for (int f = 0; f < L.nf; ++f) df[f] = vec_factor_dist(L.geom[f], s.dd[f], s.xx[f], s.yy[f], q[f], st);
    return vec_combine(L.nf, df[0], df[1]);
}

// ---- backward epilogue.  With w = x - y the gradient rows of factor f are
//     d dist / d x_i = alpha J_i w_i + bx x_i          d dist / d y_i = -alpha J_i w_i + by y_i
// (the difference form: for close points alpha w does not cancel, which alpha x - alpha y would).  q == 0 gives a zero
// gradient, as does the clamped side of min / max.
struct VecGradCoef {
    double alpha[VEC_MAX_FACTORS], bx[VEC_MAX_FACTORS], by[VEC_MAX_FACTORS];
};

SYMPA_HD void vec_factor_grad(int geom, double dd, double xx, double yy, double q, double d, double& alpha, double& bx, double& by) {
    alpha = 0.0; bx = 0.0; by = 0.0;
    if (!(q > 0.0)) return;
    if (geom == VG_E) {
        alpha = 1.0 / d;
    } else if (geom == VG_P) {
        // d = 2 asinh sqrt q: d'(q) = 1 / sqrt(q (1 + q));  q = dd / (a b), a = 1 - xx, b = 1 - yy
        const double a = 1.0 - xx, b = 1.0 - yy;
        const double c = 1.0 / std::sqrt(q * (1.0 + q));
        alpha = 2.0 * c / (a * b);
        bx = 2.0 * c * q / a;
        by = 2.0 * c * q / b;
    } else if (geom == VG_L) {
        if (dd > 0.0) alpha = 0.5 / std::sqrt(q * (1.0 + q));       // q = dd / 4
    } else {
        if (q < 1.0) alpha = 0.5 / std::sqrt(q * (1.0 - q));        // d = 2 asin sqrt q, q = dd / 4
    }
}

// coefficients of the whole pair: the factor's own, times d_f / d for a product (d = sqrt(d_0^2 + d_1^2))
SYMPA_HD void vec_pair_grad(const VecLayout& L, const VecPairSums& s, const double (&df)[VEC_MAX_FACTORS],
                            const double (&q)[VEC_MAX_FACTORS], double d, VecGradCoef& c) {
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) { c.alpha[f] = 0.0; c.bx[f] = 0.0; c.by[f] = 0.0; }
    for (int f = 0; f < L.nf; ++f) {
        vec_factor_grad(L.geom[f], s.dd[f], s.xx[f], s.yy[f], q[f], df[f], c.alpha[f], c.bx[f], c.by[f]);
        if (L.nf == 2) {
            const double w = d > 0.0 ? df[f] / d : 0.0;
            c.alpha[f] *= w; c.bx[f] *= w; c.by[f] *= w;
        }
    }
}

SYMPA_HD void vec_pair_grad_coord(const VecLayout& L, const VecGradCoef& c, int i, double x, double y, double scale, double& gx,
                                  double& gy) {
    const int f = vec_factor_of(L, i);
    const double jw = vec_sign(L, f, i) * (x - y);
    const double al = f ? c.alpha[1] : c.alpha[0];
    gx = scale * d_fma(al, jw, (f ? c.bx[1] : c.bx[0]) * x);
    gy = scale * d_fma(-al, jw, (f ? c.by[1] : c.by[0]) * y);
}

// ---- row operations: projx, egrad2rgrad and the RiemannianSGD row (geoopt, momentum 0), per factor:
//     g <- coef grad + wd x,   r = egrad2rgrad(x, g),   x <- retr(x, -lr r)
// in at most three rounds of sums.  Round 1: xx, xg, and `rest` = xx without the factor's first coordinate.  Round 2 (RSGD):
// ww = sum J_i w_i^2 of the stage-1 coordinates w.  Round 3 (RSGD, L): rest of the stage-2 coordinates.
struct VecRowSums {
    double xx[VEC_MAX_FACTORS], xg[VEC_MAX_FACTORS], rest[VEC_MAX_FACTORS];
};

SYMPA_HD void vec_row_sums_zero(VecRowSums& s) {
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) { s.xx[f] = 0.0; s.xg[f] = 0.0; s.rest[f] = 0.0; }
}

SYMPA_HD void vec_row_accumulate(const VecLayout& L, int i, double x, double g, VecRowSums& s) {
    const int f = vec_factor_of(L, i);
    const bool first = i == (f ? L.begin[1] : L.begin[0]);
    const double xx = d_fma(x, x, f ? s.xx[1] : s.xx[0]);
    const double xg = d_fma(x, g, f ? s.xg[1] : s.xg[0]);
    const double rest = first ? (f ? s.rest[1] : s.rest[0]) : d_fma(x, x, f ? s.rest[1] : s.rest[0]);
    if (f) { s.xx[1] = xx; s.xg[1] = xg; s.rest[1] = rest; } else { s.xx[0] = xx; s.xg[0] = xg; s.rest[0] = rest; }
}

// the gradient the step sees: clip coefficient (runner.py:115) and weight decay folded in
SYMPA_HD double vec_row_grad(double grad, double x, double coef, double wd) { return d_fma(wd, x, coef * grad); }

// egrad2rgrad of one coordinate from the round-1 sums
SYMPA_HD double vec_row_rgrad(const VecLayout& L, const VecRowSums& s, int i, double x, double g) {
    const int f = vec_factor_of(L, i);
    const int geom = vec_geom(L, f);
    const double xx = f ? s.xx[1] : s.xx[0], xg = f ? s.xg[1] : s.xg[0];
    if (geom == VG_P) {
        const double a = 1.0 - xx;
        return g * (0.25 * (a * a));
    }
    if (geom == VG_S) return d_fma(-xg, x, g);
    if (geom == VG_L) return d_fma(xg, x, vec_sign(L, f, i) * g);
    return g;
}

// stage 1 of the step: E, P, S: z = x - lr r;  L: u = -lr r
SYMPA_HD double vec_row_stage1(const VecLayout& L, const VecRowSums& s, int i, double x, double g, double lr) {
    const int f = vec_factor_of(L, i);
    const double r = vec_row_rgrad(L, s, i, x, g);
    return vec_geom(L, f) == VG_L ? -lr * r : d_fma(-lr, r, x);
}

// what stage 2 needs of a factor, from ww = sum J_i w_i^2:  P: the rescale (1 when the point stays inside), S: 1 / |z|,
// L: cosh nu and sinh nu / nu.  `moved`: a Poincare factor was projected.
struct VecRowStep {
    double a[VEC_MAX_FACTORS], b[VEC_MAX_FACTORS];
};

SYMPA_HD void vec_row_step_coef(const VecLayout& L, const double (&ww)[VEC_MAX_FACTORS], VecRowStep& c, bool& moved) {
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) { c.a[f] = 1.0; c.b[f] = 0.0; }
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) {
        if (f >= L.nf) continue;
        const int geom = vec_geom(L, f);
        if (geom == VG_P) {
            const double nrm = std::sqrt(ww[f]);
            if (nrm > 1.0 - VEC_BALL_EPS) { c.a[f] = (1.0 - VEC_BALL_EPS) / nrm; moved = true; }
        } else if (geom == VG_S) {
            c.a[f] = 1.0 / std::sqrt(ww[f]);
        } else if (geom == VG_L) {
            const double nu = std::sqrt(ww[f] > 0.0 ? ww[f] : 0.0);
            c.a[f] = std::cosh(nu);
            c.b[f] = nu > 0.0 ? std::sinh(nu) / nu : 1.0;
        }
    }
}

// stage 2: the new coordinate before the L factor's time coordinate is reset.  w = stage 1, x = the old coordinate.
SYMPA_HD double vec_row_stage2(const VecLayout& L, const VecRowStep& c, int i, double x, double w) {
    const int f = vec_factor_of(L, i);
    const double a = f ? c.a[1] : c.a[0], b = f ? c.b[1] : c.b[0];
    return vec_geom(L, f) == VG_L ? d_fma(a, x, b * w) : a * w;
}

// projx of one coordinate from the round-1 sums of the row itself (`moved` as above)
SYMPA_HD void vec_row_projx_coef(const VecLayout& L, const VecRowSums& s, VecRowStep& c, bool& moved) {
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) { c.a[f] = 1.0; c.b[f] = 0.0; }
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) {
        if (f >= L.nf) continue;
        if (vec_geom(L, f) == VG_P) {
            const double nrm = std::sqrt(s.xx[f]);
            if (nrm > 1.0 - VEC_BALL_EPS) { c.a[f] = (1.0 - VEC_BALL_EPS) / nrm; moved = true; }
        } else if (vec_geom(L, f) == VG_S) {
            c.a[f] = 1.0 / std::sqrt(s.xx[f]);
        }
    }
}

// the time-like coordinate of an L factor after a step or a projx: sqrt(1 + rest); every other coordinate is `v`
SYMPA_HD double vec_row_final(const VecLayout& L, const double (&rest)[VEC_MAX_FACTORS], int i, double v) {
    const int f = vec_factor_of(L, i);
    if (vec_geom(L, f) == VG_L && i == vec_begin(L, f)) return std::sqrt(1.0 + (f ? rest[1] : rest[0]));
    return v;
}

// A row is off the manifold or not finite: the status bits of its final round-1 sums (P: xx >= 1)
SYMPA_HD int vec_row_status(const VecLayout& L, const VecRowSums& s) {
    int st = 0;
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) {
        if (f >= L.nf) continue;
        if (!(s.xx[f] - s.xx[f] == 0.0) || !(s.xg[f] - s.xg[f] == 0.0)) st |= ST_NONFINITE;
    }
    return st;
}

// ---- the RiemannianAdam row (geoopt optim/radam.py per factor):
//     g = coef grad + wd x,   r = egrad2rgrad(x, g),   m1 = b1 m + (1 - b1) r,   s1 = b2 s + (1 - b2) I(x, r),
//     u = -lr (m1 / (1 - b1^t)) / (sqrt(s1 / (1 - b2^t)) + eps),   y = retr(x, u),   m' = T(x -> y, m1)
// I is geoopt's component_inner: per coordinate for E, one value per factor for P, S, L (held in every coordinate of the
// factor; the incoming value is read at the factor's first coordinate).  Rounds of sums: round 1 as above (xx, xg);
// round 2: rr = sum J_i r_i^2, xm = <x, m1>, mm = sum J_i m1_i^2 -- the norm of the stage-1 coordinates follows from them and
// xx without a round of its own (u = c m1 with one c per factor); round 3 (only with an L factor): the new time coordinate;
// round 4: the transport's inner products on the row as stored.
struct VecAdamParams {
    double lr, beta1, beta2, eps, wd, coef;
    double bc1, bc2;       // the bias corrections 1 - beta1^t, 1 - beta2^t
};

struct VecAdamCoord {
    double x, r, m1, s;    // s: the incoming exp_avg_sq of the coordinate
};

SYMPA_HD void vec_adam_coord(const VecLayout& L, const VecRowSums& rs, const VecAdamParams& P, int i, double x, double grad, double m,
                             double s, VecAdamCoord& c) {
    c.x = x;
    c.r = vec_row_rgrad(L, rs, i, x, vec_row_grad(grad, x, P.coef, P.wd));
    c.m1 = d_fma(P.beta1, m, (1.0 - P.beta1) * c.r);
    c.s = s;
}

struct VecAdamSums {
    double rr[VEC_MAX_FACTORS], xm[VEC_MAX_FACTORS], mm[VEC_MAX_FACTORS], sin[VEC_MAX_FACTORS];
};

SYMPA_HD void vec_adam_sums_zero(VecAdamSums& S) {
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) { S.rr[f] = 0.0; S.xm[f] = 0.0; S.mm[f] = 0.0; S.sin[f] = 0.0; }
}

// `sin` is the incoming s of the factor's first coordinate: its owner adds it to zeros, so the butterfly hands every lane its bits
SYMPA_HD void vec_adam_accumulate(const VecLayout& L, int i, const VecAdamCoord& c, VecAdamSums& S) {
    const int f = vec_factor_of(L, i);
    const bool first = i == (f ? L.begin[1] : L.begin[0]);
    const double j = vec_sign(L, f, i);
    const double rr = d_fma(j * c.r, c.r, f ? S.rr[1] : S.rr[0]);
    const double xm = d_fma(c.x, c.m1, f ? S.xm[1] : S.xm[0]);
    const double mm = d_fma(j * c.m1, c.m1, f ? S.mm[1] : S.mm[0]);
    const double sin = first ? c.s : (f ? S.sin[1] : S.sin[0]);
    if (f) { S.rr[1] = rr; S.xm[1] = xm; S.mm[1] = mm; S.sin[1] = sin; } else { S.rr[0] = rr; S.xm[0] = xm; S.mm[0] = mm; S.sin[0] = sin; }
}

// u = c m1:  c = -(lr / (1 - b1^t)) / (sqrt(s1 / (1 - b2^t)) + eps)
SYMPA_HD double vec_adam_scale(const VecAdamParams& P, double s1) { return -(P.lr / P.bc1) / (std::sqrt(s1 / P.bc2) + P.eps); }

// what the coordinates need of a P, S or L factor: s1, c, and ww = sum J_i w_i^2 of the stage-1 coordinates w (E, P, S:
// w = x + c m1, ww = xx + 2 c xm + c^2 mm;  L: w = c m1, ww = c^2 mm), which vec_row_step_coef takes.  An E factor keeps
// s1 and c per coordinate.
struct VecAdamStep {
    double s1[VEC_MAX_FACTORS], c[VEC_MAX_FACTORS];
};

SYMPA_HD void vec_adam_step(const VecLayout& L, const VecRowSums& rs, const VecAdamSums& S, const VecAdamParams& P, VecAdamStep& a,
                            double (&ww)[VEC_MAX_FACTORS]) {
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) { a.s1[f] = 0.0; a.c[f] = 0.0; ww[f] = 0.0; }
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) {
        if (f >= L.nf) continue;
        const int geom = vec_geom(L, f);
        if (geom == VG_E) continue;
        double inner = S.rr[f];
        if (geom == VG_P) {
            const double lam = 2.0 / (1.0 - rs.xx[f]);
            inner = lam * lam * S.rr[f];
        } else if (geom == VG_L) {
            inner = S.rr[f] > 0.0 ? S.rr[f] : (S.rr[f] == S.rr[f] ? 0.0 : S.rr[f]);
        }
        a.s1[f] = d_fma(P.beta2, S.sin[f], (1.0 - P.beta2) * inner);
        a.c[f] = vec_adam_scale(P, a.s1[f]);
        const double c = a.c[f];
        ww[f] = geom == VG_L ? (c * c) * S.mm[f] : d_fma(c * c, S.mm[f], d_fma(2.0 * c, S.xm[f], rs.xx[f]));
    }
}

// the new exp_avg_sq of one coordinate
SYMPA_HD double vec_adam_s1(const VecLayout& L, const VecAdamStep& a, const VecAdamParams& P, int i, const VecAdamCoord& c) {
    const int f = vec_factor_of(L, i);
    if (vec_geom(L, f) == VG_E) return d_fma(P.beta2, c.s, (1.0 - P.beta2) * (c.r * c.r));
    return f ? a.s1[1] : a.s1[0];
}

// stage 1 (the RSGD row's, with u in place of -lr r): E, P, S: x + u;  L: u
SYMPA_HD double vec_adam_stage1(const VecLayout& L, const VecAdamStep& a, const VecAdamParams& P, int i, const VecAdamCoord& c) {
    const int f = vec_factor_of(L, i);
    const int geom = vec_geom(L, f);
    const double cc = geom == VG_E ? vec_adam_scale(P, vec_adam_s1(L, a, P, i, c)) : (f ? a.c[1] : a.c[0]);
    return geom == VG_L ? cc * c.m1 : d_fma(cc, c.m1, c.x);
}

// ---- parallel transport T(x -> y, w) of w = m1 along the step, y = the row as stored, in forms that are the identity at
// y = x without a 0 / 0:
//     E: w      S: w - <y, w> y      L: w + <y, w>_L / (2 + dd_L / 2) (x + y),  dd_L = sum J_i (x_i - y_i)^2  (= 1 - <x, y>_L)
//     P: (1 - yy) / (1 - xx) gyr[y, -x] w,   gyr[a, b] w = w + 2 (A a + B b) / D,   A = -<a, w> bb + <b, w> + 2 <a, b> <b, w>,
//        B = -<b, w> aa - <a, w>,   D = 1 + 2 <a, b> + aa bb
// Round-4 sums: ym = sum J_i y_i w_i;  xy = <x, y> (P) or dd_L (L);  yy.
struct VecTranspSums {
    double ym[VEC_MAX_FACTORS], xy[VEC_MAX_FACTORS], yy[VEC_MAX_FACTORS];
};

SYMPA_HD void vec_transp_sums_zero(VecTranspSums& T) {
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) { T.ym[f] = 0.0; T.xy[f] = 0.0; T.yy[f] = 0.0; }
}

SYMPA_HD void vec_transp_accumulate(const VecLayout& L, int i, double x, double y, double w, VecTranspSums& T) {
    const int f = vec_factor_of(L, i);
    const double j = vec_sign(L, f, i);
    const double t = x - y;
    const double ym = d_fma(j * y, w, f ? T.ym[1] : T.ym[0]);
    const double xy = vec_geom(L, f) == VG_L ? d_fma(j * t, t, f ? T.xy[1] : T.xy[0]) : d_fma(x, y, f ? T.xy[1] : T.xy[0]);
    const double yy = d_fma(y, y, f ? T.yy[1] : T.yy[0]);
    if (f) { T.ym[1] = ym; T.xy[1] = xy; T.yy[1] = yy; } else { T.ym[0] = ym; T.xy[0] = xy; T.yy[0] = yy; }
}

// m'_i = t0 (w_i + ta y_i + tb x_i)
struct VecTransp {
    double t0[VEC_MAX_FACTORS], ta[VEC_MAX_FACTORS], tb[VEC_MAX_FACTORS];
};

// xx = <x, x> and xw = <x, w> of the factor (round 1 and round 2)
SYMPA_HD void vec_transp_coef(const VecLayout& L, const double (&xx)[VEC_MAX_FACTORS], const double (&xw)[VEC_MAX_FACTORS],
                              const VecTranspSums& T, VecTransp& c) {
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) { c.t0[f] = 1.0; c.ta[f] = 0.0; c.tb[f] = 0.0; }
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) {
        if (f >= L.nf) continue;
        const int geom = vec_geom(L, f);
        if (geom == VG_S) {
            c.ta[f] = -T.ym[f];
        } else if (geom == VG_L) {
            const double k = T.ym[f] / d_fma(0.5, T.xy[f], 2.0);
            c.ta[f] = k; c.tb[f] = k;
        } else if (geom == VG_P) {
            // a = y, b = -x:  <a, w> = ym, <b, w> = -xw, <a, b> = -xy, aa = yy, bb = xx
            const double ym = T.ym[f], xy = T.xy[f], yy = T.yy[f];
            const double A = d_fma(2.0 * xy, xw[f], d_fma(-ym, xx[f], -xw[f]));
            const double B = d_fma(xw[f], yy, -ym);
            const double D = d_fma(yy, xx[f], d_fma(-2.0, xy, 1.0));
            c.t0[f] = (1.0 - yy) / (1.0 - xx[f]);
            c.ta[f] = 2.0 * A / D;
            c.tb[f] = -2.0 * B / D;
        }
    }
}

SYMPA_HD double vec_transp_coord(const VecLayout& L, const VecTransp& c, int i, double x, double y, double w) {
    const int f = vec_factor_of(L, i);
    if (vec_geom(L, f) == VG_E) return w;
    return (f ? c.t0[1] : c.t0[0]) * d_fma(f ? c.ta[1] : c.ta[0], y, d_fma(f ? c.tb[1] : c.tb[0], x, w));
}

// non-finite sums of the Adam row (round 1 is vec_row_status)
SYMPA_HD int vec_adam_status(const VecLayout& L, const VecAdamSums& S, const double (&ww)[VEC_MAX_FACTORS], const VecTranspSums& T) {
    int st = 0;
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) {
        if (f >= L.nf) continue;
        const double all = S.rr[f] + S.xm[f] + S.mm[f] + S.sin[f] + ww[f] + T.ym[f] + T.xy[f] + T.yy[f];
        if (!(all - all == 0.0)) st |= ST_NONFINITE;
    }
    return st;
}

}  // namespace sympa
