// g++ build of the vector models' arithmetic (sympa_amd/csrc/vector_math.hpp) for the CPU tests: the per-lane sums, the xor
// butterfly over the G lanes of a pair / row emulated with a loop, the scalar epilogues and the per-coordinate outputs, in the
// order the kernels of sympa_amd/csrc/vector_models.hip run them.  G = 0 takes the kernels' own choice (vec_lanes).
#include <cstdint>
#include <vector>

#include "../../sympa_amd/csrc/vector_math.hpp"

namespace {
using namespace sympa;

// v[l] <- v[l] + v[l ^ off], off = G / 2, ..., 1: what `v += __shfl_xor(v, off)` leaves in lane l
void butterfly(std::vector<double>& v) {
    const int G = (int)v.size();
    std::vector<double> w(G);
    for (int off = G / 2; off > 0; off >>= 1) {
        for (int l = 0; l < G; ++l) w[l] = v[l] + v[l ^ off];
        v = w;
    }
}

bool valid_lanes(int G) { return G == 1 || G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64; }

// sums of one pair as lane 0 holds them after the butterfly
void pair_sums(const VecLayout& L, int dims, int G, const double* x, const double* y, VecPairSums& s) {
    std::vector<VecPairSums> lanes(G);
    for (int l = 0; l < G; ++l) vec_pair_lane_sums(L, dims, G, l, x, y, lanes[l]);
    for (int f = 0; f < VEC_MAX_FACTORS; ++f) {
        std::vector<double> a(G), b(G), c(G);
        for (int l = 0; l < G; ++l) { a[l] = lanes[l].dd[f]; b[l] = lanes[l].xx[f]; c[l] = lanes[l].yy[f]; }
        butterfly(a); butterfly(b); butterfly(c);
        s.dd[f] = a[0]; s.xx[f] = b[0]; s.yy[f] = c[0];
    }
}

template <typename F>
double lane_reduce(int dims, int G, F term) {      // term(i, acc) -> acc, over the coordinates of each lane, then the butterfly
    std::vector<double> v(G, 0.0);
    for (int l = 0; l < G; ++l)
        for (int i = 2 * l; i < dims; i += 2 * G)
            for (int k = 0; k < 2 && i + k < dims; ++k) v[l] = term(i + k, v[l]);
    butterfly(v);
    return v[0];
}
}  // namespace

extern "C" {

int sympa_hostsim_vector_lanes(int dims) { return vec_lanes(dims); }

int sympa_hostsim_vector_layout(int model, int dims) {
    VecLayout L;
    return vec_layout(model, dims, L) ? L.nf : 0;
}

int sympa_hostsim_vector_fwd(const double* x, const double* y, int64_t b, int dims, int model, int G, double* out, double* sums,
                             int32_t* status) {
    VecLayout L;
    if (!vec_layout(model, dims, L)) return -1;
    if (G == 0) G = vec_lanes(dims);
    if (!valid_lanes(G)) return -1;
    int st_all = 0;
    for (int64_t p = 0; p < b; ++p) {
        VecPairSums s;
        pair_sums(L, dims, G, x + p * dims, y + p * dims, s);
        double df[VEC_MAX_FACTORS], q[VEC_MAX_FACTORS];
        int st = 0;
        out[p] = vec_pair_dist(L, s, df, q, st);
        st_all |= st;
        if (sums != nullptr)
            for (int f = 0; f < VEC_MAX_FACTORS; ++f) {
                sums[(p * 2 + f) * 3 + 0] = s.dd[f]; sums[(p * 2 + f) * 3 + 1] = s.xx[f]; sums[(p * 2 + f) * 3 + 2] = s.yy[f];
            }
    }
    if (status != nullptr) *status = st_all;
    return 0;
}

int sympa_hostsim_vector_bwd(const double* x, const double* y, const double* go, int64_t b, int dims, int model, int G, double* out,
                             double* gx, double* gy) {
    VecLayout L;
    if (!vec_layout(model, dims, L)) return -1;
    if (G == 0) G = vec_lanes(dims);
    if (!valid_lanes(G)) return -1;
    for (int64_t p = 0; p < b; ++p) {
        const double* xp = x + p * dims;
        const double* yp = y + p * dims;
        VecPairSums s;
        pair_sums(L, dims, G, xp, yp, s);
        double df[VEC_MAX_FACTORS], q[VEC_MAX_FACTORS];
        int st = 0;
        const double d = vec_pair_dist(L, s, df, q, st);
        VecGradCoef c;
        vec_pair_grad(L, s, df, q, d, c);
        out[p] = d;
        for (int i = 0; i < dims; ++i) vec_pair_grad_coord(L, c, i, xp[i], yp[i], go[p], gx[p * dims + i], gy[p * dims + i]);
    }
    return 0;
}

// op: 0 projx, 1 the RSGD row (out <- step of x), 2 egrad2rgrad.  moved: rows whose Poincare factor was projected.
int sympa_hostsim_vector_rows(int op, const double* x, const double* g, double* out, int64_t b, int dims, int model, int G, double lr,
                              double wd, double coef, int32_t* moved_rows) {
    VecLayout L;
    if (!vec_layout(model, dims, L)) return -1;
    if (G == 0) G = vec_lanes(dims);
    if (!valid_lanes(G)) return -1;
    int moved_count = 0;
    for (int64_t p = 0; p < b; ++p) {
        const double* xp = x + p * dims;
        const double* gp = op == VR_PROJX ? xp : g + p * dims;
        const double w_d = op == VR_RSGD ? wd : 0.0, cf = op == VR_RSGD ? coef : 1.0;
        auto grad = [&](int i) { return vec_row_grad(gp[i], xp[i], cf, w_d); };
        // round 1 (three values per factor, each through its own butterfly)
        VecRowSums s;
        vec_row_sums_zero(s);
        for (int f = 0; f < VEC_MAX_FACTORS; ++f)
            for (int which = 0; which < 3; ++which) {
                const double v = lane_reduce(dims, G, [&](int i, double acc) {
                    if (vec_factor_of(L, i) != f) return acc;
                    VecRowSums t;
                    vec_row_sums_zero(t);
                    (which == 0 ? t.xx[f] : which == 1 ? t.xg[f] : t.rest[f]) = acc;
                    vec_row_accumulate(L, i, xp[i], grad(i), t);
                    return which == 0 ? t.xx[f] : which == 1 ? t.xg[f] : t.rest[f];
                });
                (which == 0 ? s.xx[f] : which == 1 ? s.xg[f] : s.rest[f]) = v;
            }
        bool moved = false;
        VecRowStep c;
        if (op == VR_PROJX) {
            vec_row_projx_coef(L, s, c, moved);
            for (int i = 0; i < dims; ++i) out[p * dims + i] = vec_row_final(L, s.rest, i, c.a[vec_factor_of(L, i)] * xp[i]);
        } else if (op == VR_EGRAD2RGRAD) {
            for (int i = 0; i < dims; ++i) out[p * dims + i] = vec_row_rgrad(L, s, i, xp[i], gp[i]);
        } else {
            double ww[VEC_MAX_FACTORS], rest[VEC_MAX_FACTORS];
            for (int f = 0; f < VEC_MAX_FACTORS; ++f)
                ww[f] = lane_reduce(dims, G, [&](int i, double acc) {
                    if (vec_factor_of(L, i) != f) return acc;
                    const double w = vec_row_stage1(L, s, i, xp[i], grad(i), lr);
                    return d_fma(vec_sign(L, f, i) * w, w, acc);
                });
            vec_row_step_coef(L, ww, c, moved);
            for (int f = 0; f < VEC_MAX_FACTORS; ++f)
                rest[f] = lane_reduce(dims, G, [&](int i, double acc) {
                    if (vec_factor_of(L, i) != f || i == L.begin[f]) return acc;
                    const double z = vec_row_stage2(L, c, i, xp[i], vec_row_stage1(L, s, i, xp[i], grad(i), lr));
                    return d_fma(z, z, acc);
                });
            for (int i = 0; i < dims; ++i)
                out[p * dims + i] = vec_row_final(L, rest, i, vec_row_stage2(L, c, i, xp[i], vec_row_stage1(L, s, i, xp[i], grad(i), lr)));
        }
        moved_count += moved ? 1 : 0;
    }
    if (moved_rows != nullptr) *moved_rows = moved_count;
    return 0;
}

}  // extern "C"
