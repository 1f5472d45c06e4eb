// gfx950 kernels + C-ABI of the vector models (vector_math.hpp): euclidean, poincare, lorentz, sphere and
// the four products.  G lanes per pair (forward, backward) or per row (projx, egrad2rgrad, RSGD step, RiemannianAdam step:
// DESIGN.md section 20), G in {1, 2, ..., 64}
// chosen from dims (vec_lanes): lane l owns the coordinate pairs (2c, 2c + 1), c = l, l + G, ..., so consecutive lanes read
// consecutive 16 bytes.  The per-factor sums go through a fixed xor butterfly over the G lanes, after which every lane of the
// pair holds the same bits and runs the scalar epilogue -- the only code that looks at the geometry (a runtime switch: the
// instantiations are 7 values of G times four kernels).
//
// Every cross-lane read (the butterflies, the ballots) is executed by all 64 lanes of the wave:
// lanes of pairs / rows past the end clamp their index to the last one, run the same arithmetic and have only their stores,
// their status bits and their contributions to loss / grad_scale / the projected counter predicated off.
#include "siegel_common.hpp"
#include "vector_math.hpp"

namespace {
using namespace sympa_hip;
using sympa::VecLayout;

constexpr int VEC_BLOCK = 256;

struct VecPairArgs {
    const double* x;        // first points [b, dims] or the table
    const double* y;        // second points or the table
    const int64_t* src;     // nullptr: pair i reads rows (i, i)
    const int64_t* dst;
    int64_t src_stride, dst_stride;
    int64_t num_rows;       // rows addressable through src / dst
    int64_t b;
    int64_t ap_cols;        // > 0: all-pairs mode, pair p = (ap_row0 + p / ap_cols, p % ap_cols), src / dst unused
    int64_t ap_row0;
    const double* scale;    // device scalar or nullptr
    double inv_scale_coef;
    double* out;            // [b] (backward: optional)
    int32_t* status;
    int dims;
    int vec_load;           // rows of x and y start on 16 bytes: one 16-byte load per coordinate pair
    // backward only
    const double* go;
    const double* graph_dist;
    double loss_scale;
    double* loss;
    double* gx;
    double* gy;
    double* gscale;
    int vec_store;          // rows of gx and gy start on 16 bytes
};

__device__ __forceinline__ void ld2(const double* __restrict__ p, const int i, const int dims, const bool vec, double& a, double& b) {
    if (vec) {
        const double2 v = *reinterpret_cast<const double2*>(p + i);
        a = v.x; b = v.y;
    } else {
        a = p[i];
        b = (i + 1 < dims) ? p[i + 1] : 0.0;
    }
}

__device__ __forceinline__ void st2(double* __restrict__ p, const int i, const int dims, const bool vec, const double a, const double b) {
    if (vec) {
        *reinterpret_cast<double2*>(p + i) = make_double2(a, b);
    } else {
        p[i] = a;
        if (i + 1 < dims) p[i + 1] = b;
    }
}

template <int G>
__device__ __forceinline__ double butterfly(double v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// rows of pair pp (already clamped into [0, b)); a bad index reads row 0 and is flagged
__device__ __forceinline__ void pair_rows(const VecPairArgs& a, const int64_t pp, int64_t& r1, int64_t& r2, int& st) {
    if (a.ap_cols > 0) {
        r1 = a.ap_row0 + pp / a.ap_cols;
        r2 = pp % a.ap_cols;
    } else if (a.src != nullptr) {
        r1 = a.src[pp * a.src_stride];
        r2 = a.dst[pp * a.dst_stride];
        if (r1 < 0 || r1 >= a.num_rows || r2 < 0 || r2 >= a.num_rows) { st |= sympa::ST_BAD_INDEX; r1 = 0; r2 = 0; }
    } else {
        r1 = pp; r2 = pp;
    }
}

template <int G>
__device__ __forceinline__ void pair_sums(const VecPairArgs& a, const VecLayout& L, const int lane, const double* __restrict__ x,
                                          const double* __restrict__ y, sympa::VecPairSums& s) {
    sympa::vec_pair_sums_zero(s);
    const bool vec = a.vec_load != 0;
    for (int i = 2 * lane; i < a.dims; i += 2 * G) {
        double x0, x1, y0, y1;
        ld2(x, i, a.dims, vec, x0, x1);
        ld2(y, i, a.dims, vec, y0, y1);
        sympa::vec_pair_accumulate(L, i, x0, y0, s);
        if (i + 1 < a.dims) sympa::vec_pair_accumulate(L, i + 1, x1, y1, s);
    }
    s.dd[0] = butterfly<G>(s.dd[0]); s.xx[0] = butterfly<G>(s.xx[0]); s.yy[0] = butterfly<G>(s.yy[0]);
    s.dd[1] = butterfly<G>(s.dd[1]); s.xx[1] = butterfly<G>(s.xx[1]); s.yy[1] = butterfly<G>(s.yy[1]);
}

__device__ __forceinline__ void report_status(int32_t* status, const bool flagged, const int st) {
    if (status != nullptr) {
        const unsigned long long m = __ballot(flagged ? 1 : 0);
        if (m != 0ull) {
            if (flagged) atomicOr(&status[0], st);
            if ((threadIdx.x & 63) == 0) atomicAdd(&status[1], (int)__popcll(m));
        }
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int G>
__global__ __launch_bounds__(VEC_BLOCK) void vec_fwd_kernel(const VecPairArgs a, const VecLayout L) {
    const int64_t t = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x;
    const int64_t p = t / G;
    const int lane = (int)(threadIdx.x % G);
    const bool live = p < a.b;
    const int64_t pp = live ? p : a.b - 1;
    int st = 0;
    int64_t r1, r2;
    pair_rows(a, pp, r1, r2, st);
    sympa::VecPairSums s;
    pair_sums<G>(a, L, lane, a.x + r1 * a.dims, a.y + r2 * a.dims, s);
    double df[sympa::VEC_MAX_FACTORS], q[sympa::VEC_MAX_FACTORS];
    double d = sympa::vec_pair_dist(L, s, df, q, st);
    if (a.scale != nullptr) d *= fmax(a.scale[0] * a.inv_scale_coef, 0.1);
    if (st & sympa::ST_BAD_INDEX) d = __builtin_nan("");
    const bool writer = live && lane == 0;
    if (writer) a.out[p] = d;
    report_status(a.status, writer && st != 0, st);
}

template <int G>
__global__ __launch_bounds__(VEC_BLOCK) void vec_bwd_kernel(const VecPairArgs a, const VecLayout L) {
    const int64_t t = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x;
    const int64_t p = t / G;
    const int lane = (int)(threadIdx.x % G);
    const bool live = p < a.b;
    const int64_t pp = live ? p : a.b - 1;
    int st = 0;
    int64_t r1, r2;
    pair_rows(a, pp, r1, r2, st);
    const double* __restrict__ x = a.x + r1 * a.dims;
    const double* __restrict__ y = a.y + r2 * a.dims;
    sympa::VecPairSums s;
    pair_sums<G>(a, L, lane, x, y, s);
    double df[sympa::VEC_MAX_FACTORS], q[sympa::VEC_MAX_FACTORS];
    const double dist = sympa::vec_pair_dist(L, s, df, q, st);
    sympa::VecGradCoef c;
    sympa::vec_pair_grad(L, s, df, q, dist, c);
    double sc = 1.0;
    bool sc_active = false;
    if (a.scale != nullptr) {
        const double raw = a.scale[0] * a.inv_scale_coef;
        sc_active = raw > 0.1;
        sc = sc_active ? raw : 0.1;
    }
    const bool bad = (st & sympa::ST_BAD_INDEX) != 0;
    double go = 0.0, loss_i = 0.0;
    if (a.graph_dist != nullptr) {            // AverageDistortionLoss (losses.py:10-19): sum |(d/g)^2 - 1|
        const double gd = a.graph_dist[pp];
        const double ratio = dist * sc / gd;
        const double e = ratio * ratio - 1.0;
        loss_i = fabs(e) * a.loss_scale;
        go = (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0)) * 2.0 * ratio / gd * a.loss_scale;
    } else {
        go = a.go[pp];
    }
    if (bad) { go = 0.0; loss_i = 0.0; }
    const double f = go * sc;
    double* __restrict__ gx = a.gx + pp * a.dims;      // lanes past the end recompute the last pair and do not store
    double* __restrict__ gy = a.gy + pp * a.dims;
    const bool vl = a.vec_load != 0, vs = a.vec_store != 0;
    for (int i = 2 * lane; i < a.dims; i += 2 * G) {
        double x0, x1, y0, y1, gx0, gx1 = 0.0, gy0, gy1 = 0.0;
        ld2(x, i, a.dims, vl, x0, x1);
        ld2(y, i, a.dims, vl, y0, y1);
        sympa::vec_pair_grad_coord(L, c, i, x0, y0, f, gx0, gy0);
        if (i + 1 < a.dims) sympa::vec_pair_grad_coord(L, c, i + 1, x1, y1, f, gx1, gy1);
        if (live) {
            st2(gx, i, a.dims, vs, gx0, gx1);
            st2(gy, i, a.dims, vs, gy0, gy1);
        }
    }
    const bool writer = live && lane == 0;
    if (writer && a.out != nullptr) a.out[p] = bad ? __builtin_nan("") : dist * sc;
    if (a.gscale != nullptr && a.scale != nullptr) {
        const double v = wave_sum((writer && sc_active) ? go * dist * a.inv_scale_coef : 0.0);
        if ((threadIdx.x & 63) == 0 && v != 0.0) atomicAdd(a.gscale, v);
    }
    if (a.loss != nullptr && a.graph_dist != nullptr) {
        const double v = wave_sum(writer ? loss_i : 0.0);
        if ((threadIdx.x & 63) == 0 && v != 0.0) atomicAdd(a.loss, v);
    }
    report_status(a.status, writer && st != 0, st);
}

struct VecRowArgs {
    double* x;              // VR_RSGD: the table, updated in place; otherwise read only
    const double* g;        // gradient rows (VR_PROJX: unused)
    double* out;            // VR_PROJX / VR_EGRAD2RGRAD
    int64_t b;
    double lr, wd;
    const double* clip;     // device: squared total gradient norm, or nullptr
    double max_norm;
    int32_t* projected;
    int32_t* status;
    int dims;
    int op;
    int vec_x, vec_g, vec_out;
};

template <int G>
__global__ __launch_bounds__(VEC_BLOCK) void vec_row_kernel(const VecRowArgs a, const VecLayout L) {
    const int64_t t = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x;
    const int64_t p = t / G;
    const int lane = (int)(threadIdx.x % G);
    const bool live = p < a.b;
    const int64_t pp = live ? p : a.b - 1;
    const int dims = a.dims;
    // (no __restrict__ here: the RSGD step writes the row it reads; a lane reads and writes its own coordinates only, and
    // writes them after its last read)
    const double* x = a.x + pp * dims;
    const double* g = a.op == sympa::VR_PROJX ? x : a.g + pp * dims;
    const bool vx = a.vec_x != 0, vg = a.op == sympa::VR_PROJX ? vx : a.vec_g != 0;
    const double coef = (a.op == sympa::VR_RSGD && a.clip != nullptr) ? fmin(1.0, a.max_norm / (sqrt(a.clip[0]) + 1e-6)) : 1.0;
    const double wd = a.op == sympa::VR_RSGD ? a.wd : 0.0;

    // round 1: xx, <x, g>, rest of the row itself
    sympa::VecRowSums s;
    sympa::vec_row_sums_zero(s);
    for (int i = 2 * lane; i < dims; i += 2 * G) {
        double x0, x1, g0, g1;
        ld2(x, i, dims, vx, x0, x1);
        ld2(g, i, dims, vg, g0, g1);
        sympa::vec_row_accumulate(L, i, x0, sympa::vec_row_grad(g0, x0, coef, wd), s);
        if (i + 1 < dims) sympa::vec_row_accumulate(L, i + 1, x1, sympa::vec_row_grad(g1, x1, coef, wd), s);
    }
    for (int f = 0; f < sympa::VEC_MAX_FACTORS; ++f) {
        s.xx[f] = butterfly<G>(s.xx[f]); s.xg[f] = butterfly<G>(s.xg[f]); s.rest[f] = butterfly<G>(s.rest[f]);
    }
    int st = sympa::vec_row_status(L, s);
    bool moved = false;

    if (a.op != sympa::VR_RSGD) {
        sympa::VecRowStep c;
        sympa::vec_row_projx_coef(L, s, c, moved);
        // projx rescales P and S factors, so the L factor's rest is the row's own (its scale is 1)
        double* __restrict__ out = a.out + pp * dims;
        for (int i = 2 * lane; i < dims; i += 2 * G) {
            double x0, x1, g0, g1, o0, o1 = 0.0;
            ld2(x, i, dims, vx, x0, x1);
            ld2(g, i, dims, vg, g0, g1);
            if (a.op == sympa::VR_PROJX) {
                o0 = sympa::vec_row_final(L, s.rest, i, (sympa::vec_factor_of(L, i) ? c.a[1] : c.a[0]) * x0);
                if (i + 1 < dims) o1 = sympa::vec_row_final(L, s.rest, i + 1, (sympa::vec_factor_of(L, i + 1) ? c.a[1] : c.a[0]) * x1);
            } else {
                o0 = sympa::vec_row_rgrad(L, s, i, x0, g0);
                if (i + 1 < dims) o1 = sympa::vec_row_rgrad(L, s, i + 1, x1, g1);
            }
            if (live) st2(out, i, dims, a.vec_out != 0, o0, o1);
        }
        if (a.op != sympa::VR_PROJX) moved = false;
    } else {
        // round 2: ww = sum J_i w_i^2 of the stage-1 coordinates
        double ww[sympa::VEC_MAX_FACTORS] = {0.0, 0.0};
        for (int i = 2 * lane; i < dims; i += 2 * G) {
            double x0, x1, g0, g1;
            ld2(x, i, dims, vx, x0, x1);
            ld2(g, i, dims, vg, g0, g1);
            for (int k = 0; k < 2 && i + k < dims; ++k) {
                const double xv = k ? x1 : x0;
                const double w = sympa::vec_row_stage1(L, s, i + k, xv, sympa::vec_row_grad(k ? g1 : g0, xv, coef, wd), a.lr);
                const int f = sympa::vec_factor_of(L, i + k);
                const double acc = sympa::d_fma(sympa::vec_sign(L, f, i + k) * w, w, f ? ww[1] : ww[0]);
                if (f) ww[1] = acc; else ww[0] = acc;
            }
        }
        ww[0] = butterfly<G>(ww[0]); ww[1] = butterfly<G>(ww[1]);
        sympa::VecRowStep c;
        sympa::vec_row_step_coef(L, ww, c, moved);
        // round 3: rest of the stage-2 coordinates (the L factor's new time coordinate)
        double rest[sympa::VEC_MAX_FACTORS] = {0.0, 0.0};
        for (int i = 2 * lane; i < dims; i += 2 * G) {
            double x0, x1, g0, g1;
            ld2(x, i, dims, vx, x0, x1);
            ld2(g, i, dims, vg, g0, g1);
            for (int k = 0; k < 2 && i + k < dims; ++k) {
                const double xv = k ? x1 : x0;
                const double w = sympa::vec_row_stage1(L, s, i + k, xv, sympa::vec_row_grad(k ? g1 : g0, xv, coef, wd), a.lr);
                const double z = sympa::vec_row_stage2(L, c, i + k, xv, w);
                const int f = sympa::vec_factor_of(L, i + k);
                if (i + k != (f ? L.begin[1] : L.begin[0])) {
                    const double acc = sympa::d_fma(z, z, f ? rest[1] : rest[0]);
                    if (f) rest[1] = acc; else rest[0] = acc;
                }
            }
        }
        rest[0] = butterfly<G>(rest[0]); rest[1] = butterfly<G>(rest[1]);
        double* xo = a.x + pp * dims;
        for (int i = 2 * lane; i < dims; i += 2 * G) {
            double x0, x1, g0, g1, o[2] = {0.0, 0.0};
            ld2(x, i, dims, vx, x0, x1);
            ld2(g, i, dims, vg, g0, g1);
            for (int k = 0; k < 2 && i + k < dims; ++k) {
                const double xv = k ? x1 : x0;
                const double w = sympa::vec_row_stage1(L, s, i + k, xv, sympa::vec_row_grad(k ? g1 : g0, xv, coef, wd), a.lr);
                o[k] = sympa::vec_row_final(L, rest, i + k, sympa::vec_row_stage2(L, c, i + k, xv, w));
            }
            if (live) st2(xo, i, dims, vx, o[0], o[1]);
        }
        if (!(ww[0] - ww[0] == 0.0) || !(ww[1] - ww[1] == 0.0)) st |= sympa::ST_NONFINITE;
    }
    const bool writer = live && lane == 0;
    const unsigned long long m = __ballot((writer && moved) ? 1 : 0);
    if (a.projected != nullptr && m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(a.projected, (int)__popcll(m));
    report_status(a.status, writer && st != 0, st);
}

struct VecAdamArgs {
    double* x;              // the table, exp_avg and exp_avg_sq: updated in place
    const double* g;
    double* m;
    double* s;
    int64_t b;
    double lr, beta1, beta2, eps, wd;
    const double* pows;     // device: (beta1^t, beta2^t) of this step
    const double* clip;     // device: squared total gradient norm, or nullptr
    double max_norm;
    int32_t* projected;
    int32_t* status;
    int dims;
    int has_l;              // the layout has an L factor: the round for its new time coordinate is taken
    int vec_x, vec_g, vec_m, vec_s;
};

// The RiemannianAdam row (vector_math.hpp): the lane ownership of vec_row_kernel, four rounds of sums
// (three without an L factor), then one pass that stores the row, exp_avg and exp_avg_sq.  A lane reads and writes its own
// coordinates only (the factor's incoming exp_avg_sq travels through a butterfly, not through memory), re-reads them from L1
// in every round, and stores a coordinate pair after its last read of it.
template <int G>
__global__ __launch_bounds__(VEC_BLOCK) void vec_radam_kernel(const VecAdamArgs a, const VecLayout L) {
    const int64_t t = (int64_t)blockIdx.x * VEC_BLOCK + threadIdx.x;
    const int64_t p = t / G;
    const int lane = (int)(threadIdx.x % G);
    const bool live = p < a.b;
    const int64_t pp = live ? p : a.b - 1;
    const int dims = a.dims;
    // (no __restrict__: the three tensors are read and written)
    double* x = a.x + pp * dims;
    const double* g = a.g + pp * dims;
    double* m = a.m + pp * dims;
    double* s = a.s + pp * dims;
    const bool vx = a.vec_x != 0, vg = a.vec_g != 0, vm = a.vec_m != 0, vs = a.vec_s != 0;
    sympa::VecAdamParams P;
    P.lr = a.lr; P.beta1 = a.beta1; P.beta2 = a.beta2; P.eps = a.eps; P.wd = a.wd;
    P.coef = a.clip != nullptr ? fmin(1.0, a.max_norm / (sqrt(a.clip[0]) + 1e-6)) : 1.0;
    P.bc1 = 1.0 - a.pows[0];
    P.bc2 = 1.0 - a.pows[1];

    // round 1: xx, <x, g> (and the row's own rest, unused here)
    sympa::VecRowSums rs;
    sympa::vec_row_sums_zero(rs);
    for (int i = 2 * lane; i < dims; i += 2 * G) {
        double x0, x1, g0, g1;
        ld2(x, i, dims, vx, x0, x1);
        ld2(g, i, dims, vg, g0, g1);
        sympa::vec_row_accumulate(L, i, x0, sympa::vec_row_grad(g0, x0, P.coef, P.wd), rs);
        if (i + 1 < dims) sympa::vec_row_accumulate(L, i + 1, x1, sympa::vec_row_grad(g1, x1, P.coef, P.wd), rs);
    }
    for (int f = 0; f < sympa::VEC_MAX_FACTORS; ++f) { rs.xx[f] = butterfly<G>(rs.xx[f]); rs.xg[f] = butterfly<G>(rs.xg[f]); }
    int st = sympa::vec_row_status(L, rs);

    // the lane's coordinates (i, i + 1) with everything round 1 decides: r and m1
    auto load = [&](const int i, sympa::VecAdamCoord (&c)[2]) {
        double x0, x1, g0, g1, m0, m1, s0, s1;
        ld2(x, i, dims, vx, x0, x1);
        ld2(g, i, dims, vg, g0, g1);
        ld2(m, i, dims, vm, m0, m1);
        ld2(s, i, dims, vs, s0, s1);
        sympa::vec_adam_coord(L, rs, P, i, x0, g0, m0, s0, c[0]);
        sympa::vec_adam_coord(L, rs, P, (i + 1 < dims) ? i + 1 : i, x1, g1, m1, s1, c[1]);
    };

    // round 2: rr, <x, m1>, mm, the factor's incoming exp_avg_sq
    sympa::VecAdamSums S;
    sympa::vec_adam_sums_zero(S);
    for (int i = 2 * lane; i < dims; i += 2 * G) {
        sympa::VecAdamCoord c[2];
        load(i, c);
        sympa::vec_adam_accumulate(L, i, c[0], S);
        if (i + 1 < dims) sympa::vec_adam_accumulate(L, i + 1, c[1], S);
    }
    for (int f = 0; f < sympa::VEC_MAX_FACTORS; ++f) {
        S.rr[f] = butterfly<G>(S.rr[f]); S.xm[f] = butterfly<G>(S.xm[f]); S.mm[f] = butterfly<G>(S.mm[f]);
        S.sin[f] = butterfly<G>(S.sin[f]);
    }
    sympa::VecAdamStep as;
    double ww[sympa::VEC_MAX_FACTORS];
    sympa::vec_adam_step(L, rs, S, P, as, ww);
    bool moved = false;
    sympa::VecRowStep sc;
    sympa::vec_row_step_coef(L, ww, sc, moved);

    // round 3 (wave-uniform: the layout is a kernel argument): the L factor's new time coordinate
    double rest[sympa::VEC_MAX_FACTORS] = {0.0, 0.0};
    if (a.has_l) {
        for (int i = 2 * lane; i < dims; i += 2 * G) {
            sympa::VecAdamCoord c[2];
            load(i, c);
            for (int k = 0; k < 2 && i + k < dims; ++k) {
                const int f = sympa::vec_factor_of(L, i + k);
                if (i + k != (f ? L.begin[1] : L.begin[0])) {
                    const double z = sympa::vec_row_stage2(L, sc, i + k, c[k].x, sympa::vec_adam_stage1(L, as, P, i + k, c[k]));
                    const double acc = sympa::d_fma(z, z, f ? rest[1] : rest[0]);
                    if (f) rest[1] = acc; else rest[0] = acc;
                }
            }
        }
        rest[0] = butterfly<G>(rest[0]); rest[1] = butterfly<G>(rest[1]);
    }

    // round 4: the transport's inner products on the row as it will be stored
    sympa::VecTranspSums T;
    sympa::vec_transp_sums_zero(T);
    for (int i = 2 * lane; i < dims; i += 2 * G) {
        sympa::VecAdamCoord c[2];
        load(i, c);
        for (int k = 0; k < 2 && i + k < dims; ++k) {
            const double z = sympa::vec_row_stage2(L, sc, i + k, c[k].x, sympa::vec_adam_stage1(L, as, P, i + k, c[k]));
            sympa::vec_transp_accumulate(L, i + k, c[k].x, sympa::vec_row_final(L, rest, i + k, z), c[k].m1, T);
        }
    }
    for (int f = 0; f < sympa::VEC_MAX_FACTORS; ++f) {
        T.ym[f] = butterfly<G>(T.ym[f]); T.xy[f] = butterfly<G>(T.xy[f]); T.yy[f] = butterfly<G>(T.yy[f]);
    }
    sympa::VecTransp tc;
    sympa::vec_transp_coef(L, rs.xx, S.xm, T, tc);
    st |= sympa::vec_adam_status(L, S, ww, T);

    for (int i = 2 * lane; i < dims; i += 2 * G) {
        sympa::VecAdamCoord c[2];
        load(i, c);
        double y[2] = {0.0, 0.0}, mo[2] = {0.0, 0.0}, so[2] = {0.0, 0.0};
        for (int k = 0; k < 2 && i + k < dims; ++k) {
            const double z = sympa::vec_row_stage2(L, sc, i + k, c[k].x, sympa::vec_adam_stage1(L, as, P, i + k, c[k]));
            y[k] = sympa::vec_row_final(L, rest, i + k, z);
            mo[k] = sympa::vec_transp_coord(L, tc, i + k, c[k].x, y[k], c[k].m1);
            so[k] = sympa::vec_adam_s1(L, as, P, i + k, c[k]);
        }
        if (live) {
            st2(x, i, dims, vx, y[0], y[1]);
            st2(m, i, dims, vm, mo[0], mo[1]);
            st2(s, i, dims, vs, so[0], so[1]);
        }
    }
    const bool writer = live && lane == 0;
    const unsigned long long mask = __ballot((writer && moved) ? 1 : 0);
    if (a.projected != nullptr && mask != 0ull && (threadIdx.x & 63) == 0) atomicAdd(a.projected, (int)__popcll(mask));
    report_status(a.status, writer && st != 0, st);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int check_dims(int dims, int model, VecLayout& L) {
    if (dims < 1) return fail(SYMPA_ERR_BAD_ARG, "vector models: dims must be positive");
    if (dims > sympa::VEC_MAX_DIMS) return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "vector models: dims outside [1, 1024]");
    if (!sympa::vec_layout(model, dims, L))
        return fail(SYMPA_ERR_BAD_ARG, "vector models: unknown model id, odd dims for a product, or a sphere / lorentz factor with "
                                       "fewer than two coordinates");
    return 0;
}

int grid_of(int64_t items, int G, unsigned& grid) {
    const int64_t blocks = (items * G + VEC_BLOCK - 1) / VEC_BLOCK;
    if (blocks > (int64_t)0x7fffffff) return fail(SYMPA_ERR_BAD_ARG, "vector models: more than 2^31-1 blocks in one launch; split the call");
    grid = (unsigned)blocks;
    return 0;
}

#define SYMPA_VEC_DISPATCH(KERNEL, G, grid, s, args, L)                                                      \
    switch (G) {                                                                                             \
        case 1: hipLaunchKernelGGL(KERNEL<1>, dim3(grid), dim3(VEC_BLOCK), 0, s, args, L); break;            \
        case 2: hipLaunchKernelGGL(KERNEL<2>, dim3(grid), dim3(VEC_BLOCK), 0, s, args, L); break;            \
        case 4: hipLaunchKernelGGL(KERNEL<4>, dim3(grid), dim3(VEC_BLOCK), 0, s, args, L); break;            \
        case 8: hipLaunchKernelGGL(KERNEL<8>, dim3(grid), dim3(VEC_BLOCK), 0, s, args, L); break;            \
        case 16: hipLaunchKernelGGL(KERNEL<16>, dim3(grid), dim3(VEC_BLOCK), 0, s, args, L); break;          \
        case 32: hipLaunchKernelGGL(KERNEL<32>, dim3(grid), dim3(VEC_BLOCK), 0, s, args, L); break;          \
        default: hipLaunchKernelGGL(KERNEL<64>, dim3(grid), dim3(VEC_BLOCK), 0, s, args, L); break;          \
    }

int launch_pair(VecPairArgs& a, int model, bool backward, void* stream) {
    if (a.b < 0) return fail(SYMPA_ERR_BAD_ARG, "negative batch size");
    VecLayout L;
    const int rc = check_dims(a.dims, model, L);
    if (rc != 0) return rc;
    if (a.b == 0) return 0;
    if (a.x == nullptr || a.y == nullptr) return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    if (!backward && a.out == nullptr) return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    if (backward && (a.gx == nullptr || a.gy == nullptr)) return fail(SYMPA_ERR_BAD_ARG, "null gradient row buffer");
    if (backward && a.go == nullptr && a.graph_dist == nullptr) return fail(SYMPA_ERR_BAD_ARG, "need grad_out or graph_dist");
    if ((a.src == nullptr) != (a.dst == nullptr)) return fail(SYMPA_ERR_BAD_ARG, "null index buffer");
    if (a.num_rows > (int64_t)0x7fffffff) return fail(SYMPA_ERR_BAD_ARG, "more than 2^31-1 table rows");
    const bool even = a.dims % 2 == 0;
    a.vec_load = (even && aligned16(a.x) && aligned16(a.y)) ? 1 : 0;
    a.vec_store = (backward && even && aligned16(a.gx) && aligned16(a.gy)) ? 1 : 0;
    const int G = sympa::vec_lanes(a.dims);
    unsigned grid;
    const int gc = grid_of(a.b, G, grid);
    if (gc != 0) return gc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (backward) {
        SYMPA_VEC_DISPATCH(vec_bwd_kernel, G, grid, s, a, L)
    } else {
        SYMPA_VEC_DISPATCH(vec_fwd_kernel, G, grid, s, a, L)
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

int launch_rows(VecRowArgs& a, int model, void* stream) {
    if (a.b < 0) return fail(SYMPA_ERR_BAD_ARG, "negative row count");
    VecLayout L;
    const int rc = check_dims(a.dims, model, L);
    if (rc != 0) return rc;
    if (a.b == 0) return 0;
    if (a.x == nullptr || (a.op != sympa::VR_PROJX && a.g == nullptr) || (a.op != sympa::VR_RSGD && a.out == nullptr))
        return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    const bool even = a.dims % 2 == 0;
    a.vec_x = (even && aligned16(a.x)) ? 1 : 0;
    a.vec_g = (even && a.g != nullptr && aligned16(a.g)) ? 1 : 0;
    a.vec_out = (even && a.out != nullptr && aligned16(a.out)) ? 1 : 0;
    const int G = sympa::vec_lanes(a.dims);
    unsigned grid;
    const int gc = grid_of(a.b, G, grid);
    if (gc != 0) return gc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SYMPA_VEC_DISPATCH(vec_row_kernel, G, grid, s, a, L)
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

int launch_radam(VecAdamArgs& a, int model, void* stream) {
    if (a.b < 0) return fail(SYMPA_ERR_BAD_ARG, "negative row count");
    VecLayout L;
    const int rc = check_dims(a.dims, model, L);
    if (rc != 0) return rc;
    if (!(a.beta1 >= 0.0 && a.beta1 < 1.0) || !(a.beta2 >= 0.0 && a.beta2 < 1.0))
        return fail(SYMPA_ERR_BAD_ARG, "sympa_vector_radam_step: betas must be in [0, 1)");
    if (!(a.eps > 0.0)) return fail(SYMPA_ERR_BAD_ARG, "sympa_vector_radam_step: eps_adam must be positive");
    if (a.b == 0) return 0;
    if (a.x == nullptr || a.g == nullptr || a.m == nullptr || a.s == nullptr || a.pows == nullptr)
        return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    const bool even = a.dims % 2 == 0;
    a.vec_x = (even && aligned16(a.x)) ? 1 : 0;
    a.vec_g = (even && aligned16(a.g)) ? 1 : 0;
    a.vec_m = (even && aligned16(a.m)) ? 1 : 0;
    a.vec_s = (even && aligned16(a.s)) ? 1 : 0;
    a.has_l = 0;
    for (int f = 0; f < L.nf; ++f) a.has_l |= (L.geom[f] == sympa::VG_L) ? 1 : 0;
    const int G = sympa::vec_lanes(a.dims);
    unsigned grid;
    const int gc = grid_of(a.b, G, grid);
    if (gc != 0) return gc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    SYMPA_VEC_DISPATCH(vec_radam_kernel, G, grid, s, a, L)
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

int scale_args(VecPairArgs& a, const double* scale, double scale_coef) {
    if (scale != nullptr && !(scale_coef != 0.0)) return fail(SYMPA_ERR_BAD_ARG, "scale_coef must be non-zero");
    a.scale = scale;
    a.inv_scale_coef = scale != nullptr ? 1.0 / scale_coef : 1.0;
    return 0;
}

}  // namespace

extern "C" {

int sympa_vector_dist_fwd(const double* x, const double* y, int64_t b, int dims, int model, double* out, int32_t* status,
                          int flags, void* stream) {
    (void)flags;
    VecPairArgs a{};
    a.x = x; a.y = y; a.b = b; a.num_rows = b; a.dims = dims; a.out = out; a.status = status; a.inv_scale_coef = 1.0;
    return launch_pair(a, model, false, stream);
}

int sympa_vector_model_forward(const double* table, int64_t num_rows, int dims, const int64_t* src, int64_t src_stride,
                               const int64_t* dst, int64_t dst_stride, int64_t b, int model, const double* scale,
                               double scale_coef, double* out, int32_t* status, int flags, void* stream) {
    (void)flags;
    if (b > 0 && (src == nullptr || dst == nullptr)) return fail(SYMPA_ERR_BAD_ARG, "null index buffer");
    if (num_rows <= 0 && b > 0) return fail(SYMPA_ERR_BAD_ARG, "empty table");
    VecPairArgs a{};
    a.x = table; a.y = table; a.src = src; a.dst = dst; a.src_stride = src_stride; a.dst_stride = dst_stride;
    a.num_rows = num_rows; a.b = b; a.dims = dims; a.out = out; a.status = status;
    const int rc = scale_args(a, scale, scale_coef);
    if (rc != 0) return rc;
    return launch_pair(a, model, false, stream);
}

int sympa_vector_all_pairs_dist(const double* table, int64_t num_rows, int dims, int64_t row_begin, int64_t row_count, int model,
                                const double* scale, double scale_coef, double* out, int32_t* status, int flags, void* stream) {
    (void)flags;
    if (num_rows <= 0) return fail(SYMPA_ERR_BAD_ARG, "empty table");
    if (row_begin < 0 || row_count < 0 || row_begin + row_count > num_rows) return fail(SYMPA_ERR_BAD_ARG, "row block outside the table");
    if (num_rows > (int64_t)0x7fffffff) return fail(SYMPA_ERR_BAD_ARG, "more than 2^31-1 table rows");
    VecPairArgs a{};
    a.x = table; a.y = table; a.num_rows = num_rows; a.b = row_count * num_rows; a.dims = dims; a.out = out; a.status = status;
    a.ap_cols = num_rows; a.ap_row0 = row_begin;
    const int rc = scale_args(a, scale, scale_coef);
    if (rc != 0) return rc;
    return launch_pair(a, model, false, stream);
}

int sympa_vector_backward_rows(const double* x, const double* y, int64_t num_rows, int dims, int model, const int64_t* src,
                               int64_t src_stride, const int64_t* dst, int64_t dst_stride, int64_t b, const double* scale,
                               double scale_coef, const double* grad_out, const double* graph_dist, double loss_scale,
                               double* loss, double* grad_x_rows, double* grad_y_rows, double* grad_scale, double* out,
                               int32_t* status, int flags, void* stream) {
    (void)flags;
    if (src != nullptr && num_rows <= 0 && b > 0) return fail(SYMPA_ERR_BAD_ARG, "empty table");
    VecPairArgs a{};
    a.x = x; a.y = y; a.src = src; a.dst = dst; a.src_stride = src_stride; a.dst_stride = dst_stride;
    a.num_rows = src != nullptr ? num_rows : b; a.b = b; a.dims = dims; a.out = out; a.status = status;
    a.go = grad_out; a.graph_dist = graph_dist; a.loss_scale = loss_scale; a.loss = loss;
    a.gx = grad_x_rows; a.gy = grad_y_rows; a.gscale = grad_scale;
    const int rc = scale_args(a, scale, scale_coef);
    if (rc != 0) return rc;
    return launch_pair(a, model, true, stream);
}

int sympa_vector_egrad2rgrad(const double* x, const double* u, int64_t b, int dims, int model, double* out, void* stream) {
    VecRowArgs a{};
    a.x = const_cast<double*>(x); a.g = u; a.out = out; a.b = b; a.dims = dims; a.op = sympa::VR_EGRAD2RGRAD;
    return launch_rows(a, model, stream);
}

int sympa_vector_projx(const double* x, int64_t b, int dims, int model, double* out, int32_t* projected_count, int32_t* status,
                       void* stream) {
    VecRowArgs a{};
    a.x = const_cast<double*>(x); a.out = out; a.b = b; a.dims = dims; a.op = sympa::VR_PROJX;
    a.projected = projected_count; a.status = status;
    return launch_rows(a, model, stream);
}

int sympa_vector_rsgd_step(double* table, const double* grad, int64_t num_rows, int dims, int model, double lr, double weight_decay,
                           const double* total_sqnorm, double max_norm, int32_t* projected_count, int32_t* status, void* stream) {
    VecRowArgs a{};
    a.x = table; a.g = grad; a.b = num_rows; a.dims = dims; a.op = sympa::VR_RSGD; a.lr = lr; a.wd = weight_decay;
    a.clip = total_sqnorm; a.max_norm = max_norm; a.projected = projected_count; a.status = status;
    return launch_rows(a, model, stream);
}

int sympa_vector_radam_step(double* table, const double* grad, double* exp_avg, double* exp_avg_sq, int64_t num_rows, int dims,
                            int model, double lr, double beta1, double beta2, double eps_adam, double weight_decay,
                            const double* bias_pows, const double* total_sqnorm, double max_norm, int32_t* projected_count,
                            int32_t* status, void* stream) {
    VecAdamArgs a{};
    a.x = table; a.g = grad; a.m = exp_avg; a.s = exp_avg_sq; a.b = num_rows; a.dims = dims;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps_adam; a.wd = weight_decay; a.pows = bias_pows;
    a.clip = total_sqnorm; a.max_norm = max_norm; a.projected = projected_count; a.status = status;
    return launch_radam(a, model, stream);
}

}  // extern "C"
