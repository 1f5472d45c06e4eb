// SPD model: exponential map, logarithm, geodesic and the geodesic RSGD step with sixteen lanes per row / pair (layout and DPP
// machinery of spd_coop.hpp, the eigen-decomposition of spd_coop_bwd.hpp).  Same formulas as spd_expmap_math.hpp (DESIGN.md
// section 28):   out = (x +) L V diag(f) V^T L^T,   A = V diag(a) V^T,   x = L L^T
//   maps:  A = L^-1 W L^-T  (W = sym(u) or y - x: two solves and a transpose, as the backward's front)
//   step:  A = L^T S L      (S = coef sym(g) + wd x: two triangular products, no solve)
// Lane r of a group owns row r of every matrix.  Every cross-lane read (the DPP broadcasts, transpose_rows, group_sum, the wave
// vote of the QL) is executed by all 64 lanes outside divergent control flow; only the stores are predicated.  A phantom lane
// (r >= M) reads element 0 / row 0 and computes values nobody reads; a past-the-end group recomputes the last row and does not
// store.  The QL iteration ends when all four groups of the wave agree (tridiag_ql_vectors_row).
#pragma once

#include <cmath>

#include "siegel_common.hpp"
#include "spd_coop_bwd.hpp"
#include "spd_coop_table.hpp"
#include "spd_expmap_math.hpp"

namespace sympa_hip {
// op: sympa::SPD_MAP_EXP / SPD_MAP_LOG / SPD_MAP_GEODESIC (x, p2 -> out) or SPD_EXPMAP_OP_STEP (x in place, p2 = the gradient)
constexpr int SPD_EXPMAP_OP_STEP = 3;
constexpr int SPD_EXPMAP_COOP_MIN_N = 3;      // below: one row per lane (spd_expmap.hip)
// sixteen lanes per row / pair: n = 3..11 (spd_expmap_coop_lo.hip), n = 12..16 (spd_expmap_coop_hi.hip)
void launch_spd_coop_expmap_lo(int op, int n, double* x, const double* p2, double t, int64_t b, double* out, double lr, double wd,
                               const double* clip, double max_norm, int32_t* status, hipStream_t s);
void launch_spd_coop_expmap_hi(int op, int n, double* x, const double* p2, double t, int64_t b, double* out, double lr, double wd,
                               const double* clip, double max_norm, int32_t* status, hipStream_t s);
}  // namespace sympa_hip

namespace spd_coop {

// a <- L^T (S L) for the rows held one per lane: s = my row of the symmetric S, l = my row of L (register k of lane i >= k)
template <int M>
__device__ __forceinline__ void ltsl_rows(double (&s)[M], double (&l)[M], double (&a)[M], double* __restrict__ tbuf, const int r) {
    double w[M], lt[M];
    sfor<0, M>([&](auto J) { s[J] = settle(s[J]); l[J] = settle(l[J]); });
    sfor<0, M>([&](auto J) {                            // W = S L:  W[me][j] = sum_{k >= j} S[me][k] L[k][j]
        constexpr int j = J;
        double a0 = 0.0, a1 = 0.0;
        sfor<j, M>([&](auto K) {
            constexpr int k = K;
            if constexpr (k % 2 == 0) fmac_bc<k>(a0, l[j], s[k]);
            else fmac_bc<k>(a1, l[j], s[k]);
        });
        w[j] = settle(a0 + a1);
    });
    transpose_rows(l, lt, tbuf, r);                     // lt[k] = L[k][me]: the factor for k >= me, leftovers above
#pragma unroll
    for (int k = 0; k < M; ++k) lt[k] = (k >= r) ? lt[k] : 0.0;
    sfor<0, M>([&](auto J) {                            // A = L^T W:  A[me][j] = sum_k L[k][me] W[k][j]
        constexpr int j = J;
        double a0 = 0.0, a1 = 0.0;
        sfor<0, M>([&](auto K) {
            constexpr int k = K;
            if constexpr (k % 2 == 0) fmac_bc<k>(a0, w[j], lt[k]);
            else fmac_bc<k>(a1, w[j], lt[k]);
        });
        a[j] = a0 + a1;
    });
}

// p <- sym(L p L^T) for the rows held one per lane (l: register k of lane i >= k is L[i][k]; the leftovers above are masked)
template <int M>
__device__ __forceinline__ void congruence_l_rows(double (&p)[M], const double (&l)[M], double* __restrict__ tbuf, const int r) {
    double lz[M], t[M], o[M], ot[M];
#pragma unroll
    for (int k = 0; k < M; ++k) lz[k] = settle((k <= r) ? l[k] : 0.0);
    matmul_rows(lz, p, t);                              // T = L P
    sfor<0, M>([&](auto J) {                            // T L^T:  sum_{k <= j} T[me][k] L[j][k], lane j's register k times mine
        constexpr int j = J;
        double a0 = 0.0, a1 = 0.0;
        sfor<0, j + 1>([&](auto K) {
            constexpr int k = K;
            if constexpr (k % 2 == 0) fmac_bc<j>(a0, lz[k], t[k]);
            else fmac_bc<j>(a1, lz[k], t[k]);
        });
        o[j] = a0 + a1;
    });
    transpose_rows(o, ot, tbuf, r);
#pragma unroll
    for (int j = 0; j < M; ++j) p[j] = 0.5 * (o[j] + ot[j]);
}

// The factor is needed before the eigen-decomposition and after it, not inside, and the reflectors are not needed inside the QL
// iteration: they wait in LDS meanwhile (2 KB per group each), which is what keeps the large instantiations out of scratch memory.  Every lane writes and reads only its own 16 doubles.
template <int M>
__device__ __forceinline__ void park_rows(const double (&l)[M], double* __restrict__ lpark, const int r) {
    sfor<0, M>([&](auto J) { lpark[r * N + J] = l[J]; });
    wave_lds_fence();
}
template <int M>
__device__ __forceinline__ void unpark_rows(double (&l)[M], const double* __restrict__ lpark, const int r) {
    wave_lds_fence();
    sfor<0, M>([&](auto J) { l[J] = lpark[r * N + J]; });
}

// m = my row of the symmetric A (destroyed) -> d = its eigenvalues (group-uniform), vrow = my row of V; returns "the QL converged"
template <int M>
__device__ __forceinline__ bool eigh_rows(double (&m)[M], double (&d)[M], double (&vrow)[M], double* __restrict__ tbuf,
                                          double* __restrict__ vpark, const int r) {
    // SLIM (M >= 13, where the reflectors, their beta and the QL's state do not fit 512 registers next to the factor): NORMALISED
    // reflectors, P_k = I - w_k w_k^T with w = sqrt(beta) v, as spd_coop_bwd2_kernel keeps them -- no beta array through the QL
    constexpr bool SLIM = M >= 13;
    // A arrives symmetric up to the rounding of the two solves (or products), whose skew part is as large as their whole error;
    // the tridiagonalisation reads columns as rows, so the skew part goes first (the one-lane arithmetic symmetrises A as well)
    {
        double mt[M];
        transpose_rows(m, mt, tbuf, r);
#pragma unroll
        for (int j = 0; j < M; ++j) m[j] = 0.5 * (m[j] + mt[j]);
    }
    double e[M], vk[M], bk[M];
    tridiagonalize_keep(m, r, d, e, vk, bk);
    if constexpr (SLIM) {
#pragma unroll
        for (int j = 0; j < M; ++j) { vk[j] *= sympa::d_sqrt(bk[j]); bk[j] = 1.0; }
    }
    // the QL runs redundantly in the sixteen lanes and its predicates must agree bit for bit (spd_coop_bwd_kernel.hpp)
#pragma unroll
    for (int j = 0; j < M; ++j) { d[j] = bcast<0>(d[j]); e[j] = bcast<0>(e[j]); }
    double zrow[M], zc[M];
#pragma unroll
    for (int j = 0; j < M; ++j) zrow[j] = (r == j) ? 1.0 : 0.0;
    park_rows(vk, vpark, r);
    const bool conv = tridiag_ql_vectors_row(d, e, zrow);
    transpose_rows(zrow, zc, tbuf, r);                  // lane c holds column c of Z
    unpark_rows(vk, vpark, r);
    back_transform_columns(zc, vk, bk);                 // ... of V = Q Z
    transpose_rows(zc, vrow, tbuf, r);                  // lane i holds row i of V
    return conv;
}

// f[k] = fn(d[k]) for the group-uniform eigenvalues d: lane k of the group evaluates fn ONCE, on d[k], and the sixteen results are
// broadcast (one transcendental chain per lane instead of M interleaved ones: their temporaries would not fit the registers).
// Returns the bitmask of the lanes k < M of my group whose fn flagged its value (bit 0 of the flags: not in the domain; bit 1:
// not finite) as two group-uniform booleans.
template <int M, class F>
__device__ __forceinline__ void spectral_function(const double (&d)[M], double (&f)[M], const int grp, const int r, bool& domain,
                                                  bool& finite, F&& fn) {
    double mine = d[0];
    sfor<1, M>([&](auto K) { mine = (r == K) ? d[K] : mine; });
    bool in_domain = true;
    const double fr = fn(mine, in_domain);
    const unsigned long long out_of_domain = __ballot(r < M && !in_domain), nonfinite = __ballot(r < M && !sympa::d_finite(fr));
    domain = ((out_of_domain >> (16 * grp)) & 0xffffull) == 0ull;
    finite = ((nonfinite >> (16 * grp)) & 0xffffull) == 0ull;
    sfor<0, M>([&](auto K) { f[K] = bcast<K>(fr); });
}

__device__ __forceinline__ void coop_status(int32_t* __restrict__ status, const int st, int nbad, const int lane) {
    if (status != nullptr) {
        if (__ballot(st != 0) != 0ull) {
            if (st != 0) atomicOr(&status[0], st);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) nbad += __shfl_xor(nbad, off);
            if (lane == 0) atomicAdd(&status[1], nbad);          // rows flagged
        }
    }
}

// kind: sympa::SPD_MAP_EXP (p2 = u), SPD_MAP_LOG / SPD_MAP_GEODESIC (p2 = y); wave-uniform.  KIND >= 0: the kind at compile time
// (M = 16: with the three maps behind a run-time kind the instantiation needs 76 bytes of scratch memory, apart it needs none).
template <int M, int KIND = -1>
__global__ __launch_bounds__(64) void spd_coop_map_kernel(const int kind_arg, const double* __restrict__ x, const double* __restrict__ p2,
                                                          const double tpar, const int64_t b, double* __restrict__ out,
                                                          int32_t* __restrict__ status, const int rounds) {
    __shared__ __attribute__((aligned(16))) double tbuf_all[4 * TBUF];
    __shared__ __attribute__((aligned(16))) double lpark_all[4 * 2 * N * N];
    const int lane = threadIdx.x;
    const int grp = lane >> 4, r = lane & 15;
    double* const tbuf = tbuf_all + grp * TBUF;
    double* const lpark = lpark_all + grp * 2 * N * N;      // the factor, then the reflectors
    constexpr int nn = M * M;
    const int kind = KIND >= 0 ? KIND : kind_arg;
    int st = 0, nbad = 0;
    for (int t = 0; t < rounds; ++t) {
        const int64_t first = ((int64_t)blockIdx.x * rounds + t) * 4;
        if (first >= b) break;                                   // wave-uniform
        const int64_t i = first + grp;
        const bool live = i < b;
        const int64_t ii = live ? i : b - 1;
        const double* px = x + ii * nn;
        const double* pp = p2 + ii * nn;
        double l[M], w[M];
        if (kind == sympa::SPD_MAP_EXP) {                        // (wave-uniform)
#pragma unroll
            for (int j = 0; j < M; ++j) {
                const int lo = r < j ? r : j, hi = r < j ? j : r;
                const bool real = hi < M;                        // upper triangle; a phantom lane reads element 0
                l[j] = px[real ? lo * M + hi : 0];
                w[j] = 0.5 * (pp[real ? lo * M + hi : 0] + pp[real ? hi * M + lo : 0]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < M; ++j) {
                const int lo = r < j ? r : j, hi = r < j ? j : r;
                const int e = (hi < M) ? lo * M + hi : 0;
                l[j] = px[e];
                w[j] = pp[e] - l[j];
            }
        }
        double rd[M], m[M];
        const bool pd = cholesky_rows(l, rd);
        solve_right_lt(w, l, rd);                                // W L^-T
        transpose_rows(w, m, tbuf, r);
        solve_right_lt(m, l, rd);                                // A = L^-1 W L^-T
        park_rows(l, lpark, r);
        double d[M], vrow[M], f[M], p[M];
        const bool conv = eigh_rows(m, d, vrow, tbuf, lpark + N * N, r);
        bool dom, fin;
        spectral_function(d, f, grp, r, dom, fin, [&](const double a, bool& in_domain) {
            if (kind == sympa::SPD_MAP_EXP) return std::expm1(a);
            in_domain = a > -1.0;
            const double lg = sympa::d_log1p_signed(a);
            return (kind == sympa::SPD_MAP_LOG) ? lg : std::expm1(tpar * lg);
        });
        const bool ok = pd && dom;
        vdvt_rows(vrow, f, p);
        unpark_rows(l, lpark, r);
        congruence_l_rows(p, l, tbuf, r);
        if (live && r < M) {
            double* po = out + i * nn + r * M;
#pragma unroll
            for (int j = 0; j < M; ++j) {
                // (x read again, not kept through the QL: 2 M registers; out aliases nothing)
                const double val = (kind == sympa::SPD_MAP_LOG) ? p[j] : px[r < j ? r * M + j : j * M + r] + p[j];
                po[j] = ok ? val : __builtin_nan("");
            }
        }
        if (live && r == 0) {
            int s = 0;
            if (!ok) s |= sympa::ST_NOT_PD;
            if (!conv) s |= sympa::ST_NO_CONVERGENCE;
            if (ok && !fin) s |= sympa::ST_NONFINITE;
            st |= s;
            nbad += (s != 0) ? 1 : 0;
        }
    }
    coop_status(status, st, nbad, lane);
}

// the geodesic RSGD step of the table rows in place; every load of a row stands before its stores (same wave, program order)
template <int M>
__global__ __launch_bounds__(64) void spd_coop_rsgd_exp_kernel(double* __restrict__ x, const double* __restrict__ g, const int64_t b,
                                                               const double lr, const double wd, const double* __restrict__ clip,
                                                               const double max_norm, int32_t* __restrict__ status, const int rounds) {
    __shared__ __attribute__((aligned(16))) double tbuf_all[4 * TBUF];
    __shared__ __attribute__((aligned(16))) double lpark_all[4 * 2 * N * N];
    const int lane = threadIdx.x;
    const int grp = lane >> 4, r = lane & 15;
    double* const tbuf = tbuf_all + grp * TBUF;
    double* const lpark = lpark_all + grp * 2 * N * N;      // the factor, then the reflectors
    constexpr int nn = M * M;
    const double coef = (clip != nullptr) ? fmin(1.0, max_norm / (sqrt(clip[0]) + 1e-6)) : 1.0;
    int st = 0, nbad = 0;
    for (int t = 0; t < rounds; ++t) {
        const int64_t first = ((int64_t)blockIdx.x * rounds + t) * 4;
        if (first >= b) break;                                   // wave-uniform
        const int64_t i = first + grp;
        const bool live = i < b;
        const int64_t ii = live ? i : b - 1;
        const double* px = x + ii * nn;
        const double* pg = g + ii * nn;
        const int rr = r < M ? r : 0;                            // a phantom lane reads row 0
        double xs[M], s[M];
#pragma unroll
        for (int j = 0; j < M; ++j) {
            xs[j] = 0.5 * (px[rr * M + j] + px[j * M + rr]);
            s[j] = 0.5 * (pg[rr * M + j] + pg[j * M + rr]);
        }
#pragma unroll
        for (int j = 0; j < M; ++j) s[j] = sympa::d_fma(wd, xs[j], coef * s[j]);
        double l[M], rd[M], m[M];
#pragma unroll
        for (int j = 0; j < M; ++j) l[j] = xs[j];
        const bool pd = cholesky_rows(l, rd);
        ltsl_rows(s, l, m, tbuf, r);                             // A = L^T S L
        park_rows(l, lpark, r);
        double d[M], vrow[M], f[M], p[M];
        const bool conv = eigh_rows(m, d, vrow, tbuf, lpark + N * N, r);
        bool dom, fin;
        spectral_function(d, f, grp, r, dom, fin, [&](const double c, bool&) { return std::expm1(-lr * c); });
        vdvt_rows(vrow, f, p);
        unpark_rows(l, lpark, r);
        congruence_l_rows(p, l, tbuf, r);
        if (live && r < M) {
            // sym(x) read again, not kept through the QL -- the whole row before the first store: the column entries are other
            // lanes' rows, which their store instructions below would already have replaced
            double xv[M];
#pragma unroll
            for (int j = 0; j < M; ++j) xv[j] = 0.5 * (px[r * M + j] + px[j * M + r]);
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __builtin_amdgcn_s_waitcnt(0x0070);                  // vmcnt(0): every load of the wave has returned
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            double* po = x + i * nn + r * M;
#pragma unroll
            for (int j = 0; j < M; ++j) po[j] = pd ? xv[j] + p[j] : __builtin_nan("");
        }
        if (live && r == 0) {
            int sb = 0;
            if (!pd) sb |= sympa::ST_NOT_PD;
            if (!conv) sb |= sympa::ST_NO_CONVERGENCE;
            if (pd && !fin) sb |= sympa::ST_NONFINITE;
            st |= sb;
            nbad += (sb != 0) ? 1 : 0;
        }
    }
    coop_status(status, st, nbad, lane);
}

template <int M>
inline void launch_spd_coop_expmap_m(int op, double* x, const double* p2, double t, int64_t b, double* out, double lr, double wd,
                                     const double* clip, double max_norm, int32_t* status, hipStream_t s) {
    const int rounds = coop_rounds(b);
    const dim3 grid((unsigned)((b + 4 * rounds - 1) / (4 * rounds)));
    if (op == sympa_hip::SPD_EXPMAP_OP_STEP)
        hipLaunchKernelGGL((spd_coop_rsgd_exp_kernel<M>), grid, dim3(64), 0, s, x, p2, b, lr, wd, clip, max_norm, status, rounds);
    else if constexpr (M < 16)
        hipLaunchKernelGGL((spd_coop_map_kernel<M>), grid, dim3(64), 0, s, op, x, p2, t, b, out, status, rounds);
    else if (op == sympa::SPD_MAP_EXP)
        hipLaunchKernelGGL((spd_coop_map_kernel<M, sympa::SPD_MAP_EXP>), grid, dim3(64), 0, s, op, x, p2, t, b, out, status, rounds);
    else if (op == sympa::SPD_MAP_LOG)
        hipLaunchKernelGGL((spd_coop_map_kernel<M, sympa::SPD_MAP_LOG>), grid, dim3(64), 0, s, op, x, p2, t, b, out, status, rounds);
    else
        hipLaunchKernelGGL((spd_coop_map_kernel<M, sympa::SPD_MAP_GEODESIC>), grid, dim3(64), 0, s, op, x, p2, t, b, out, status, rounds);
}

}  // namespace spd_coop
