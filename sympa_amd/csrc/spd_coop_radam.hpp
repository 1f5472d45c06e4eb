// SPD model, RiemannianAdam step of the table rows with sixteen lanes per row (layout and DPP machinery of spd_coop.hpp, the
// row products of spd_coop_table.hpp).  Same formulas as spd_row_radam (spd_math_bwd.hpp):
//   S = coef sym(g) + wd x,  r = sym(x S x),  I = || L^T S L ||_F^2,  m1 = b1 sym(m) + (1 - b1) r,  s1 = b2 s + (1 - b2) I,
//   c = -lr / (1 - p1) / (sqrt(s1 / (1 - p2)) + eps),  P = m1 L^-T,  A = P P^T,  y = x + c m1 + 1/2 c^2 A,
//   R = A L^-T,  B = sym(R P^T),  m' = m1 + c A + 1/2 c^2 B
// Lane r of a group owns row r of every matrix.  Every cross-lane read (the DPP broadcasts, transpose_rows, group_sum) is
// executed by all 64 lanes outside divergent control flow; only the loads of s and the stores are predicated.  A phantom lane
// (r >= M) reads row 0, computes values nobody reads and is masked out of the one group sum.
#pragma once

#include "spd_coop_table.hpp"

namespace spd_coop {

struct SpdAdamArgs {
    double lr, beta1, beta2, eps, wd, max_norm;
    const double* pows;       // device pair (beta1^t, beta2^t) of this step
    const double* clip;       // device total squared gradient norm, or nullptr
};

template <int M>
__global__ __launch_bounds__(64) void spd_coop_radam_kernel(double* __restrict__ x, const double* __restrict__ g,
                                                            double* __restrict__ m, double* __restrict__ sq, const int64_t b,
                                                            const SpdAdamArgs p, int32_t* __restrict__ status, const int rounds) {
    __shared__ __attribute__((aligned(16))) double tbuf_all[4 * TBUF];
    const int lane = threadIdx.x;
    const int grp = lane >> 4, r = lane & 15;
    double* const tbuf = tbuf_all + grp * TBUF;
    constexpr int nn = M * M;
    const double coef = (p.clip != nullptr) ? fmin(1.0, p.max_norm / (sqrt(p.clip[0]) + 1e-6)) : 1.0;
    const double bc1 = 1.0 - p.pows[0], bc2 = 1.0 - p.pows[1];
    const double ob1 = 1.0 - p.beta1, ob2 = 1.0 - p.beta2;
    int st = 0, nbad = 0;
    for (int t = 0; t < rounds; ++t) {
        const int64_t first = ((int64_t)blockIdx.x * rounds + t) * 4;
        if (first >= b) break;                                   // wave-uniform
        const int64_t i = first + grp;
        const bool live = i < b;
        const int64_t ii = live ? i : b - 1;
        const double* px = x + ii * nn;
        const double* pg = g + ii * nn;
        const double* pm = m + ii * nn;
        const int rr = r < M ? r : 0;                       // a phantom lane reads row 0
        // every load of the three matrices of my row comes before any store below (same wave, program order)
        double xs[M], u[M], m1[M];
#pragma unroll
        for (int j = 0; j < M; ++j) {
            xs[j] = 0.5 * (px[rr * M + j] + px[j * M + rr]);
            u[j] = 0.5 * (pg[rr * M + j] + pg[j * M + rr]);
            m1[j] = 0.5 * (pm[rr * M + j] + pm[j * M + rr]);
        }
        double sv = 0.0;
        if (r == 0) sv = sq[ii];                            // one lane reads the row's second moment
#pragma unroll
        for (int j = 0; j < M; ++j) u[j] = sympa::d_fma(p.wd, xs[j], coef * u[j]);
        double l[M], rd[M];
        {
            double tt[M], pr[M];
            matmul_rows(xs, u, tt);                         // x S   (u settled)
#pragma unroll
            for (int j = 0; j < M; ++j) l[j] = xs[j];
            matmul_rows(tt, l, pr);                         // x S x (l = x, settled)
            transpose_rows(pr, tt, tbuf, r);
#pragma unroll
            for (int j = 0; j < M; ++j) m1[j] = sympa::d_fma(p.beta1, m1[j], ob1 * (0.5 * (pr[j] + tt[j])));
        }
        const bool pd = cholesky_rows(l, rd);
        // I = || L^T (S L) ||_F^2;  W = S L: W[me][j] = sum_{k >= j} S[me][k] L[k][j],  L[k][j] = register j of lane k
        double inner = 0.0;
        {
            double w[M], lt[M];
            sfor<0, M>([&](auto J) {
                constexpr int j = J;
                double a0 = 0.0, a1 = 0.0;
                sfor<j, M>([&](auto K) {
                    constexpr int k = K;
                    if constexpr (k % 2 == 0) fmac_bc<k>(a0, l[j], u[k]);
                    else fmac_bc<k>(a1, l[j], u[k]);
                });
                w[j] = settle(a0 + a1);
            });
            transpose_rows(l, lt, tbuf, r);                 // lt[k] = L[k][me]: the factor for k >= me, leftovers above
#pragma unroll
            for (int k = 0; k < M; ++k) lt[k] = (k >= r) ? lt[k] : 0.0;
            sfor<0, M>([&](auto J) {
                constexpr int j = J;
                double a0 = 0.0, a1 = 0.0;
                sfor<0, M>([&](auto K) {
                    constexpr int k = K;
                    if constexpr (k % 2 == 0) fmac_bc<k>(a0, w[j], lt[k]);
                    else fmac_bc<k>(a1, w[j], lt[k]);
                });
                const double z = a0 + a1;
                inner = sympa::d_fma(z, z, inner);
            });
        }
        inner = fmax(group_sum(r < M ? inner : 0.0), 0.0);
        const double s0 = bcast<0>(settle(sv));
        const double s1 = sympa::d_fma(p.beta2, s0, ob2 * inner);
        const double c = -p.lr / bc1 / (sympa::d_sqrt(s1 / bc2) + p.eps);
        const double hc2 = 0.5 * c * c;
        double pp[M], a[M];
#pragma unroll
        for (int j = 0; j < M; ++j) pp[j] = m1[j];
        solve_right_lt(pp, l, rd);                          // rows of P = m1 L^-T
#pragma unroll
        for (int j = 0; j < M; ++j) pp[j] = settle(pp[j]);
        sfor<0, M>([&](auto J) {                            // A = P P^T: my register k times lane j's register k
            constexpr int j = J;
            double a0 = 0.0, a1 = 0.0;
            sfor<0, M>([&](auto K) {
                constexpr int k = K;
                if constexpr (k % 2 == 0) fmac_bc<j>(a0, pp[k], pp[k]);
                else fmac_bc<j>(a1, pp[k], pp[k]);
            });
            a[j] = a0 + a1;
        });
        if (live && r < M) {
            double* po = x + i * nn + r * M;
#pragma unroll
            for (int j = 0; j < M; ++j) po[j] = sympa::d_fma(hc2, a[j], sympa::d_fma(c, m1[j], xs[j]));
            if (r == 0) sq[i] = s1;
        }
        double bb[M], bt[M];
        {
            double rs[M];
#pragma unroll
            for (int j = 0; j < M; ++j) rs[j] = a[j];
            solve_right_lt(rs, l, rd);                      // rows of R = A L^-T
            sfor<0, M>([&](auto J) {                        // R P^T
                constexpr int j = J;
                double a0 = 0.0, a1 = 0.0;
                sfor<0, M>([&](auto K) {
                    constexpr int k = K;
                    if constexpr (k % 2 == 0) fmac_bc<j>(a0, pp[k], rs[k]);
                    else fmac_bc<j>(a1, pp[k], rs[k]);
                });
                bb[j] = a0 + a1;
            });
        }
        transpose_rows(bb, bt, tbuf, r);
        if (live && r < M) {
            double* po = m + i * nn + r * M;
#pragma unroll
            for (int j = 0; j < M; ++j) po[j] = sympa::d_fma(hc2, 0.5 * (bb[j] + bt[j]), sympa::d_fma(c, a[j], m1[j]));
        }
        if (live && !pd && r == 0) { st |= sympa::ST_NOT_PD; ++nbad; }
    }
    if (status != nullptr) {
        if (__ballot(st != 0) != 0ull) {
            if (st != 0) atomicOr(&status[0], st);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) nbad += __shfl_xor(nbad, off);
            if (lane == 0) atomicAdd(&status[1], nbad);          // rows flagged
        }
    }
}

template <int M>
inline void launch_spd_coop_radam_m(double* x, const double* g, double* m, double* sq, int64_t b, const SpdAdamArgs& p,
                                    int32_t* status, hipStream_t s) {
    const int rounds = coop_rounds(b);
    const dim3 grid((unsigned)((b + 4 * rounds - 1) / (4 * rounds)));
    hipLaunchKernelGGL((spd_coop_radam_kernel<M>), grid, dim3(64), 0, s, x, g, m, sq, b, p, status, rounds);
}

}  // namespace spd_coop
