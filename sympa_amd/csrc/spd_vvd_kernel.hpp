// Kernels of the SPD model's differentiable vector-valued distance:  v_j = log(1 + a_j) ascending and signed,
// a = the eigenvalues of A = L^-1 (y - x) L^-T, x = L L^T.  Kernels of their own beside spd16_coop_kernel (spd.hip) and
// spd_coop_bwd_kernel (spd_coop_bwd_kernel.hpp), which stay as they are; same routines (spd_coop.hpp, spd_coop_bwd.hpp).
//   forward   n <= 5 / SYMPA_FLAG_GENERIC: spd_vvd_fwd_kernel (one lane per pair, spd_math.hpp spd_pair_vvd)
//             n = 6..16: spd_vvd_coop_fwd_kernel<n> -- the rounds of spd16_coop_kernel (rows loaded by the lanes themselves at every
//             n, no LDS-DMA tile), then each lane ranks its pair's eigenvalues and the rows of v leave through the LDS, coalesced
//   backward  n <= 2 / SYMPA_FLAG_GENERIC: spd_vvd_bwd_kernel (one lane per pair, spd_math_bwd.hpp spd_pair_backward_vvd)
//             n = 3..16: spd_vvd_coop_bwd_kernel<n> -- spd_coop_bwd_kernel with the spectral weights log(1 + a_k) / dist replaced by
//             the pair's cotangent row, gv[i, rank(k)]; dense rows or the in-kernel scatter (scatter_plane)
// Instantiated in spd_vvd_fwd_coop_{lo,hi}.hip and spd_vvd_bwd_coop_{lo,mid,hi}.hip; launched from spd_vvd.hip.
#pragma once

#include "siegel_common.hpp"
#include "spd_coop_bwd.hpp"
#include "spd_math_bwd.hpp"

namespace sympa_hip {

struct SpdVvdArgs {
    const double* x;          // [.., n, n] points or the table
    const double* y;
    const int64_t* src;       // nullptr -> pair i = rows i
    const int64_t* dst;
    int64_t src_stride, dst_stride;
    int64_t num_rows, b;
    const double* gv;         // [b, n] cotangent on the ascending v (backward)
    double* gtab;             // scatter form: [num_rows, n, n] table gradient, accumulated with atomics (gx, gy unused); or null
    double* gx;               // [b, n, n] rows of the src / x points
    double* gy;               // [b, n, n] rows of the dst / y points
    double* vvd;              // [b, n] (the backward: or null)
    int32_t* status;
};

constexpr int SPD_VVD_COOP_FWD_MIN_N = 6;      // the crossovers of the distance kernels (spd.hip, spd_coop_bwd_kernel.hpp)
constexpr int SPD_VVD_COOP_BWD_MIN_N = 3;

template <int M>
constexpr int spd_vvd_coop_bwd_waves() { return M <= 11 ? 2 : 1; }

inline dim3 spd_vvd_coop_bwd_grid(const int64_t b, const int n) {
    const int rounds = spd_coop::coop_rounds(b, n <= 11 ? 2 : 1);
    return dim3((unsigned)((b + 4 * rounds - 1) / (4 * rounds)));
}

void launch_spd_vvd_fwd_one_lane(const SpdVvdArgs& a, int n, hipStream_t s);
void launch_spd_vvd_bwd_one_lane(const SpdVvdArgs& a, int n, hipStream_t s);
void launch_spd_vvd_fwd_coop_lo(const SpdVvdArgs& a, int n, hipStream_t s);     // n = 6..11
void launch_spd_vvd_fwd_coop_hi(const SpdVvdArgs& a, int n, hipStream_t s);     // n = 12..16
void launch_spd_vvd_bwd_coop_lo(const SpdVvdArgs& a, int n, hipStream_t s);     // n = 3..9
void launch_spd_vvd_bwd_coop_mid(const SpdVvdArgs& a, int n, hipStream_t s);    // n = 10..13
void launch_spd_vvd_bwd_coop_hi(const SpdVvdArgs& a, int n, hipStream_t s);     // n = 14..16

__device__ __forceinline__ void spd_vvd_report(int32_t* status, const int st, const bool counted, const int lane) {
    if (status != nullptr) {
        const unsigned long long mk = __ballot(counted && st != 0);
        if (mk != 0ull) {
            if (counted && st != 0) atomicOr(&status[0], st);
            if (lane == 0) atomicAdd(&status[1], (int)__popcll(mk));
        }
    }
}

// Eigenvalues of the tridiagonal (d, e2) of every lane's own pair, PWK QL (dsterf) stage by stage like sympa::tridiag_ql_lockstep
// (siegel_math.hpp), deflation at eps^2 -- but a lane whose position L has deflated is FROZEN for the rest of the stage: it runs the
// wave's sweeps (one instruction stream) and keeps its values.  tridiag_ql_lockstep lets such a lane sweep ahead, so the last bits of
// a pair depend on how long the slowest pair of its wave takes; here a row of v depends on its own pair alone, whatever shares the
// wave: a bad index next to it, the tail of the batch, another batch size.
template <int N, int L>
__device__ __forceinline__ bool spd_vvd_ql_stage(double (&d)[N], double (&e2)[N]) {
    bool conv = false;
    for (int it = 0; it < 60; ++it) {
        conv = sympa::ql_deflated<true>(e2[L], d[L], d[L + 1], sympa::QL_DEFLATE_TOL_EXACT);
        if (sympa::wave_all(conv)) break;
        const double el = conv ? 1.0 : e2[L];                     // (a frozen lane computes on a harmless value and discards it)
        const double irte = sympa::d_rsqrt(el);
        const double rte = el * irte;
        const double sg = 0.5 * (d[L + 1] - d[L]) * irte;
        const double rr = sympa::d_sqrt(sympa::d_fma(sg, sg, 1.0));
        const double sigma = d[L] - rte * sympa::d_rcp(sg + copysign(rr, sg));      // Wilkinson shift
        double c = 1.0, sn = 0.0, gamma = d[N - 1] - sigma, p = gamma * gamma;
#pragma unroll
        for (int i = N - 2; i >= L; --i) {
            const double bb = e2[i];
            const double r = p + bb;
            if (i != N - 2) e2[i + 1] = conv ? e2[i + 1] : sn * r;
            const double oldc = c;
            const double rs = fmax(r, sympa::TINY);               // r = 0 (decoupled and converged) gives c = 1, s = 0
            const double ir = sympa::d_rcp(rs);
            c = (p + (rs - r)) * ir;
            sn = bb * ir;
            const double oldgam = gamma;
            const double alpha = d[i];
            gamma = sympa::d_fma(c, alpha - sigma, -sn * oldgam);
            d[i + 1] = conv ? d[i + 1] : oldgam + (alpha - gamma);
            const double pn = gamma * gamma * sympa::d_rcp(c);
            const double pz = oldc * bb;
            p = (c != 0.0) ? pn : pz;
        }
        e2[L] = conv ? e2[L] : sn * p;
        d[L] = conv ? d[L] : sigma + gamma;
    }
    return conv;
}

template <int N, int L = 0>
__device__ __forceinline__ bool spd_vvd_ql(double (&d)[N], double (&e2)[N]) {
    if constexpr (L >= N - 1) {
        return true;
    } else {
        const bool here = spd_vvd_ql_stage<N, L>(d, e2);
        const bool rest = spd_vvd_ql<N, L + 1>(d, e2);
        return here && rest;
    }
}

// Forward, sixteen lanes per pair for the factorisation, the solves and the first M - TB Householder steps, one lane per pair
// for the trailing block, the QL and the ranking: the structure of spd16_coop_kernel<M, false> (spd.hip; see there and spd_coop.hpp).
// One wave per block, 64 pairs per wave; lane 16 g + t owns pair 4 t + g of the wave's 64.  After the QL each lane holds its pair's
// eigenvalues; a lane writing its M doubles at a stride of 8 M bytes would be an uncoalesced store, so the rows go through the
// wave's LDS tile (free by then) and leave as 64 M consecutive doubles.
template <int M>
__global__ __launch_bounds__(64, (spd_coop::trailing_block<M>() <= 10 ? 2 : 1)) void spd_vvd_coop_fwd_kernel(const SpdVvdArgs a) {
    using namespace spd_coop;
    constexpr int TB = trailing_block<M>();
    constexpr int TILE = GROUPS_PER_WAVE * TBUF > 64 * M ? GROUPS_PER_WAVE * TBUF : 64 * M;      // doubles: transposes, then the rows of v
    __shared__ __attribute__((aligned(16))) double tile[TILE];
    __shared__ __attribute__((aligned(16))) double hand_all[GROUPS_PER_WAVE * (TB >= 3 ? TB * TB : 2) + (TB >= 3 ? TB + (TB & 1) : 0)];
    const int lane = threadIdx.x;
    const int g = lane >> 4, r = lane & 15;
    double* const hand = hand_all + g * (TB >= 3 ? TB * TB : 2);
    const int slot = 4 * r + g;                                    // my pair among the wave's 64
    const int64_t i = (int64_t)blockIdx.x * 64 + slot;
    const bool live = i < a.b;
    const int64_t ii = live ? i : a.b - 1;
    int st = 0;
    int64_t r1 = ii, r2 = ii;
    if (a.src != nullptr) {
        r1 = a.src[ii * a.src_stride];
        r2 = a.dst[ii * a.dst_stride];
        if (r1 < 0 || r1 >= a.num_rows || r2 < 0 || r2 >= a.num_rows) { st |= sympa::ST_BAD_INDEX; r1 = 0; r2 = 0; }
    }
    const int row1 = (int)r1, row2 = (int)r2;      // num_rows < 2^31 (checked on the host)
    double d[M], e2[M], blk[packed_len<TB>()];
#pragma unroll
    for (int k = 0; k < M; ++k) { d[k] = 0.0; e2[k] = 0.0; }
#pragma unroll
    for (int k = 0; k < packed_len<TB>(); ++k) blk[k] = 0.0;
    bool ok = true;
    for (int t = 0; t < ROUNDS; ++t) {
        double x[M], y[M];
        const int rowx = __builtin_amdgcn_ds_bpermute(4 * (16 * g + t), row1);     // rows of my group's pair
        const int rowy = __builtin_amdgcn_ds_bpermute(4 * (16 * g + t), row2);
        const double* px = a.x + (size_t)(unsigned)rowx * (unsigned)(M * M);
        const double* py = a.y + (size_t)(unsigned)rowy * (unsigned)(M * M);
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int lo = r < j ? r : j, hi = r < j ? j : r;
            const int e = (hi < M) ? lo * M + hi : 0;          // a phantom lane (r >= M) reads element 0
            x[j] = px[e];
            y[j] = py[e];
        }
        if constexpr (TB >= 3) {
            wave_lds_fence();
            if (t > 0 && r == t - 1) take_block<TB>(blk, hand);
        }
        double rdl, m[M];
        const bool pd = reduce_pair_front(x, y, rdl, m, tile + g * TBUF, r);
        wave_lds_fence();
        const bool keep = (r == t);
        ok = keep ? pd : ok;
        reduce_pair_back<M, TB>(m, x, rdl, r, keep, 0x0001000100010001ull << t, d, e2, hand,
                                hand_all + GROUPS_PER_WAVE * (TB >= 3 ? TB * TB : 2));
    }
    if constexpr (TB >= 3) {
        wave_lds_fence();
        if (r == ROUNDS - 1) take_block<TB>(blk, hand);
    }
    // one pair per lane from here
    if constexpr (TB >= 3) sympa::tridiag_packed<TB>(blk, d + (M - TB), e2 + (M - TB));
    {   // (the QL from the end of the Householder form, as in spd16_coop_kernel)
        double dr[M], er[M];
#pragma unroll
        for (int k = 0; k < M; ++k) { dr[k] = d[M - 1 - k]; er[k] = (k < M - 1) ? e2[M - 2 - k] : 0.0; }
#pragma unroll
        for (int k = 0; k < M; ++k) { d[k] = dr[k]; e2[k] = er[k]; }
    }
    // a general function of v weights every eigenvalue by itself: deflation at eps^2, as for the Siegel v (siegel_math.hpp)
    const bool conv = spd_vvd_ql<M>(d, e2);
    bool fin = true;
    wave_lds_fence();                                              // the transposes of the last round are consumed
#pragma unroll
    for (int k = 0; k < M; ++k) {
        ok = ok && (d[k] > -1.0);
        double lg = sympa::d_log1p_signed(d[k]);
        fin = fin && sympa::d_finite(lg);
        int rk = 0;
#pragma unroll
        for (int mm = 0; mm < M; ++mm) rk += (d[mm] < d[k] || (d[mm] == d[k] && mm < k)) ? 1 : 0;
        if (st & sympa::ST_BAD_INDEX) lg = __builtin_nan("");
        tile[slot * M + rk] = lg;                                  // rk < M: at most M - 1 others compare below
    }
    wave_lds_fence();
    {
        const int64_t first = (int64_t)blockIdx.x * 64;
        const int64_t left = a.b - first;
        const int count = (int)(left < 64 ? left : 64) * M;        // doubles of this wave's live pairs
        double* out = a.vvd + first * M;
#pragma unroll
        for (int c = 0; c < M; ++c) {
            const int idx = c * 64 + lane;
            if (idx < count) out[idx] = tile[idx];
        }
    }
    if (!ok) st |= sympa::ST_NOT_PD;
    if (!conv) st |= sympa::ST_NO_CONVERGENCE;
    if (!fin) st |= sympa::ST_NONFINITE;
    spd_vvd_report(a.status, st, live, lane);
}

// Backward, sixteen lanes per pair: spd_coop_bwd_kernel (spd_coop_bwd_kernel.hpp) with a cotangent row per pair.  One wave per block,
// `rounds` rounds of 4 pairs; group g handles pair 4 (rounds * block + t) + g in round t, lane r of the group owns row r of every
// matrix of that pair.  The eigenvalues d[0 .. M) are group-uniform after the QL: every lane ranks them (M^2 compares, stable: equal
// values get distinct ranks), loads gv[i, rank(k)] (one address per group) and forms the weights
//     gy[k] = gv[i, rank(k)] / (1 + d[k]),   gx[k] = -gv[i, rank(k)];
// x == y (every d[k] == 0) takes the zero subgradient.  Lane r < M keeps the value of rank r, so a group stores its row of v as M
// consecutive doubles.
template <int M>
__global__ __launch_bounds__(64, spd_vvd_coop_bwd_waves<M>()) void spd_vvd_coop_bwd_kernel(const SpdVvdArgs a, const int rounds) {
    using namespace spd_coop;
    __shared__ __attribute__((aligned(16))) double tbuf_all[4 * TBUF];
    const int lane = threadIdx.x;
    const int g = lane >> 4, r = lane & 15;
    double* const tbuf = tbuf_all + g * TBUF;
    constexpr int nn = M * M;
    int st = 0;
    for (int t = 0; t < rounds; ++t) {
        const int64_t first = ((int64_t)blockIdx.x * rounds + t) * 4;
        if (first >= a.b) break;                                     // wave-uniform
        const int64_t i = first + g;                                 // my group's pair in this round
        const bool live = i < a.b;
        const int64_t ii = live ? i : a.b - 1;
        int64_t r1 = ii, r2 = ii;
        bool bad = false;
        if (a.src != nullptr) {
            r1 = a.src[ii * a.src_stride];
            r2 = a.dst[ii * a.dst_stride];
            if (r1 < 0 || r1 >= a.num_rows || r2 < 0 || r2 >= a.num_rows) { bad = true; r1 = 0; r2 = 0; }
        }
        const double* px = a.x + r1 * nn;
        const double* py = a.y + r2 * nn;
        double x[M], y[M];
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int lo = r < j ? r : j, hi = r < j ? j : r;
            const int e = (hi < M) ? lo * M + hi : 0;            // upper triangle; a phantom lane reads element 0
            x[j] = px[e];
            y[j] = py[e];
        }
#pragma unroll
        for (int j = 0; j < M; ++j) y[j] -= x[j];                 // D = Y - X
        double rd[M], m[M];
        const bool pd = cholesky_rows(x, rd);                     // x <- rows of L
        solve_right_lt(y, x, rd);                                 // W = D L^-T
        transpose_rows(y, m, tbuf, r);
        solve_right_lt(m, x, rd);                                 // A = L^-1 D L^-T
        double d[M], e[M], vk[M], bk[M];
        tridiagonalize_keep(m, r, d, e, vk, bk);
        // (d, e) from lane 0: the redundant QL of the sixteen lanes must agree bit for bit (spd_coop_bwd_kernel)
#pragma unroll
        for (int j = 0; j < M; ++j) { d[j] = bcast<0>(d[j]); e[j] = bcast<0>(e[j]); }
        double zrow[M];
#pragma unroll
        for (int j = 0; j < M; ++j) zrow[j] = (r == j) ? 1.0 : 0.0;
        const bool conv = tridiag_ql_vectors_row(d, e, zrow);
        double zc[M], vrow[M];
        transpose_rows(zrow, zc, tbuf, r);                        // lane c holds column c of Z
        back_transform_columns(zc, vk, bk);                       // ... of V = Q Z
        transpose_rows(zc, vrow, tbuf, r);                        // lane i holds row i of V
        // the cotangent's spectral weights (group-uniform) and my component of the ascending v
        bool ok = pd, same = true, fin = true;
        const double* gvi = a.gv + ii * M;
        double gy[M], gx[M];
        double mine = 0.0;
#pragma unroll
        for (int k = 0; k < M; ++k) {
            ok = ok && (d[k] > -1.0);
            same = same && (d[k] == 0.0);
            const double lg = sympa::d_log1p_signed(d[k]);
            fin = fin && sympa::d_finite(lg);
            int rk = 0;
#pragma unroll
            for (int mm = 0; mm < M; ++mm) rk += (d[mm] < d[k] || (d[mm] == d[k] && mm < k)) ? 1 : 0;
            const double w = gvi[rk];                             // rk < M
            gy[k] = w * sympa::d_rcp(1.0 + d[k]);
            gx[k] = -w;
            mine = (rk == r) ? lg : mine;
        }
        if (!live || bad || same) {
#pragma unroll
            for (int k = 0; k < M; ++k) { gy[k] = 0.0; gx[k] = 0.0; }
        }
        double py_[M], px_[M];
        vdvt_rows(vrow, gy, py_);
        vdvt_rows(vrow, gx, px_);
        congruence_inv_t_rows(py_, x, rd, tbuf, r);
        congruence_inv_t_rows(px_, x, rd, tbuf, r);
        if (a.gtab != nullptr) {            // in-kernel scatter, consecutive lanes on consecutive doubles (spd_coop.hpp)
            scatter_plane<M>(px_, tbuf, a.gtab + r1 * nn, r, live && !bad);
            scatter_plane<M>(py_, tbuf, a.gtab + r2 * nn, r, live && !bad);
        } else if (live && r < M) {
            double* ox = a.gx + i * nn + r * M;
            double* oy = a.gy + i * nn + r * M;
#pragma unroll
            for (int j = 0; j < M; ++j) { ox[j] = px_[j]; oy[j] = py_[j]; }
        }
        if (live && r < M && a.vvd != nullptr) a.vvd[i * M + r] = bad ? __builtin_nan("") : mine;
        if (r == 0 && live) {
            if (bad) st |= sympa::ST_BAD_INDEX;
            if (!ok) st |= sympa::ST_NOT_PD;
            if (!conv) st |= sympa::ST_NO_CONVERGENCE;
            if (!fin) st |= sympa::ST_NONFINITE;
        }
    }
    spd_vvd_report(a.status, st, true, lane);
}

}  // namespace sympa_hip
