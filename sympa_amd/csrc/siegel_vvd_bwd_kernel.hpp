// Backward of the vector-valued distance (C-ABI sympa_siegel_vvd_bwd / sympa_model_vvd_backward): one pair per lane, the kernel
// template shared by siegel_vvd_bwd.hip (dims 1..6, unrolled, register-resident), siegel_vvd_bwd_dual.hip (the compact dual, dims
// 1..6) and siegel_vvd_bwd_rolled.hip / siegel_vvd_bwd_rolled_dual.hip (dims 7..16: the same arithmetic with rolled loops over
// per-lane scratch).  The cotangent is a ROW per pair, gv = grad_v + i * n on the ascending v, instead of the scalar go of
// siegel_bwd_kernel.hpp, whose gather, scatter and row-store helpers this kernel reuses; there is no metric, no scale, no loss.
#pragma once
#include "siegel_bwd_kernel.hpp"

namespace sympa_hip {

struct VvdBwdArgs {
    DistArgs f;              // base1 / base2 / idx1 / idx2 / strides / num_rows / b / inv_eps / status (f.vvd: [b, n] or null)
    const double* gv;        // [b, n] dLoss / dv, ascending order
    double* g1;              // dense [b,2,n,n] or the grad table
    double* g2;
};

template <int N, int MODEL, bool SCATTER>
__device__ __forceinline__ void siegel_vvd_bwd_body(const VvdBwdArgs& a, const int64_t i, v2d* __restrict__ tile) {
    constexpr bool ROWS_TILE = BwdLds<N, SCATTER>::ROWS_TILE;
    const DistArgs& f = a.f;
    const bool live = i < f.b;
    const int64_t ii = live ? i : f.b - 1;       // idle tail lanes recompute the last pair (the wave ballots need them)

    int st = 0;
    int64_t r1 = ii, r2 = ii;
    if (f.idx1 != nullptr) {
        r1 = f.idx1[ii * f.idx1_stride];
        r2 = f.idx2[ii * f.idx2_stride];
        if (r1 < 0 || r1 >= f.num_rows || r2 < 0 || r2 >= f.num_rows) {
            st |= sympa::ST_BAD_INDEX;
            r1 = 0;
            r2 = 0;
        }
    }
    constexpr int64_t ROW = 2 * N * N;
    sympa::CMat<N> z1, z2;
    if constexpr (DmaTile<N>::ENABLED) {
        gather_pair_dma_low<N>(f.base1, (int)r1, f.base2, (int)r2, tile, z1, z2);
    } else if constexpr (Tile<N>::STAGED) {
        gather_pair_staged<N>(f.base1, (int)r1, f.base2, (int)r2, tile, z1, z2);
    } else {
        sympa::load_point<N>(f.base1 + r1 * ROW, z1);
        sympa::load_point<N>(f.base2 + r2 * ROW, z2);
    }
    const bool bad = (st & sympa::ST_BAD_INDEX) != 0;
    sympa::CMat<N> g1, g2;
    double* const vrow = (f.vvd != nullptr && live) ? f.vvd + i * N : nullptr;
    sympa::pair_backward_vvd<N, MODEL>(z1, z2, a.gv + ii * N, f.inv_eps, g1, g2, vrow, st);
    if (bad && vrow != nullptr) {
SYMPA_UNROLL
        for (int k = 0; k < N; ++k) vrow[k] = __builtin_nan("");
    }

    if constexpr (SCATTER) {
        double* dtile = reinterpret_cast<double*>(tile);
        if constexpr (N >= 7) {
            scatter_add_rows_outlined<N>(g1, (int)r1, a.g1, dtile, live && !bad);
            scatter_add_rows_outlined<N>(g2, (int)r2, a.g2, dtile, live && !bad);
        } else {
            scatter_add_rows<N>(g1, (int)r1, a.g1, dtile, live && !bad);
            scatter_add_rows<N>(g2, (int)r2, a.g2, dtile, live && !bad);
        }
    } else if constexpr (ROWS_TILE) {
        // per-pair rows (a pair with an out-of-range index contributes zeros, like the scatter form skips it)
        double* dtile = reinterpret_cast<double*>(tile);
        const int64_t wave_first = i - (threadIdx.x & 63);
        const int64_t left = f.b - wave_first;
        const int live_pairs = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
        store_rows_coalesced<N>(g1, a.g1 + wave_first * ROW, dtile, bad, live_pairs);
        store_rows_coalesced<N>(g2, a.g2 + wave_first * ROW, dtile, bad, live_pairs);
    } else if (live) {
SYMPA_UNROLL
        for (int r = 0; r < N; ++r)
SYMPA_UNROLL
            for (int c = 0; c < N; ++c) {
                a.g1[i * ROW + r * N + c] = bad ? 0.0 : g1.re[r][c];
                a.g1[i * ROW + N * N + r * N + c] = bad ? 0.0 : g1.im[r][c];
                a.g2[i * ROW + r * N + c] = bad ? 0.0 : g2.re[r][c];
                a.g2[i * ROW + N * N + r * N + c] = bad ? 0.0 : g2.im[r][c];
            }
    }
    if (f.status != nullptr) {
        const int flagged = (live && st != 0) ? 1 : 0;
        const unsigned long long m = __ballot(flagged);
        if (m != 0ull) {
            if (flagged) atomicOr(&f.status[0], st);
            if ((threadIdx.x & 63) == 0) atomicAdd(&f.status[1], (int)__popcll(m));
        }
    }
}

// The factors of the upper model stay in registers at n <= 4 (KeepFactors; the scalar backward parks them in the wave's tile).
// Upper n = 4 then needs 254 (rows) / 257 (scatter) registers: asked for two blocks per CU it fits 256 -- two waves per SIMD instead
// of one -- and two 67.6 KB tiles fit the CU's LDS.  Every other instantiation keeps what it needs.
template <int N, int MODEL>
constexpr int vvd_bwd_min_blocks() { return (N == 4 && MODEL == sympa::MODEL_UPPER) ? 2 : 1; }

template <int N, int MODEL, bool SCATTER>
__global__ __launch_bounds__(bwd_block<N>(), (vvd_bwd_min_blocks<N, MODEL>())) void siegel_vvd_bwd_kernel(const VvdBwdArgs a) {
    constexpr int BLOCK = bwd_block<N>();
    constexpr int WAVE_SLOTS = BwdLds<N, SCATTER>::WAVE_SLOTS;
    __shared__ v2d lds[(BLOCK / 64) * WAVE_SLOTS];
    siegel_vvd_bwd_body<N, MODEL, SCATTER>(a, (int64_t)blockIdx.x * BLOCK + threadIdx.x, lds + (threadIdx.x >> 6) * WAVE_SLOTS);
}

template <int N, int MODEL>
int launch_vvd_bwd_nm(const VvdBwdArgs& a, bool scatter, hipStream_t s) {
    constexpr int BLOCK = bwd_block<N>();
    const unsigned grid = (unsigned)((a.f.b + BLOCK - 1) / BLOCK);
    if (scatter) hipLaunchKernelGGL((siegel_vvd_bwd_kernel<N, MODEL, true>), dim3(grid), dim3(BLOCK), 0, s, a);
    else hipLaunchKernelGGL((siegel_vvd_bwd_kernel<N, MODEL, false>), dim3(grid), dim3(BLOCK), 0, s, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail((int)e, hipGetErrorString(e));
}

// siegel_vvd_bwd.hip: upper / bounded dims 1..6;  siegel_vvd_bwd_dual.hip: dual dims 1..6;  siegel_vvd_bwd_rolled*.hip: dims 7..16
int launch_vvd_bwd_dual(const VvdBwdArgs& a, int n, bool scatter, hipStream_t s);
int launch_vvd_bwd_rolled(const VvdBwdArgs& a, int n, int model, bool scatter, hipStream_t s);
int launch_vvd_bwd_rolled_dual(const VvdBwdArgs& a, int n, bool scatter, hipStream_t s);

}  // namespace sympa_hip
