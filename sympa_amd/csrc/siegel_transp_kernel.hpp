// Kernel templates of the parallel transport along geodesics (siegel_transp_math.hpp), one row per lane, dims 1..8, fully
// unrolled; instantiated per model by siegel_transp_upper.hip and siegel_transp_bounded.hip, dispatched by siegel_transp.hip.
// Loads, stores, the tail lanes and the status words follow the exponential map's kernels (siegel_expmap_kernel.hpp), whose
// expmap_report is used as it is.  Every row is in registers before anything is stored: out_v may alias v, out_y may alias z.
// Blocks are one wave: nothing is shared between waves.
#pragma once
#include "siegel_expmap_kernel.hpp"
#include "siegel_transp_math.hpp"

namespace sympa_hip {

// OP 0: out_v = v transported from a along the tangent c;  OP 1: the same and out_y = expmap(a, c);
// OP 2: out_v = v transported from a to the point c.  No __restrict__: the outputs may alias the inputs.
template <int N, int MODEL, int OP>
__global__ __launch_bounds__(EXPMAP_BLOCK) void transp_kernel(const double* a, const double* c, const double* v, double* out_y,
                                                              double* out_v, int64_t b, int32_t* status) {
    const int64_t i = (int64_t)blockIdx.x * EXPMAP_BLOCK + threadIdx.x;
    const bool live = i < b;
    const int64_t ii = live ? i : b - 1;      // tail lanes recompute the last row (the eigenvalue loops ballot)
    constexpr int64_t ROW = 2 * N * N;
    sympa::CMat<N> x, y, w, rv;
    sympa::load_full<N>(a + ii * ROW, x);
    sympa::load_full<N>(c + ii * ROW, y);
    sympa::load_full<N>(v + ii * ROW, w);
    int st = 0;
    if constexpr (OP == 0) {
        sympa::transp_exp_row<N, MODEL>(x, y, w, rv, st);
    } else if constexpr (OP == 1) {
        sympa::CMat<N> ry;
        sympa::expmap_transp_row<N, MODEL>(x, y, w, ry, rv, st);
        if (live) sympa::store_full<N>(out_y + i * ROW, ry);
    } else {
        sympa::transp_pair<N, MODEL>(x, y, w, rv, st);
    }
    if (live) sympa::store_full<N>(out_v + i * ROW, rv);
    expmap_report(status, live, st);
}

template <int N, int MODEL>
int launch_transp_n(int op, const double* a, const double* c, const double* v, double* out_y, double* out_v, int64_t b,
                    int32_t* status, hipStream_t s) {
    const unsigned grid = (unsigned)((b + EXPMAP_BLOCK - 1) / EXPMAP_BLOCK);
    if (op == 0) hipLaunchKernelGGL((transp_kernel<N, MODEL, 0>), dim3(grid), dim3(EXPMAP_BLOCK), 0, s, a, c, v, out_y, out_v, b, status);
    else if (op == 1) hipLaunchKernelGGL((transp_kernel<N, MODEL, 1>), dim3(grid), dim3(EXPMAP_BLOCK), 0, s, a, c, v, out_y, out_v, b, status);
    else hipLaunchKernelGGL((transp_kernel<N, MODEL, 2>), dim3(grid), dim3(EXPMAP_BLOCK), 0, s, a, c, v, out_y, out_v, b, status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

template <int MODEL>
int launch_transp_model(int op, int n, const double* a, const double* c, const double* v, double* out_y, double* out_v, int64_t b,
                        int32_t* status, hipStream_t s) {
#define SYMPA_TRANSP_CASE(NN) case NN: return launch_transp_n<NN, MODEL>(op, a, c, v, out_y, out_v, b, status, s);
    switch (n) {
        SYMPA_TRANSP_CASE(1) SYMPA_TRANSP_CASE(2) SYMPA_TRANSP_CASE(3) SYMPA_TRANSP_CASE(4)
        SYMPA_TRANSP_CASE(5) SYMPA_TRANSP_CASE(6) SYMPA_TRANSP_CASE(7) SYMPA_TRANSP_CASE(8)
        default: break;
    }
#undef SYMPA_TRANSP_CASE
    return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "the parallel transport: dims 1..8");
}

// siegel_transp_upper.hip / siegel_transp_bounded.hip
int launch_transp_upper(int op, int n, const double* a, const double* c, const double* v, double* out_y, double* out_v, int64_t b,
                        int32_t* status, hipStream_t s);
int launch_transp_bounded(int op, int n, const double* a, const double* c, const double* v, double* out_y, double* out_v, int64_t b,
                          int32_t* status, hipStream_t s);

}  // namespace sympa_hip
