// Kernel templates of the exponential / logarithm maps and of the geodesic RiemannianSGD step (siegel_expmap_math.hpp), one
// row or pair per lane, dims 1..8, fully unrolled; instantiated per model by siegel_expmap_upper.hip and
// siegel_expmap_bounded.hip (two units: the n = 7, 8 bodies take the compile time), dispatched by siegel_expmap.hip.
// Loads, stores, the tail lanes and the status / projected words follow the table kernels (siegel_table_kernel.hpp).
// Blocks are one wave: nothing is shared between waves, and a table of a few thousand rows spreads over the CUs.
#pragma once
#include "siegel_common.hpp"
#include "siegel_expmap_math.hpp"

namespace sympa_hip {

constexpr int EXPMAP_BLOCK = 64;

__device__ __forceinline__ void expmap_report(int32_t* status, const bool live, const int st) {
    if (status == nullptr) return;
    const unsigned long long f = __ballot(live && st != 0);
    if (f != 0ull) {
        if (live && st != 0) atomicOr(&status[0], st);
        if ((threadIdx.x & 63) == 0) atomicAdd(&status[1], (int)__popcll(f));
    }
}

// OP 0: out = expmap(a, c) (c = the tangent vectors);  OP 1: out = logmap(a, c) (c = the second points)
template <int N, int MODEL, int OP>
__global__ __launch_bounds__(EXPMAP_BLOCK) void expmap_kernel(const double* __restrict__ a, const double* __restrict__ c,
                                                              double* __restrict__ out, int64_t b, int32_t* status) {
    const int64_t i = (int64_t)blockIdx.x * EXPMAP_BLOCK + threadIdx.x;
    const bool live = i < b;
    const int64_t ii = live ? i : b - 1;      // tail lanes recompute the last row (the eigenvalue loops ballot)
    constexpr int64_t ROW = 2 * N * N;
    sympa::CMat<N> x, y, r;
    sympa::load_full<N>(a + ii * ROW, x);
    sympa::load_full<N>(c + ii * ROW, y);
    int st = 0;
    if (OP == 0) sympa::expmap_row<N, MODEL>(x, y, r, st);
    else sympa::logmap_pair<N, MODEL>(x, y, r, st);
    if (live) sympa::store_full<N>(out + i * ROW, r);
    expmap_report(status, live, st);
}

template <int N, int MODEL>
__global__ __launch_bounds__(EXPMAP_BLOCK) void rsgd_exp_kernel(double* __restrict__ z, const double* __restrict__ grad, int64_t b,
                                                                double lr, double wd, double eps, int32_t* projected,
                                                                int32_t* status) {
    const int64_t i = (int64_t)blockIdx.x * EXPMAP_BLOCK + threadIdx.x;
    const bool live = i < b;
    const int64_t ii = live ? i : b - 1;
    constexpr int64_t ROW = 2 * N * N;
    sympa::CMat<N> x, g;
    sympa::load_full<N>(z + ii * ROW, x);
    sympa::load_full<N>(grad + ii * ROW, g);
    int st = 0;
    const bool moved = sympa::rsgd_exp_row<N, MODEL>(x, g, lr, wd, eps, st);
    if (live) sympa::store_full<N>(z + i * ROW, x);
    const unsigned long long m = __ballot(live && moved);
    if (projected != nullptr && m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(projected, (int)__popcll(m));
    expmap_report(status, live, st);
}

// op 0 / 1: expmap / logmap (a, c -> out);  op 2: the step (a = table in place, c = grad)
template <int N, int MODEL>
int launch_expmap_n(int op, double* a, const double* c, double* out, int64_t b, double lr, double wd, double eps,
                    int32_t* projected, int32_t* status, hipStream_t s) {
    const unsigned grid = (unsigned)((b + EXPMAP_BLOCK - 1) / EXPMAP_BLOCK);
    if (op == 0) hipLaunchKernelGGL((expmap_kernel<N, MODEL, 0>), dim3(grid), dim3(EXPMAP_BLOCK), 0, s, a, c, out, b, status);
    else if (op == 1) hipLaunchKernelGGL((expmap_kernel<N, MODEL, 1>), dim3(grid), dim3(EXPMAP_BLOCK), 0, s, a, c, out, b, status);
    else hipLaunchKernelGGL((rsgd_exp_kernel<N, MODEL>), dim3(grid), dim3(EXPMAP_BLOCK), 0, s, a, c, b, lr, wd, eps, projected, status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

template <int MODEL>
int launch_expmap_model(int op, int n, double* a, const double* c, double* out, int64_t b, double lr, double wd, double eps,
                        int32_t* projected, int32_t* status, hipStream_t s) {
#define SYMPA_EXPMAP_CASE(NN) case NN: return launch_expmap_n<NN, MODEL>(op, a, c, out, b, lr, wd, eps, projected, status, s);
    switch (n) {
        SYMPA_EXPMAP_CASE(1) SYMPA_EXPMAP_CASE(2) SYMPA_EXPMAP_CASE(3) SYMPA_EXPMAP_CASE(4)
        SYMPA_EXPMAP_CASE(5) SYMPA_EXPMAP_CASE(6) SYMPA_EXPMAP_CASE(7) SYMPA_EXPMAP_CASE(8)
        default: break;
    }
#undef SYMPA_EXPMAP_CASE
    return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "the exponential / logarithm maps: dims 1..8");
}

// siegel_expmap_upper.hip / siegel_expmap_bounded.hip
int launch_expmap_upper(int op, int n, double* a, const double* c, double* out, int64_t b, double lr, double wd, double eps,
                        int32_t* projected, int32_t* status, hipStream_t s);
int launch_expmap_bounded(int op, int n, double* a, const double* c, double* out, int64_t b, double lr, double wd, double eps,
                          int32_t* projected, int32_t* status, hipStream_t s);

}  // namespace sympa_hip
