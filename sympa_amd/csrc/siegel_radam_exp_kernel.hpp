// Kernel template of the geodesic RiemannianAdam step (siegel_radam_exp_math.hpp), one row per lane, dims 1..8, fully unrolled;
// instantiated per model by siegel_radam_exp_upper.hip and siegel_radam_exp_bounded.hip, dispatched by siegel_radam_exp.hip.
// Loads, stores, the tail lanes and the status / projected words follow the exponential map's kernels
// (siegel_expmap_kernel.hpp), whose expmap_report is used as it is.  The table and both moments are updated in place: every
// output row is in registers before anything is stored.  Blocks are one wave: nothing is shared between waves.
#pragma once
#include "siegel_expmap_kernel.hpp"
#include "siegel_radam_exp_math.hpp"

namespace sympa_hip {

// pows: device words {b1^t, b2^t}, already advanced to this step (as sympa_radam_step reads them: a captured launch carries no
// step count).  clip: device word with the squared total gradient norm, or null (no clip).
template <int N, int MODEL>
__global__ __launch_bounds__(EXPMAP_BLOCK) void radam_exp_kernel(double* z, const double* grad, double* m, double* v, int64_t b,
                                                                 double lr, double b1, double b2, double eps_adam, double wd,
                                                                 const double* pows, double eps, const double* clip,
                                                                 double max_norm, int32_t* projected, int32_t* status) {
    const int64_t i = (int64_t)blockIdx.x * EXPMAP_BLOCK + threadIdx.x;
    const bool live = i < b;
    const int64_t ii = live ? i : b - 1;      // tail lanes recompute the last row (the eigenvalue loops ballot)
    constexpr int64_t ROW = 2 * N * N;
    sympa::CMat<N> x, g, mm;
    sympa::load_full<N>(z + ii * ROW, x);
    sympa::load_full<N>(grad + ii * ROW, g);
    sympa::load_full<N>(m + ii * ROW, mm);
    const double coef = clip != nullptr ? fmin(1.0, max_norm / (sqrt(clip[0]) + 1e-6)) : 1.0;
    int st = 0;
    double vn;
    const bool moved = sympa::radam_exp_row<N, MODEL>(x, g, mm, v[ii], vn, lr, b1, b2, eps_adam, wd, pows[0], pows[1], coef, eps, st);
    if (live) {
        sympa::store_full<N>(m + i * ROW, g);
        v[i] = vn;
        sympa::store_full<N>(z + i * ROW, x);
    }
    const unsigned long long mv = __ballot(live && moved);
    if (projected != nullptr && mv != 0ull && (threadIdx.x & 63) == 0) atomicAdd(projected, (int)__popcll(mv));
    expmap_report(status, live, st);
}

template <int MODEL>
int launch_radam_exp_model(int n, double* z, const double* grad, double* m, double* v, int64_t b, double lr, double b1, double b2,
                           double eps_adam, double wd, const double* pows, double eps, const double* clip, double max_norm,
                           int32_t* projected, int32_t* status, hipStream_t s) {
    const unsigned grid = (unsigned)((b + EXPMAP_BLOCK - 1) / EXPMAP_BLOCK);
#define SYMPA_RADAM_EXP_CASE(NN)                                                                                                  \
    case NN:                                                                                                                      \
        hipLaunchKernelGGL((radam_exp_kernel<NN, MODEL>), dim3(grid), dim3(EXPMAP_BLOCK), 0, s, z, grad, m, v, b, lr, b1, b2,     \
                           eps_adam, wd, pows, eps, clip, max_norm, projected, status);                                           \
        break;
    switch (n) {
        SYMPA_RADAM_EXP_CASE(1) SYMPA_RADAM_EXP_CASE(2) SYMPA_RADAM_EXP_CASE(3) SYMPA_RADAM_EXP_CASE(4)
        SYMPA_RADAM_EXP_CASE(5) SYMPA_RADAM_EXP_CASE(6) SYMPA_RADAM_EXP_CASE(7) SYMPA_RADAM_EXP_CASE(8)
        default: return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "the geodesic RiemannianAdam step: dims 1..8");
    }
#undef SYMPA_RADAM_EXP_CASE
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

// siegel_radam_exp_upper.hip / siegel_radam_exp_bounded.hip
int launch_radam_exp_upper(int n, double* z, const double* grad, double* m, double* v, int64_t b, double lr, double b1, double b2,
                           double eps_adam, double wd, const double* pows, double eps, const double* clip, double max_norm,
                           int32_t* projected, int32_t* status, hipStream_t s);
int launch_radam_exp_bounded(int n, double* z, const double* grad, double* m, double* v, int64_t b, double lr, double b1, double b2,
                             double eps_adam, double wd, const double* pows, double eps, const double* clip, double max_norm,
                             int32_t* projected, int32_t* status, hipStream_t s);

}  // namespace sympa_hip
