// gfx950 kernels + C-ABI of the spd exponential map, logarithm, geodesic and geodesic RSGD step (spd_expmap_math.hpp, DESIGN.md
// section 28).  Sixteen lanes per row / pair for n >= 3 (spd_expmap_kernel.hpp, units spd_expmap_coop_{lo,hi}.hip); the
// one-row-per-lane kernels below (runtime n <= 16, per-lane scratch) serve n <= 2, SYMPA_FLAG_GENERIC and an instantiation the
// self-check demoted (SYMPA_FAMILY_SPD_TABLE).  PARITY UNPINNED with respect to geoopt (absent); pinned by 100-digit fixtures.
#include <cmath>

#include "siegel_common.hpp"
#include "spd_expmap_kernel.hpp"
#include "spd_expmap_math.hpp"

namespace {
using namespace sympa_hip;

__device__ __forceinline__ void lane_status(int32_t* status, const bool live, const int st) {
    if (status != nullptr) {
        const unsigned long long f = __ballot(live && st != 0);
        if (f != 0ull) {
            if (live && st != 0) atomicOr(&status[0], st);
            if (threadIdx.x == 0) atomicAdd(&status[1], (int)__popcll(f));
        }
    }
}

// tail lanes recompute the last pair and do not store
__global__ __launch_bounds__(64) void spd_map_kernel(const int kind, const double* x, const double* p2, const double t, const int64_t b,
                                                     const int n, double* out, int32_t* status) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = i < b;
    const int64_t ii = live ? i : b - 1;
    const int nn = n * n;
    sympa::SpdExpWork w;
    int st = 0;
    double row[sympa::SPD_MAX_N * sympa::SPD_MAX_N];
    sympa::spd_map_row(w, kind, x + ii * nn, p2 + ii * nn, t, n, row, st);
    if (live) for (int k = 0; k < nn; ++k) out[i * nn + k] = row[k];
    lane_status(status, live, st);
}

__global__ __launch_bounds__(64) void spd_rsgd_exp_kernel(double* x, const double* g, const int64_t b, const int n, const double lr,
                                                          const double wd, const double* clip, const double max_norm, int32_t* status) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = i < b;
    const int64_t ii = live ? i : b - 1;
    const int nn = n * n;
    sympa::SpdExpWork w;
    int st = 0;
    double row[sympa::SPD_MAX_N * sympa::SPD_MAX_N], xs[sympa::SPD_MAX_N * sympa::SPD_MAX_N];
    const double coef = (clip != nullptr) ? fmin(1.0, max_norm / (sqrt(clip[0]) + 1e-6)) : 1.0;
    for (int k = 0; k < nn; ++k) row[k] = x[ii * nn + k];
    sympa::spd_row_rsgd_exp(w, xs, row, g + ii * nn, n, lr, wd, coef, st);
    if (live) for (int k = 0; k < nn; ++k) x[i * nn + k] = row[k];
    lane_status(status, live, st);
}

int launch_spd_expmap(int op, double* x, const double* p2, double t, int64_t b, int n, double* out, double lr, double wd,
                      const double* clip, double max_norm, int32_t* status, int flags, void* stream) {
    if (b < 0) return fail(SYMPA_ERR_BAD_ARG, "negative row count");
    if (flags & ~SYMPA_FLAG_GENERIC) return fail(SYMPA_ERR_BAD_ARG, "spd maps: flags are 0 or SYMPA_FLAG_GENERIC");
    if (n < 1 || n > sympa::SPD_MAX_N) return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "spd: dims outside [1, 16]");
    if (b == 0) return 0;
    if (x == nullptr || p2 == nullptr || (op != SPD_EXPMAP_OP_STEP && out == nullptr)) return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n >= SPD_EXPMAP_COOP_MIN_N && !(flags & SYMPA_FLAG_GENERIC) && !instance_fallback(SYMPA_FAMILY_SPD_TABLE, 0, n)) {
        if (n >= 12) launch_spd_coop_expmap_hi(op, n, x, p2, t, b, out, lr, wd, clip, max_norm, status, s);
        else launch_spd_coop_expmap_lo(op, n, x, p2, t, b, out, lr, wd, clip, max_norm, status, s);
    } else if (op == SPD_EXPMAP_OP_STEP) {
        hipLaunchKernelGGL(spd_rsgd_exp_kernel, dim3((unsigned)((b + 63) / 64)), dim3(64), 0, s, x, p2, b, n, lr, wd, clip, max_norm, status);
    } else {
        hipLaunchKernelGGL(spd_map_kernel, dim3((unsigned)((b + 63) / 64)), dim3(64), 0, s, op, x, p2, t, b, n, out, status);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

int sympa_spd_expmap(const double* x, const double* u, int64_t b, int n, double* out, int32_t* status, int flags, void* stream) {
    return launch_spd_expmap(sympa::SPD_MAP_EXP, const_cast<double*>(x), u, 0.0, b, n, out, 0.0, 0.0, nullptr, 0.0, status, flags, stream);
}

int sympa_spd_logmap(const double* x, const double* y, int64_t b, int n, double* out, int32_t* status, int flags, void* stream) {
    return launch_spd_expmap(sympa::SPD_MAP_LOG, const_cast<double*>(x), y, 0.0, b, n, out, 0.0, 0.0, nullptr, 0.0, status, flags, stream);
}

int sympa_spd_geodesic(const double* x, const double* y, double t, int64_t b, int n, double* out, int32_t* status, int flags,
                       void* stream) {
    if (!std::isfinite(t)) return fail(SYMPA_ERR_BAD_ARG, "spd geodesic: t must be finite");
    return launch_spd_expmap(sympa::SPD_MAP_GEODESIC, const_cast<double*>(x), y, t, b, n, out, 0.0, 0.0, nullptr, 0.0, status, flags, stream);
}

int sympa_spd_rsgd_step_exp(double* table, const double* grad, int64_t num_rows, int n, double lr, double weight_decay,
                            const double* total_sqnorm, double max_norm, int32_t* status, int flags, void* stream) {
    if (total_sqnorm != nullptr && !(max_norm > 0.0)) return fail(SYMPA_ERR_BAD_ARG, "max_norm must be > 0");
    return launch_spd_expmap(SPD_EXPMAP_OP_STEP, table, grad, 0.0, num_rows, n, nullptr, lr, weight_decay, total_sqnorm, max_norm, status,
                             flags, stream);
}

}  // extern "C"
