// The SPD model's differentiable vector-valued distance: C-ABI sympa_spd_vvd_fwd / sympa_spd_model_vvd_forward /
// sympa_spd_vvd_bwd / sympa_spd_model_vvd_backward, the dispatch, and the one-pair-per-lane kernels (runtime n <= 16, per-lane scratch:
// the forward at n <= 5, the backward at n <= 2, and SYMPA_FLAG_GENERIC at every n).  The sixteen-lanes-per-pair kernels
// (spd_vvd_kernel.hpp) are units of their own.
#include "spd_vvd_kernel.hpp"

namespace sympa_hip {
namespace {

__device__ __forceinline__ bool spd_vvd_rows_of(const SpdVvdArgs& a, const int64_t ii, int64_t& r1, int64_t& r2) {
    r1 = ii; r2 = ii;
    if (a.src != nullptr) {
        r1 = a.src[ii * a.src_stride];
        r2 = a.dst[ii * a.dst_stride];
        if (r1 < 0 || r1 >= a.num_rows || r2 < 0 || r2 >= a.num_rows) { r1 = 0; r2 = 0; return true; }
    }
    return false;
}

__global__ __launch_bounds__(64) void spd_vvd_fwd_kernel(const SpdVvdArgs a, const int n) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = i < a.b;
    const int64_t ii = live ? i : a.b - 1;
    int64_t r1, r2;
    const bool bad = spd_vvd_rows_of(a, ii, r1, r2);
    int st = bad ? sympa::ST_BAD_INDEX : 0;
    const int nn = n * n;
    sympa::SpdWork w;
    double v[sympa::SPD_MAX_N];
    sympa::spd_pair_vvd(w, a.x + r1 * nn, a.y + r2 * nn, n, v, st);
    if (live)
        for (int k = 0; k < n; ++k) a.vvd[i * n + k] = bad ? __builtin_nan("") : v[k];
    spd_vvd_report(a.status, st, live, threadIdx.x);
}

__global__ __launch_bounds__(64) void spd_vvd_bwd_kernel(const SpdVvdArgs a, const int n) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = i < a.b;
    const int64_t ii = live ? i : a.b - 1;      // tail lanes recompute the last pair and do not store
    int64_t r1, r2;
    const bool bad = spd_vvd_rows_of(a, ii, r1, r2);
    int st = bad ? sympa::ST_BAD_INDEX : 0;
    const int nn = n * n;
    sympa::SpdBwdWork w;
    double lgx[sympa::SPD_MAX_N * sympa::SPD_MAX_N], lgy[sympa::SPD_MAX_N * sympa::SPD_MAX_N], v[sympa::SPD_MAX_N];
    sympa::spd_pair_backward_vvd(w, a.x + r1 * nn, a.y + r2 * nn, n, a.gv + ii * n, lgx, lgy, v, st);
    if (live) {
        if (a.gtab != nullptr) {
            if (!bad) {
                double* tx = a.gtab + r1 * nn;
                double* ty = a.gtab + r2 * nn;
                for (int k = 0; k < nn; ++k) {
                    if (lgx[k] != 0.0) atomicAdd(tx + k, lgx[k]);
                    if (lgy[k] != 0.0) atomicAdd(ty + k, lgy[k]);
                }
            }
        } else {
            double* gx = a.gx + i * nn;
            double* gy = a.gy + i * nn;
            for (int k = 0; k < nn; ++k) { gx[k] = bad ? 0.0 : lgx[k]; gy[k] = bad ? 0.0 : lgy[k]; }
        }
        if (a.vvd != nullptr)
            for (int k = 0; k < n; ++k) a.vvd[i * n + k] = bad ? __builtin_nan("") : v[k];
    }
    spd_vvd_report(a.status, st, live, threadIdx.x);
}

}  // namespace

void launch_spd_vvd_fwd_one_lane(const SpdVvdArgs& a, int n, hipStream_t s) {
    hipLaunchKernelGGL(spd_vvd_fwd_kernel, dim3((unsigned)((a.b + 63) / 64)), dim3(64), 0, s, a, n);
}

void launch_spd_vvd_bwd_one_lane(const SpdVvdArgs& a, int n, hipStream_t s) {
    hipLaunchKernelGGL(spd_vvd_bwd_kernel, dim3((unsigned)((a.b + 63) / 64)), dim3(64), 0, s, a, n);
}

}  // namespace sympa_hip

namespace {
using namespace sympa_hip;

int check_common(int64_t b, int n, int flags) {
    if (b < 0) return fail(SYMPA_ERR_BAD_ARG, "negative batch size");
    if ((flags & ~SYMPA_FLAG_GENERIC) != 0) return fail(SYMPA_ERR_BAD_ARG, "spd vector-valued distance: flags is 0 or SYMPA_FLAG_GENERIC");
    if (n < 1 || n > sympa::SPD_MAX_N) return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "spd: dims outside [1, 16]");
    return 0;
}

int last_error() {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

int launch_fwd(const SpdVvdArgs& a, int n, int flags, void* stream) {
    if (a.num_rows > (int64_t)0x7fffffff) return fail(SYMPA_ERR_BAD_ARG, "more than 2^31-1 table rows");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n < SPD_VVD_COOP_FWD_MIN_N || (flags & SYMPA_FLAG_GENERIC)) launch_spd_vvd_fwd_one_lane(a, n, s);
    else if (n <= 11) launch_spd_vvd_fwd_coop_lo(a, n, s);
    else launch_spd_vvd_fwd_coop_hi(a, n, s);
    return last_error();
}

int launch_bwd(const SpdVvdArgs& a, int n, int flags, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n < SPD_VVD_COOP_BWD_MIN_N || (flags & SYMPA_FLAG_GENERIC)) launch_spd_vvd_bwd_one_lane(a, n, s);
    else if (n <= 9) launch_spd_vvd_bwd_coop_lo(a, n, s);
    else if (n <= 13) launch_spd_vvd_bwd_coop_mid(a, n, s);
    else launch_spd_vvd_bwd_coop_hi(a, n, s);
    return last_error();
}

}  // namespace

extern "C" {

int sympa_spd_vvd_fwd(const double* x, const double* y, int64_t b, int n, double* vvd_out, int32_t* status, int flags, void* stream) {
    const int rc = check_common(b, n, flags);
    if (rc != 0) return rc;
    if (b == 0) return 0;
    if (x == nullptr || y == nullptr || vvd_out == nullptr) return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    SpdVvdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = x; a.y = y; a.b = b; a.num_rows = b; a.vvd = vvd_out; a.status = status;
    return launch_fwd(a, n, flags, stream);
}

int sympa_spd_model_vvd_forward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                                const int64_t* dst, int64_t dst_stride, int64_t b, double* vvd_out, int32_t* status, int flags,
                                void* stream) {
    const int rc = check_common(b, n, flags);
    if (rc != 0) return rc;
    if (b == 0) return 0;
    if (table == nullptr || src == nullptr || dst == nullptr || vvd_out == nullptr) return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    if (num_rows <= 0) return fail(SYMPA_ERR_BAD_ARG, "empty table");
    SpdVvdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = table; a.y = table; a.src = src; a.dst = dst; a.src_stride = src_stride; a.dst_stride = dst_stride;
    a.num_rows = num_rows; a.b = b; a.vvd = vvd_out; a.status = status;
    return launch_fwd(a, n, flags, stream);
}

int sympa_spd_vvd_bwd(const double* x, const double* y, const double* grad_v, int64_t b, int n, double* grad_x, double* grad_y,
                      double* vvd_out, int32_t* status, int flags, void* stream) {
    const int rc = check_common(b, n, flags);
    if (rc != 0) return rc;
    if (b == 0) return 0;
    if (x == nullptr || y == nullptr || grad_v == nullptr || grad_x == nullptr || grad_y == nullptr)
        return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    SpdVvdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = x; a.y = y; a.b = b; a.num_rows = b; a.gv = grad_v; a.gx = grad_x; a.gy = grad_y; a.vvd = vvd_out; a.status = status;
    return launch_bwd(a, n, flags, stream);
}

int sympa_spd_model_vvd_backward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                                 const int64_t* dst, int64_t dst_stride, int64_t b, const double* grad_v, double* grad_table,
                                 double* vvd_out, int32_t* status, int flags, void* stream) {
    const int rc = check_common(b, n, flags);
    if (rc != 0) return rc;
    if (b == 0) return 0;
    if (table == nullptr || src == nullptr || dst == nullptr || grad_v == nullptr || grad_table == nullptr)
        return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    if (num_rows <= 0) return fail(SYMPA_ERR_BAD_ARG, "empty table");
    SpdVvdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = table; a.y = table; a.src = src; a.dst = dst; a.src_stride = src_stride; a.dst_stride = dst_stride;
    a.num_rows = num_rows; a.b = b; a.gv = grad_v; a.gtab = grad_table; a.vvd = vvd_out; a.status = status;
    return launch_bwd(a, n, flags, stream);
}

}  // extern "C"
