// The differentiable vector-valued distance: C-ABI sympa_model_vvd_forward / sympa_siegel_vvd_bwd / sympa_model_vvd_backward and the
// one-pair-per-lane backward kernels of dims 1..6, upper and bounded model (siegel_vvd_bwd_kernel.hpp; the compact dual and dims
// 7..16 are units of their own).  The forward is the existing forward kernel with DistArgs.vvd set (siegel_dist.hip).
#include "siegel_vvd_bwd_kernel.hpp"

namespace sympa_hip {

template <int N>
int launch_vvd_bwd_n(const VvdBwdArgs& a, int model, bool scatter, hipStream_t s) {
    return model == SYMPA_MODEL_UPPER ? launch_vvd_bwd_nm<N, sympa::MODEL_UPPER>(a, scatter, s)
                                      : launch_vvd_bwd_nm<N, sympa::MODEL_BOUNDED>(a, scatter, s);
}

}  // namespace sympa_hip

namespace {
using namespace sympa_hip;

int check_common(int64_t b, int n, int model, double eps, int flags) {
    if (b < 0) return fail(SYMPA_ERR_BAD_ARG, "negative batch size");
    if (flags != 0) return fail(SYMPA_ERR_BAD_ARG, "flags is reserved and must be 0");
    if (model != SYMPA_MODEL_UPPER && model != SYMPA_MODEL_BOUNDED && model != SYMPA_MODEL_DUAL) return fail(SYMPA_ERR_BAD_ARG, "unknown model");
    if (!(eps > 0.0)) return fail(SYMPA_ERR_BAD_ARG, "eps must be > 0");
    if (n < 1 || n > SYMPA_MAX_DIMS_BACKWARD)
        return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "vector-valued distance: dims outside [1, SYMPA_MAX_DIMS_BACKWARD]");
    return 0;
}

int launch_vvd_bwd(const VvdBwdArgs& a, int n, int model, bool scatter, void* stream) {
    const int rc = validate(a.f, model, n);
    if (rc != 0) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n >= 7) return launch_vvd_bwd_rolled(a, n, model, scatter, s);
    if (model == SYMPA_MODEL_DUAL) return launch_vvd_bwd_dual(a, n, scatter, s);
    switch (n) {
        case 1: return launch_vvd_bwd_n<1>(a, model, scatter, s);
        case 2: return launch_vvd_bwd_n<2>(a, model, scatter, s);
        case 3: return launch_vvd_bwd_n<3>(a, model, scatter, s);
        case 4: return launch_vvd_bwd_n<4>(a, model, scatter, s);
        case 5: return launch_vvd_bwd_n<5>(a, model, scatter, s);
        default: return launch_vvd_bwd_n<6>(a, model, scatter, s);
    }
}

// The forward kernel evaluates a pair with an out-of-range index on row 0 and marks only its scalar value; its row of v becomes NaN here.
__global__ __launch_bounds__(256) void vvd_bad_index_rows_kernel(const int64_t* __restrict__ src, const int64_t src_stride,
                                                                  const int64_t* __restrict__ dst, const int64_t dst_stride,
                                                                  const int64_t b, const int64_t num_rows, const int n,
                                                                  double* __restrict__ vvd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= b) return;
    const int64_t r1 = src[i * src_stride], r2 = dst[i * dst_stride];
    if (r1 < 0 || r1 >= num_rows || r2 < 0 || r2 >= num_rows)
        for (int k = 0; k < n; ++k) vvd[i * n + k] = __builtin_nan("");
}

}  // namespace

extern "C" {

int sympa_model_vvd_forward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                            const int64_t* dst, int64_t dst_stride, int64_t b, int model, double eps, double* vvd_out,
                            int32_t* status, int flags, void* stream) {
    const int rc = check_common(b, n, model, eps, flags);
    if (rc != 0) return rc;
    if (b == 0) return 0;
    if (table == nullptr || src == nullptr || dst == nullptr || vvd_out == nullptr) return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    if (num_rows <= 0) return fail(SYMPA_ERR_BAD_ARG, "empty table");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // the forward kernels always store the scalar value: it goes to a stream-ordered scratch nobody reads
    double* sink = nullptr;
    hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&sink), (size_t)b * sizeof(double), s);
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    DistArgs a;
    std::memset(&a, 0, sizeof(a));
    a.base1 = table;
    a.base2 = table;
    a.idx1 = src;
    a.idx2 = dst;
    a.idx1_stride = src_stride;
    a.idx2_stride = dst_stride;
    a.num_rows = num_rows;
    a.b = b;
    a.inv_scale_coef = 1.0;
    a.inv_eps = 1.0 / eps;
    a.out = sink;
    a.vvd = vvd_out;
    a.status = status;
    a.metric = SYMPA_METRIC_RIEM;
    int lrc = launch_dist(a, n, model, stream);
    if (lrc == 0) {
        hipLaunchKernelGGL(vvd_bad_index_rows_kernel, dim3((unsigned)((b + 255) / 256)), dim3(256), 0, s, src, src_stride, dst,
                           dst_stride, b, num_rows, n, vvd_out);
        e = hipGetLastError();
        if (e != hipSuccess) lrc = fail((int)e, hipGetErrorString(e));
    }
    e = hipFreeAsync(sink, s);
    if (lrc == 0 && e != hipSuccess) lrc = fail((int)e, hipGetErrorString(e));
    return lrc;
}

int sympa_siegel_vvd_bwd(const double* z1, const double* z2, const double* grad_v, int64_t b, int n, int model, double eps,
                         double* grad_z1, double* grad_z2, double* vvd_out, int32_t* status, int flags, void* stream) {
    const int rc = check_common(b, n, model, eps, flags);
    if (rc != 0) return rc;
    if (b == 0) return 0;
    if (z1 == nullptr || z2 == nullptr || grad_v == nullptr || grad_z1 == nullptr || grad_z2 == nullptr)
        return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    VvdBwdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.f.base1 = z1;
    a.f.base2 = z2;
    a.f.b = b;
    a.f.num_rows = b;
    a.f.inv_scale_coef = 1.0;
    a.f.inv_eps = 1.0 / eps;
    a.f.vvd = vvd_out;
    a.f.status = status;
    a.f.metric = SYMPA_METRIC_RIEM;
    a.gv = grad_v;
    a.g1 = grad_z1;
    a.g2 = grad_z2;
    return launch_vvd_bwd(a, n, model, false, stream);
}

int sympa_model_vvd_backward(const double* table, int64_t num_rows, int n, const int64_t* src, int64_t src_stride,
                             const int64_t* dst, int64_t dst_stride, int64_t b, int model, double eps, const double* grad_v,
                             double* grad_table, double* vvd_out, int32_t* status, int flags, void* stream) {
    const int rc = check_common(b, n, model, eps, flags);
    if (rc != 0) return rc;
    if (b == 0) return 0;
    if (table == nullptr || src == nullptr || dst == nullptr || grad_v == nullptr || grad_table == nullptr)
        return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    if (num_rows <= 0) return fail(SYMPA_ERR_BAD_ARG, "empty table");
    VvdBwdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.f.base1 = table;
    a.f.base2 = table;
    a.f.idx1 = src;
    a.f.idx2 = dst;
    a.f.idx1_stride = src_stride;
    a.f.idx2_stride = dst_stride;
    a.f.num_rows = num_rows;
    a.f.b = b;
    a.f.inv_scale_coef = 1.0;
    a.f.inv_eps = 1.0 / eps;
    a.f.vvd = vvd_out;
    a.f.status = status;
    a.f.metric = SYMPA_METRIC_RIEM;
    a.gv = grad_v;
    a.g1 = grad_table;
    a.g2 = grad_table;
    return launch_vvd_bwd(a, n, model, true, stream);
}

}  // extern "C"
