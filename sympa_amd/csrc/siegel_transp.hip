// C-ABI of the parallel transport along geodesics of the upper and bounded models (include/sympa_hip.h; arithmetic:
// siegel_transp_math.hpp; kernels: siegel_transp_kernel.hpp, instantiated per model in siegel_transp_upper.hip /
// siegel_transp_bounded.hip).  Arguments are validated before anything touches the device.
#include "siegel_transp_kernel.hpp"

namespace {
using namespace sympa_hip;

// op 0 / 1: along the tangent c, without / with out_y;  op 2: to the point c
int dispatch_transp(int op, int n, int model, const double* a, const double* c, const double* v, double* out_y, double* out_v,
                    int64_t b, int32_t* status, void* stream) {
    if (b < 0) return fail(SYMPA_ERR_BAD_ARG, "negative row count");
    if (model == SYMPA_MODEL_DUAL)
        return fail(SYMPA_ERR_BAD_ARG, "the compact dual model has no inner product (the reference's inner raises "
                                       "NotImplementedError, compact_dual.py:96): no parallel transport");
    if (model != SYMPA_MODEL_UPPER && model != SYMPA_MODEL_BOUNDED) return fail(SYMPA_ERR_BAD_ARG, "unknown model");
    if (n < 1 || n > 8) return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "the parallel transport: dims 1..8");
    if (b == 0) return 0;
    if (a == nullptr || c == nullptr || v == nullptr || out_v == nullptr) return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    if (b > (int64_t)0x7fffffff * EXPMAP_BLOCK) return fail(SYMPA_ERR_BAD_ARG, "too many rows for one launch");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (model == SYMPA_MODEL_UPPER) return launch_transp_upper(op, n, a, c, v, out_y, out_v, b, status, s);
    return launch_transp_bounded(op, n, a, c, v, out_y, out_v, b, status, s);
}

}  // namespace

extern "C" {

int sympa_transp_exp(const double* z, const double* u, const double* v, int64_t b, int n, int model, double* out_y, double* out_v,
                     int32_t* status, void* stream) {
    return dispatch_transp(out_y != nullptr ? 1 : 0, n, model, z, u, v, out_y, out_v, b, status, stream);
}

int sympa_transp(const double* z1, const double* z2, const double* v, int64_t b, int n, int model, double* out_v, int32_t* status,
                 void* stream) {
    return dispatch_transp(2, n, model, z1, z2, v, nullptr, out_v, b, status, stream);
}

}  // extern "C"
