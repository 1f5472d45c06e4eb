// C-ABI of the exponential / logarithm maps of the upper and bounded models and of the RiemannianSGD step along the geodesic
// (include/sympa_hip.h; arithmetic: siegel_expmap_math.hpp; kernels: siegel_expmap_kernel.hpp, instantiated per model in
// siegel_expmap_upper.hip / siegel_expmap_bounded.hip).  Arguments are validated before anything touches the device.
#include "siegel_expmap_kernel.hpp"

namespace {
using namespace sympa_hip;

int dispatch_expmap(int op, int n, int model, double* a, const double* c, double* out, int64_t b, double lr, double wd, double eps,
                    int32_t* projected, int32_t* status, void* stream) {
    if (b < 0) return fail(SYMPA_ERR_BAD_ARG, "negative row count");
    if (model == SYMPA_MODEL_DUAL)
        return fail(SYMPA_ERR_BAD_ARG, "the compact dual model has no inner product (the reference's inner raises "
                                       "NotImplementedError, compact_dual.py:96): no exponential / logarithm map");
    if (model != SYMPA_MODEL_UPPER && model != SYMPA_MODEL_BOUNDED) return fail(SYMPA_ERR_BAD_ARG, "unknown model");
    if (n < 1 || n > 8) return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "the exponential / logarithm maps: dims 1..8");
    if (b == 0) return 0;
    if (a == nullptr || c == nullptr || (op != 2 && out == nullptr)) return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    if (b > (int64_t)0x7fffffff * EXPMAP_BLOCK) return fail(SYMPA_ERR_BAD_ARG, "too many rows for one launch");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (model == SYMPA_MODEL_UPPER) return launch_expmap_upper(op, n, a, c, out, b, lr, wd, eps, projected, status, s);
    return launch_expmap_bounded(op, n, a, c, out, b, lr, wd, eps, projected, status, s);
}

}  // namespace

extern "C" {

int sympa_expmap(const double* z, const double* u, int64_t b, int n, int model, double* out, int32_t* status, void* stream) {
    return dispatch_expmap(0, n, model, const_cast<double*>(z), u, out, b, 0.0, 0.0, 0.0, nullptr, status, stream);
}

int sympa_logmap(const double* z1, const double* z2, int64_t b, int n, int model, double* out, int32_t* status, void* stream) {
    return dispatch_expmap(1, n, model, const_cast<double*>(z1), z2, out, b, 0.0, 0.0, 0.0, nullptr, status, stream);
}

int sympa_rsgd_step_exp(double* table, const double* grad, int64_t num_rows, int n, int model, double lr, double weight_decay,
                        double eps, int32_t* projected_count, int32_t* status, void* stream) {
    if (!(eps > 0.0)) return fail(SYMPA_ERR_BAD_ARG, "eps must be > 0");
    return dispatch_expmap(2, n, model, table, grad, nullptr, num_rows, lr, weight_decay, eps, projected_count, status, stream);
}

}  // extern "C"
