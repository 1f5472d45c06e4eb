// C-ABI of the geodesic RiemannianAdam step of the upper and bounded models (include/sympa_hip.h; arithmetic:
// siegel_radam_exp_math.hpp; kernels: siegel_radam_exp_kernel.hpp, instantiated per model in siegel_radam_exp_upper.hip /
// siegel_radam_exp_bounded.hip).  Arguments are validated before anything touches the device.
#include "siegel_radam_exp_kernel.hpp"

extern "C" {

int sympa_radam_step_exp(double* table, const double* grad, double* exp_avg, double* exp_avg_sq, int64_t num_rows, int n,
                         int model, double lr, double beta1, double beta2, double eps_adam, double weight_decay,
                         const double* bias_pows, double eps, const double* total_sqnorm, double max_norm,
                         int32_t* projected_count, int32_t* status, void* stream) {
    using namespace sympa_hip;
    if (num_rows < 0) return fail(SYMPA_ERR_BAD_ARG, "negative row count");
    if (model == SYMPA_MODEL_DUAL)
        return fail(SYMPA_ERR_BAD_ARG, "the compact dual model has no inner product (the reference's inner raises "
                                       "NotImplementedError, compact_dual.py:96): no geodesic RiemannianAdam step");
    if (model != SYMPA_MODEL_UPPER && model != SYMPA_MODEL_BOUNDED) return fail(SYMPA_ERR_BAD_ARG, "unknown model");
    if (n < 1 || n > 8) return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "the geodesic RiemannianAdam step: dims 1..8");
    if (!(eps > 0.0)) return fail(SYMPA_ERR_BAD_ARG, "eps must be > 0");
    if (total_sqnorm != nullptr && !(max_norm > 0.0)) return fail(SYMPA_ERR_BAD_ARG, "max_norm must be > 0");
    if (num_rows == 0) return 0;
    if (table == nullptr || grad == nullptr || exp_avg == nullptr || exp_avg_sq == nullptr || bias_pows == nullptr)
        return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    if (num_rows > (int64_t)0x7fffffff * EXPMAP_BLOCK) return fail(SYMPA_ERR_BAD_ARG, "too many rows for one launch");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (model == SYMPA_MODEL_UPPER)
        return launch_radam_exp_upper(n, table, grad, exp_avg, exp_avg_sq, num_rows, lr, beta1, beta2, eps_adam, weight_decay,
                                      bias_pows, eps, total_sqnorm, max_norm, projected_count, status, s);
    return launch_radam_exp_bounded(n, table, grad, exp_avg, exp_avg_sq, num_rows, lr, beta1, beta2, eps_adam, weight_decay,
                                    bias_pows, eps, total_sqnorm, max_norm, projected_count, status, s);
}

}  // extern "C"
