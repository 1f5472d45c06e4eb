// gfx950 instantiations of the geodesic RiemannianAdam step, bounded model, dims 1..8 (siegel_radam_exp_kernel.hpp).
#include "siegel_radam_exp_kernel.hpp"

namespace sympa_hip {

int launch_radam_exp_bounded(int n, double* z, const double* grad, double* m, double* v, int64_t b, double lr, double b1, double b2,
                             double eps_adam, double wd, const double* pows, double eps, const double* clip, double max_norm,
                             int32_t* projected, int32_t* status, hipStream_t s) {
    return launch_radam_exp_model<sympa::MODEL_BOUNDED>(n, z, grad, m, v, b, lr, b1, b2, eps_adam, wd, pows, eps, clip, max_norm,
                                                        projected, status, s);
}

}  // namespace sympa_hip
