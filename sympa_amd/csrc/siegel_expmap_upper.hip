// gfx950 instantiations of the exponential / logarithm maps and the geodesic RiemannianSGD step, upper model, dims 1..8
// (siegel_expmap_kernel.hpp).
#include "siegel_expmap_kernel.hpp"

namespace sympa_hip {

int launch_expmap_upper(int op, int n, double* a, const double* c, double* out, int64_t b, double lr, double wd, double eps,
                        int32_t* projected, int32_t* status, hipStream_t s) {
    return launch_expmap_model<sympa::MODEL_UPPER>(op, n, a, c, out, b, lr, wd, eps, projected, status, s);
}

}  // namespace sympa_hip
