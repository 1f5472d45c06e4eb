// gfx950 instantiations of the parallel transport along geodesics, bounded model, dims 1..8 (siegel_transp_kernel.hpp).
#include "siegel_transp_kernel.hpp"

namespace sympa_hip {

int launch_transp_bounded(int op, int n, const double* a, const double* c, const double* v, double* out_y, double* out_v, int64_t b,
                          int32_t* status, hipStream_t s) {
    return launch_transp_model<sympa::MODEL_BOUNDED>(op, n, a, c, v, out_y, out_v, b, status, s);
}

}  // namespace sympa_hip
