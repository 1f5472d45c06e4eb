// Optimiser-side table operations of the compact dual model, one row per lane, dims 1..8 (siegel_table_kernel.hpp):
// egrad2rgrad = (I + conj(Z) Z) G (I + Z conj(Z)), projx = symmetrise, the RSGD step from the two.
#include "siegel_table_kernel.hpp"

namespace sympa_hip {
int launch_table_dual(int op, int n, double* z, const double* g, double* out, int64_t b, double lr, double wd, double eps,
                      int32_t* projected, int32_t* status, hipStream_t s, const double* clip, double max_norm) {
    switch (n) {
        case 1: return launch_table<1, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 2: return launch_table<2, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 3: return launch_table<3, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 4: return launch_table<4, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 5: return launch_table<5, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 6: return launch_table<6, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 7: return launch_table<7, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 8: return launch_table<8, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        default: return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "dims 1..8");
    }
}
}  // namespace sympa_hip
