// Optimiser-side table operations of the compact dual model for dims 9..16: the per-row arithmetic of siegel_table_math.hpp with
// rolled loops over per-lane scratch, as siegel_table_rolled.hip compiles it for the other two models.
#define SYMPA_UNROLL _Pragma("nounroll")
#include "siegel_table_kernel.hpp"

namespace sympa_hip {
int launch_table_rolled_dual(int op, int n, double* z, const double* g, double* out, int64_t b, double lr, double wd, double eps,
                             int32_t* projected, int32_t* status, hipStream_t s, const double* clip, double max_norm) {
    switch (n) {
        case 9: return launch_table<9, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 10: return launch_table<10, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 11: return launch_table<11, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 12: return launch_table<12, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 13: return launch_table<13, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 14: return launch_table<14, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 15: return launch_table<15, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        case 16: return launch_table<16, true>(op, SYMPA_MODEL_DUAL, z, g, out, b, lr, wd, eps, projected, status, s, clip, max_norm);
        default: return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "rolled table operations cover dims 9..16");
    }
}
}  // namespace sympa_hip
