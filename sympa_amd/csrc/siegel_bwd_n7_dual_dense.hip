// Backward kernel for n = 7, compact dual model, dense per-pair gradient rows (see siegel_bwd_kernel.hpp).
#include "siegel_bwd_kernel.hpp"

namespace sympa_hip {
int launch_bwd_n7_dual_dense(const BwdArgs& a, hipStream_t s) { return launch_bwd_nms<7, sympa::MODEL_DUAL, false>(a, s); }
}  // namespace sympa_hip
