// Backward kernel for n = 8, compact dual model, dense per-pair gradient rows (see siegel_bwd_kernel.hpp).
#include "siegel_bwd_kernel.hpp"

namespace sympa_hip {
int launch_bwd_n8_dual_dense(const BwdArgs& a, hipStream_t s) { return launch_bwd_nms<8, sympa::MODEL_DUAL, false>(a, s); }
}  // namespace sympa_hip
