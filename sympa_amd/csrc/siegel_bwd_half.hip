// Siegel backward, eight lanes per pair (SYMPA_COOP_HALF kernels: the SYMPA_BWD_HALF instances of siegel_bwd_instances.hpp,
// compiled from siegel_bwd_half_instance.hip): dispatch, dims 5..8
#include "siegel_bwd_kernel.hpp"

namespace sympa_hip {
int launch_bwd_half(const BwdArgs& a, int n, int model, bool scatter, hipStream_t s) {
    const int m = model == SYMPA_MODEL_UPPER ? bwd_word::upper : bwd_word::bounded;
#define SYMPA_BWD_HALF(M, N, F) \
    if (n == N && m == bwd_word::M && scatter == bwd_word::F) return SYMPA_BWD_HALF_NAME(M, N, F)(a, s);
#include "siegel_bwd_instances.hpp"
    return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "eight-lanes-per-pair backward covers dims 5..8");
}
}  // namespace sympa_hip
