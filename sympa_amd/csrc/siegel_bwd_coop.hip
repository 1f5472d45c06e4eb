// Siegel backward, sixteen lanes per pair: dispatch over model, size and output form (the SYMPA_BWD_COOP instances of
// siegel_bwd_instances.hpp, compiled from siegel_bwd_coop_instance.hip)
#include "siegel_coop_bwd_kernel.hpp"

namespace sympa_hip {
int launch_bwd_coop(const BwdArgs& a, int n, int model, bool scatter, hipStream_t s) {
    const int m = model == SYMPA_MODEL_UPPER ? bwd_word::upper : bwd_word::bounded;
#define SYMPA_BWD_COOP(M, N, F) \
    if (n == N && m == bwd_word::M && scatter == bwd_word::F) return SYMPA_BWD_COOP_NAME(M, N, F)(a, s);
#include "siegel_bwd_instances.hpp"
    return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "sixteen-lanes-per-pair backward covers dims 9..16");
}
}  // namespace sympa_hip
