// Backward kernels of the compact dual model, one pair per lane, dims 1..6 (siegel_bwd_kernel.hpp); dims 7, 8 have one compile job
// per kernel like the other models (the dual lines of SYMPA_BWD_ONE_LANE in siegel_bwd_instances.hpp).
#include "siegel_bwd_kernel.hpp"

namespace sympa_hip {

int launch_bwd_dual(const BwdArgs& a, int n, bool scatter, hipStream_t s) {
    switch (n) {
        case 1: return launch_bwd_nm<1, sympa::MODEL_DUAL>(a, scatter, s);
        case 2: return launch_bwd_nm<2, sympa::MODEL_DUAL>(a, scatter, s);
        case 3: return launch_bwd_nm<3, sympa::MODEL_DUAL>(a, scatter, s);
        case 4: return launch_bwd_nm<4, sympa::MODEL_DUAL>(a, scatter, s);
        case 5: return launch_bwd_nm<5, sympa::MODEL_DUAL>(a, scatter, s);
        case 6: return launch_bwd_nm<6, sympa::MODEL_DUAL>(a, scatter, s);
        default: break;
    }
#define SYMPA_BWD_ONE_LANE(M, N, F) \
    if (n == N && bwd_word::M == bwd_word::dual && scatter == bwd_word::F) return SYMPA_BWD_ONE_LANE_NAME(M, N, F)(a, s);
#include "siegel_bwd_instances.hpp"
    return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "one-pair-per-lane backward: dims 1..8");
}

}  // namespace sympa_hip
