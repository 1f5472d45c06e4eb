// Backward kernels of the compact dual model, one pair per lane, dims 1..6 (siegel_bwd_kernel.hpp); dims 7, 8 have one unit per
// kernel like the other models.
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
        case 7: return launch_bwd_n7_dual(a, scatter, s);
        case 8: return launch_bwd_n8_dual(a, scatter, s);
        default: return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "one-pair-per-lane backward: dims 1..8");
    }
}

}  // namespace sympa_hip
