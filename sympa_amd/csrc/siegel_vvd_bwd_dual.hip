// Backward of the vector-valued distance, compact dual model, one pair per lane, dims 1..6 (siegel_vvd_bwd_kernel.hpp).
#include "siegel_vvd_bwd_kernel.hpp"

namespace sympa_hip {

int launch_vvd_bwd_dual(const VvdBwdArgs& a, int n, bool scatter, hipStream_t s) {
    switch (n) {
        case 1: return launch_vvd_bwd_nm<1, sympa::MODEL_DUAL>(a, scatter, s);
        case 2: return launch_vvd_bwd_nm<2, sympa::MODEL_DUAL>(a, scatter, s);
        case 3: return launch_vvd_bwd_nm<3, sympa::MODEL_DUAL>(a, scatter, s);
        case 4: return launch_vvd_bwd_nm<4, sympa::MODEL_DUAL>(a, scatter, s);
        case 5: return launch_vvd_bwd_nm<5, sympa::MODEL_DUAL>(a, scatter, s);
        case 6: return launch_vvd_bwd_nm<6, sympa::MODEL_DUAL>(a, scatter, s);
        default: return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "unrolled vvd backward covers dims 1..6");
    }
}

}  // namespace sympa_hip
