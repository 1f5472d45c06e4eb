// Backward of the vector-valued distance for dims 7..16, compact dual model: rolled loops over per-lane scratch
// (siegel_vvd_bwd_rolled.hip has the recipe).
#define SYMPA_UNROLL _Pragma("nounroll")
#include "siegel_vvd_bwd_kernel.hpp"

namespace sympa_hip {

int launch_vvd_bwd_rolled_dual(const VvdBwdArgs& a, int n, bool scatter, hipStream_t s) {
    switch (n) {
        case 7: return launch_vvd_bwd_nm<7, sympa::MODEL_DUAL>(a, scatter, s);
        case 8: return launch_vvd_bwd_nm<8, sympa::MODEL_DUAL>(a, scatter, s);
        case 9: return launch_vvd_bwd_nm<9, sympa::MODEL_DUAL>(a, scatter, s);
        case 10: return launch_vvd_bwd_nm<10, sympa::MODEL_DUAL>(a, scatter, s);
        case 11: return launch_vvd_bwd_nm<11, sympa::MODEL_DUAL>(a, scatter, s);
        case 12: return launch_vvd_bwd_nm<12, sympa::MODEL_DUAL>(a, scatter, s);
        case 13: return launch_vvd_bwd_nm<13, sympa::MODEL_DUAL>(a, scatter, s);
        case 14: return launch_vvd_bwd_nm<14, sympa::MODEL_DUAL>(a, scatter, s);
        case 15: return launch_vvd_bwd_nm<15, sympa::MODEL_DUAL>(a, scatter, s);
        case 16: return launch_vvd_bwd_nm<16, sympa::MODEL_DUAL>(a, scatter, s);
        default: return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "rolled vvd backward covers dims 7..16");
    }
}

}  // namespace sympa_hip
