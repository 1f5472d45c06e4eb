// Backward kernels of the compact dual model for dims 9..16: the per-pair adjoint of siegel_math_bwd.hpp with rolled loops over
// per-lane scratch arrays, as siegel_bwd_rolled.hip compiles it for the other two models.
#define SYMPA_UNROLL _Pragma("nounroll")
#include "siegel_bwd_kernel.hpp"

namespace sympa_hip {

int launch_bwd_rolled_dual(const BwdArgs& a, int n, bool scatter, hipStream_t s) {
    switch (n) {
        case 9: return launch_bwd_nm<9, sympa::MODEL_DUAL>(a, scatter, s);
        case 10: return launch_bwd_nm<10, sympa::MODEL_DUAL>(a, scatter, s);
        case 11: return launch_bwd_nm<11, sympa::MODEL_DUAL>(a, scatter, s);
        case 12: return launch_bwd_nm<12, sympa::MODEL_DUAL>(a, scatter, s);
        case 13: return launch_bwd_nm<13, sympa::MODEL_DUAL>(a, scatter, s);
        case 14: return launch_bwd_nm<14, sympa::MODEL_DUAL>(a, scatter, s);
        case 15: return launch_bwd_nm<15, sympa::MODEL_DUAL>(a, scatter, s);
        case 16: return launch_bwd_nm<16, sympa::MODEL_DUAL>(a, scatter, s);
        default: return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "rolled backward covers dims 9..16");
    }
}

}  // namespace sympa_hip
