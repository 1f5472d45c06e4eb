// Backward of the vector-valued distance for dims 7..16, upper and bounded model: the SAME per-pair adjoint as dims <= 6
// (siegel_math_bwd.hpp) compiled with rolled loops -- SYMPA_UNROLL = nounroll -- so that the working matrices are per-lane scratch
// arrays instead of registers (the recipe of siegel_bwd_rolled.hip).  One pair per lane, 64-thread blocks.  Functional, not tuned.
#define SYMPA_UNROLL _Pragma("nounroll")
#include "siegel_vvd_bwd_kernel.hpp"

namespace sympa_hip {

template <int N>
int launch_vvd_bwd_rolled_n(const VvdBwdArgs& a, int model, bool scatter, hipStream_t s) {
    return model == SYMPA_MODEL_UPPER ? launch_vvd_bwd_nm<N, sympa::MODEL_UPPER>(a, scatter, s)
                                      : launch_vvd_bwd_nm<N, sympa::MODEL_BOUNDED>(a, scatter, s);
}

int launch_vvd_bwd_rolled(const VvdBwdArgs& a, int n, int model, bool scatter, hipStream_t s) {
    if (model == SYMPA_MODEL_DUAL) return launch_vvd_bwd_rolled_dual(a, n, scatter, s);
    switch (n) {
        case 7: return launch_vvd_bwd_rolled_n<7>(a, model, scatter, s);
        case 8: return launch_vvd_bwd_rolled_n<8>(a, model, scatter, s);
        case 9: return launch_vvd_bwd_rolled_n<9>(a, model, scatter, s);
        case 10: return launch_vvd_bwd_rolled_n<10>(a, model, scatter, s);
        case 11: return launch_vvd_bwd_rolled_n<11>(a, model, scatter, s);
        case 12: return launch_vvd_bwd_rolled_n<12>(a, model, scatter, s);
        case 13: return launch_vvd_bwd_rolled_n<13>(a, model, scatter, s);
        case 14: return launch_vvd_bwd_rolled_n<14>(a, model, scatter, s);
        case 15: return launch_vvd_bwd_rolled_n<15>(a, model, scatter, s);
        case 16: return launch_vvd_bwd_rolled_n<16>(a, model, scatter, s);
        default: return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "rolled vvd backward covers dims 7..16");
    }
}

}  // namespace sympa_hip
