// Siegel backward, one pair per lane, n = 7, 8 (siegel_bwd_kernel.hpp): ONE kernel instance, chosen by the build, which compiles
// this file once per SYMPA_BWD_ONE_LANE line of siegel_bwd_instances.hpp with the line's words -- model, n, output form.  One kernel
// per compile job: the fully unrolled adjoint of an 8 x 8 pair takes a minute or two to compile.
#if !defined(SYMPA_INST_MODEL) || !defined(SYMPA_INST_N) || !defined(SYMPA_INST_FORM)
#error "compiled once per SYMPA_BWD_ONE_LANE line of siegel_bwd_instances.hpp: -DSYMPA_INST_MODEL=upper -DSYMPA_INST_N=7 -DSYMPA_INST_FORM=dense"
#endif
#include "siegel_bwd_kernel.hpp"

namespace sympa_hip {
#define SYMPA_BWD_ONE_LANE(M, N, F) \
    int SYMPA_BWD_ONE_LANE_NAME(M, N, F)(const BwdArgs& a, hipStream_t s) { return launch_bwd_nms<N, bwd_word::M, bwd_word::F>(a, s); }
SYMPA_BWD_ONE_LANE(SYMPA_INST_MODEL, SYMPA_INST_N, SYMPA_INST_FORM)
}  // namespace sympa_hip
