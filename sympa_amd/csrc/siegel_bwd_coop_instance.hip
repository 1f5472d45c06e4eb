// Siegel backward, sixteen lanes per pair (siegel_coop_bwd_kernel.hpp): ONE kernel instance, chosen by the build, which compiles
// this file once per SYMPA_BWD_COOP line of siegel_bwd_instances.hpp with the line's words -- model, M = n, output form.
// One kernel per compile job: the build checks each object's ISA for the DPP copy hazard (tools/check_dpp_hazards.py) and only
// a kernel that fails pays for the safe form.
#if !defined(SYMPA_INST_MODEL) || !defined(SYMPA_INST_N) || !defined(SYMPA_INST_FORM)
#error "compiled once per SYMPA_BWD_COOP line of siegel_bwd_instances.hpp: -DSYMPA_INST_MODEL=upper -DSYMPA_INST_N=9 -DSYMPA_INST_FORM=dense"
#endif
#include "siegel_coop_bwd_kernel.hpp"

namespace sympa_hip {
#define SYMPA_BWD_COOP(M, N, F) \
    int SYMPA_BWD_COOP_NAME(M, N, F)(const BwdArgs& a, hipStream_t s) { return launch_coop_bwd_ms<bwd_word::M, N, bwd_word::F>(a, s); }
SYMPA_BWD_COOP(SYMPA_INST_MODEL, SYMPA_INST_N, SYMPA_INST_FORM)
}  // namespace sympa_hip
