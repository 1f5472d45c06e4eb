// Siegel backward, EIGHT lanes per pair (two pairs per DPP row: SYMPA_COOP_HALF, spd_coop.hpp): ONE kernel instance, chosen by the
// build, which compiles this file once per SYMPA_BWD_HALF line of siegel_bwd_instances.hpp with the line's words -- model, M = n,
// output form.  One kernel per compile job (the build's DPP hazard check works per object).
#if !defined(SYMPA_INST_MODEL) || !defined(SYMPA_INST_N) || !defined(SYMPA_INST_FORM)
#error "compiled once per SYMPA_BWD_HALF line of siegel_bwd_instances.hpp: -DSYMPA_INST_MODEL=upper -DSYMPA_INST_N=5 -DSYMPA_INST_FORM=dense"
#endif
#define SYMPA_COOP_HALF
#define SYMPA_INST_IS_upper 1
#define SYMPA_INST_IS_bounded 0
#define SYMPA_INST_IS_(M) SYMPA_INST_IS_##M
#define SYMPA_INST_IS(M) SYMPA_INST_IS_(M)
#if SYMPA_INST_IS(SYMPA_INST_MODEL)       // the upper model only
#define SYMPA_COOP_BWD_WAVES_UPPER 2      // two 256-register waves per SIMD: fused step n = 8 1663 -> 1487 us per 262 144 pairs
#endif
#include "siegel_coop_bwd_kernel.hpp"

namespace sympa_hip {
#define SYMPA_BWD_HALF(M, N, F) \
    int SYMPA_BWD_HALF_NAME(M, N, F)(const BwdArgs& a, hipStream_t s) { return launch_coop_bwd_ms<bwd_word::M, N, bwd_word::F>(a, s); }
SYMPA_BWD_HALF(SYMPA_INST_MODEL, SYMPA_INST_N, SYMPA_INST_FORM)
}  // namespace sympa_hip
