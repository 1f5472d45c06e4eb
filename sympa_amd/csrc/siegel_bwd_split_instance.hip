// Split Siegel backward (siegel_bwd_split_kernel.hpp), one pair per lane: ONE kernel instance, chosen by the build, which compiles
// this file once per SYMPA_BWD_SPLIT_SPECTRAL line of siegel_bwd_instances.hpp with the line's words -- model, n -- for stage 1
// (eigen-decomposition with vectors -> Hbar, K), and once per SYMPA_BWD_SPLIT_GRADIENT line -- model, n, output form -- for stage 2
// (factors and E again, products / solves / congruences from Hbar, K).  One kernel per compile job: the unrolled kernels compile
// in parallel.
#if !defined(SYMPA_INST_MODEL) || !defined(SYMPA_INST_N)
#error "compiled once per SYMPA_BWD_SPLIT_* line of siegel_bwd_instances.hpp: -DSYMPA_INST_MODEL=upper -DSYMPA_INST_N=5 [-DSYMPA_INST_FORM=dense]"
#endif
#include "siegel_bwd_split_kernel.hpp"

namespace sympa_hip {
#ifndef SYMPA_INST_FORM
#define SYMPA_BWD_SPLIT_SPECTRAL(M, N) \
    int SYMPA_BWD_SPLIT_SPECTRAL_NAME(M, N)(const SplitArgs& sa, hipStream_t s) { return launch_bwd_split_spectral<N, bwd_word::M>(sa, s); }
SYMPA_BWD_SPLIT_SPECTRAL(SYMPA_INST_MODEL, SYMPA_INST_N)
#else
#define SYMPA_BWD_SPLIT_GRADIENT(M, N, F) \
    int SYMPA_BWD_SPLIT_GRADIENT_NAME(M, N, F)(const SplitArgs& sa, hipStream_t s) { return launch_bwd_split_gradient<N, bwd_word::M, bwd_word::F>(sa, s); }
SYMPA_BWD_SPLIT_GRADIENT(SYMPA_INST_MODEL, SYMPA_INST_N, SYMPA_INST_FORM)
#endif
}  // namespace sympa_hip
