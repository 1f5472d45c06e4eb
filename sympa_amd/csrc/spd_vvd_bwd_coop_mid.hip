// spd vector-valued distance, backward, sixteen lanes per pair, M = 10..13 (spd_vvd_kernel.hpp)
#include "spd_vvd_kernel.hpp"

namespace sympa_hip {
void launch_spd_vvd_bwd_coop_mid(const SpdVvdArgs& a, int n, hipStream_t s) {
    const dim3 grid = spd_vvd_coop_bwd_grid(a.b, n);
    switch (n) {
        case 10: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<10>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<10>())); break;
        case 11: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<11>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<11>())); break;
        case 12: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<12>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<12>())); break;
        case 13: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<13>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<13>())); break;
        default: break;
    }
}
}  // namespace sympa_hip
