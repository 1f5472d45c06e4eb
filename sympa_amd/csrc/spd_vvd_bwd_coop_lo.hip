// spd vector-valued distance, backward, sixteen lanes per pair, M = 3..9 (spd_vvd_kernel.hpp)
#include "spd_vvd_kernel.hpp"

namespace sympa_hip {
void launch_spd_vvd_bwd_coop_lo(const SpdVvdArgs& a, int n, hipStream_t s) {
    const dim3 grid = spd_vvd_coop_bwd_grid(a.b, n);
    switch (n) {
        case 3: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<3>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<3>())); break;
        case 4: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<4>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<4>())); break;
        case 5: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<5>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<5>())); break;
        case 6: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<6>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<6>())); break;
        case 7: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<7>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<7>())); break;
        case 8: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<8>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<8>())); break;
        case 9: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<9>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<9>())); break;
        default: break;
    }
}
}  // namespace sympa_hip
