// spd vector-valued distance, forward, sixteen lanes per pair, M = 6..11 (spd_vvd_kernel.hpp)
#include "spd_vvd_kernel.hpp"

namespace sympa_hip {
void launch_spd_vvd_fwd_coop_lo(const SpdVvdArgs& a, int n, hipStream_t s) {
    const dim3 grid((unsigned)((a.b + 63) / 64));
    switch (n) {
        case 6: hipLaunchKernelGGL(spd_vvd_coop_fwd_kernel<6>, grid, dim3(64), 0, s, a); break;
        case 7: hipLaunchKernelGGL(spd_vvd_coop_fwd_kernel<7>, grid, dim3(64), 0, s, a); break;
        case 8: hipLaunchKernelGGL(spd_vvd_coop_fwd_kernel<8>, grid, dim3(64), 0, s, a); break;
        case 9: hipLaunchKernelGGL(spd_vvd_coop_fwd_kernel<9>, grid, dim3(64), 0, s, a); break;
        case 10: hipLaunchKernelGGL(spd_vvd_coop_fwd_kernel<10>, grid, dim3(64), 0, s, a); break;
        case 11: hipLaunchKernelGGL(spd_vvd_coop_fwd_kernel<11>, grid, dim3(64), 0, s, a); break;
        default: break;
    }
}
}  // namespace sympa_hip
