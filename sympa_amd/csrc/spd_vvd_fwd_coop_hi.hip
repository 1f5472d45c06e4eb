// spd vector-valued distance, forward, sixteen lanes per pair, M = 12..16 (spd_vvd_kernel.hpp)
#include "spd_vvd_kernel.hpp"

namespace sympa_hip {
void launch_spd_vvd_fwd_coop_hi(const SpdVvdArgs& a, int n, hipStream_t s) {
    const dim3 grid((unsigned)((a.b + 63) / 64));
    switch (n) {
        case 12: hipLaunchKernelGGL(spd_vvd_coop_fwd_kernel<12>, grid, dim3(64), 0, s, a); break;
        case 13: hipLaunchKernelGGL(spd_vvd_coop_fwd_kernel<13>, grid, dim3(64), 0, s, a); break;
        case 14: hipLaunchKernelGGL(spd_vvd_coop_fwd_kernel<14>, grid, dim3(64), 0, s, a); break;
        case 15: hipLaunchKernelGGL(spd_vvd_coop_fwd_kernel<15>, grid, dim3(64), 0, s, a); break;
        case 16: hipLaunchKernelGGL(spd_vvd_coop_fwd_kernel<16>, grid, dim3(64), 0, s, a); break;
        default: break;
    }
}
}  // namespace sympa_hip
