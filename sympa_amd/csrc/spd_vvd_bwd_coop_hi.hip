// spd vector-valued distance, backward, sixteen lanes per pair, M = 14..16 (spd_vvd_kernel.hpp)
#include "spd_vvd_kernel.hpp"

namespace sympa_hip {
void launch_spd_vvd_bwd_coop_hi(const SpdVvdArgs& a, int n, hipStream_t s) {
    const dim3 grid = spd_vvd_coop_bwd_grid(a.b, n);
    switch (n) {
        case 14: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<14>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<14>())); break;
        case 15: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<15>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<15>())); break;
        case 16: hipLaunchKernelGGL(spd_vvd_coop_bwd_kernel<16>, grid, dim3(64), 0, s, a, spd_coop::coop_rounds(a.b, spd_vvd_coop_bwd_waves<16>())); break;
        default: break;
    }
}
}  // namespace sympa_hip
