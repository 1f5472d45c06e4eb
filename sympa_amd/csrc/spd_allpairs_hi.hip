// spd all-pairs distance rows, sixteen lanes per pair, M = 12..16 (spd_allpairs_kernel.hpp)
#include "spd_allpairs_kernel.hpp"

namespace sympa_hip {
void launch_spd_all_pairs_coop_hi(const SpdAllPairsArgs& a, int n, dim3 grid, hipStream_t s) {
    switch (n) {
        case 12: hipLaunchKernelGGL(spd_all_pairs_kernel<12>, grid, dim3(64), 0, s, a); break;
        case 13: hipLaunchKernelGGL(spd_all_pairs_kernel<13>, grid, dim3(64), 0, s, a); break;
        case 14: hipLaunchKernelGGL(spd_all_pairs_kernel<14>, grid, dim3(64), 0, s, a); break;
        case 15: hipLaunchKernelGGL(spd_all_pairs_kernel<15>, grid, dim3(64), 0, s, a); break;
        case 16: hipLaunchKernelGGL(spd_all_pairs_kernel<16>, grid, dim3(64), 0, s, a); break;
        default: break;
    }
}
}  // namespace sympa_hip
