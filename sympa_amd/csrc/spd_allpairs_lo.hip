// spd all-pairs distance rows, sixteen lanes per pair, M = 6..11 (spd_allpairs_kernel.hpp)
#include "spd_allpairs_kernel.hpp"

namespace sympa_hip {
void launch_spd_all_pairs_coop_lo(const SpdAllPairsArgs& a, int n, dim3 grid, hipStream_t s) {
    switch (n) {
        case 6: hipLaunchKernelGGL(spd_all_pairs_kernel<6>, grid, dim3(64), 0, s, a); break;
        case 7: hipLaunchKernelGGL(spd_all_pairs_kernel<7>, grid, dim3(64), 0, s, a); break;
        case 8: hipLaunchKernelGGL(spd_all_pairs_kernel<8>, grid, dim3(64), 0, s, a); break;
        case 9: hipLaunchKernelGGL(spd_all_pairs_kernel<9>, grid, dim3(64), 0, s, a); break;
        case 10: hipLaunchKernelGGL(spd_all_pairs_kernel<10>, grid, dim3(64), 0, s, a); break;
        case 11: hipLaunchKernelGGL(spd_all_pairs_kernel<11>, grid, dim3(64), 0, s, a); break;
        default: break;
    }
}
}  // namespace sympa_hip
