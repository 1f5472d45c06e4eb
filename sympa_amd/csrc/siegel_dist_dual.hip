// Forward, one pair per lane, compact dual model, dims 1..4 (siegel_dist_kernel.hpp); dims 5..8: siegel_dist_big_dual.hip.
#include "siegel_dist_kernel.hpp"

namespace sympa_hip {

int launch_dist_dual(const DistArgs& a, int n, hipStream_t s) {
    switch (n) {
        case 1: return launch_n<1, true>(a, SYMPA_MODEL_DUAL, s);
        case 2: return launch_n<2, true>(a, SYMPA_MODEL_DUAL, s);
        case 3: return launch_n<3, true>(a, SYMPA_MODEL_DUAL, s);
        case 4: return launch_n<4, true>(a, SYMPA_MODEL_DUAL, s);
        default: return launch_dist_big_dual(a, n, s);
    }
}

int launch_multi_dual(const MultiArgs& m, unsigned grid, int n, hipStream_t s) {
    switch (n) {
        case 1: return launch_multi_n<1, true>(m, grid, SYMPA_MODEL_DUAL, s);
        case 2: return launch_multi_n<2, true>(m, grid, SYMPA_MODEL_DUAL, s);
        case 3: return launch_multi_n<3, true>(m, grid, SYMPA_MODEL_DUAL, s);
        case 4: return launch_multi_n<4, true>(m, grid, SYMPA_MODEL_DUAL, s);
        default: return launch_multi_big_dual(m, grid, n, s);
    }
}

}  // namespace sympa_hip
