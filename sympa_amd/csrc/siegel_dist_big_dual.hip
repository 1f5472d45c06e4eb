// Forward, one pair per lane, compact dual model, dims 5..8 (siegel_dist_kernel.hpp).  Compiled like siegel_dist_big.hip, with
// -mllvm -enable-misched=0 (__graft_entry__.py).
#include "siegel_dist_kernel.hpp"

namespace sympa_hip {

int launch_dist_big_dual(const DistArgs& a, int n, hipStream_t s) {
    switch (n) {
        case 5: return launch_n<5, true>(a, SYMPA_MODEL_DUAL, s);
        case 6: return launch_n<6, true>(a, SYMPA_MODEL_DUAL, s);
        case 7: return launch_n<7, true>(a, SYMPA_MODEL_DUAL, s);
        case 8: return launch_n<8, true>(a, SYMPA_MODEL_DUAL, s);
        default: return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "dims 5..8");
    }
}

int launch_multi_big_dual(const MultiArgs& m, unsigned grid, int n, hipStream_t s) {
    switch (n) {
        case 5: return launch_multi_n<5, true>(m, grid, SYMPA_MODEL_DUAL, s);
        case 6: return launch_multi_n<6, true>(m, grid, SYMPA_MODEL_DUAL, s);
        case 7: return launch_multi_n<7, true>(m, grid, SYMPA_MODEL_DUAL, s);
        case 8: return launch_multi_n<8, true>(m, grid, SYMPA_MODEL_DUAL, s);
        default: return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "dims 5..8");
    }
}

}  // namespace sympa_hip
