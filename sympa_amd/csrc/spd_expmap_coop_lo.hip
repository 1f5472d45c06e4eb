// spd exponential / logarithm / geodesic maps and the geodesic RSGD step with sixteen lanes per row (spd_expmap_kernel.hpp):
// M = 3..11 here, 12..16 in spd_expmap_coop_hi.hip
#include "spd_expmap_kernel.hpp"

namespace sympa_hip {
void launch_spd_coop_expmap_lo(int op, int n, double* x, const double* p2, double t, int64_t b, double* out, double lr, double wd,
                               const double* clip, double max_norm, int32_t* status, hipStream_t s) {
    switch (n) {
#define SYMPA_CASE(M) case M: spd_coop::launch_spd_coop_expmap_m<M>(op, x, p2, t, b, out, lr, wd, clip, max_norm, status, s); break;
        SYMPA_CASE(3) SYMPA_CASE(4) SYMPA_CASE(5) SYMPA_CASE(6) SYMPA_CASE(7) SYMPA_CASE(8) SYMPA_CASE(9) SYMPA_CASE(10) SYMPA_CASE(11)
#undef SYMPA_CASE
        default: break;
    }
}
}  // namespace sympa_hip
