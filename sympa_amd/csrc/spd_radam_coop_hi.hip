// spd RiemannianAdam step with sixteen lanes per table row (spd_coop_radam.hpp): M = 12..16 (dispatched from spd_radam_coop.hip)
#include "spd_coop_bwd_kernel.hpp"
#include "spd_coop_radam.hpp"

namespace sympa_hip {
void launch_spd_coop_radam_hi(int n, double* x, const double* g, double* m, double* sq, int64_t b, const spd_coop::SpdAdamArgs& p,
                              int32_t* status, hipStream_t s) {
    switch (n) {
#define SYMPA_CASE(M) case M: spd_coop::launch_spd_coop_radam_m<M>(x, g, m, sq, b, p, status, s); break;
        SYMPA_CASE(12) SYMPA_CASE(13) SYMPA_CASE(14) SYMPA_CASE(15) SYMPA_CASE(16)
#undef SYMPA_CASE
        default: break;
    }
}
}  // namespace sympa_hip
