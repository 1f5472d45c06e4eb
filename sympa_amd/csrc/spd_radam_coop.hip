// spd RiemannianAdam step with sixteen lanes per table row (spd_coop_radam.hpp): M = 3..11 here, 12..16 in spd_radam_coop_hi.hip
#include "spd_coop_bwd_kernel.hpp"
#include "spd_coop_radam.hpp"

namespace sympa_hip {
void launch_spd_coop_radam_hi(int n, double* x, const double* g, double* m, double* sq, int64_t b, const spd_coop::SpdAdamArgs& p,
                              int32_t* status, hipStream_t s);

void launch_spd_coop_radam(int n, double* x, const double* g, double* m, double* sq, int64_t b, double lr, double beta1, double beta2,
                           double eps_adam, double wd, const double* pows, const double* clip, double max_norm, int32_t* status,
                           hipStream_t s) {
    const spd_coop::SpdAdamArgs p{lr, beta1, beta2, eps_adam, wd, max_norm, pows, clip};
    switch (n) {
#define SYMPA_CASE(M) case M: spd_coop::launch_spd_coop_radam_m<M>(x, g, m, sq, b, p, status, s); break;
        SYMPA_CASE(3) SYMPA_CASE(4) SYMPA_CASE(5) SYMPA_CASE(6) SYMPA_CASE(7) SYMPA_CASE(8) SYMPA_CASE(9) SYMPA_CASE(10) SYMPA_CASE(11)
#undef SYMPA_CASE
        default: launch_spd_coop_radam_hi(n, x, g, m, sq, b, p, status, s); break;
    }
}
}  // namespace sympa_hip
