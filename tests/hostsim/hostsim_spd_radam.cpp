// g++ build of the spd model's RiemannianAdam row (sympa::spd_row_radam, sympa_amd/csrc/spd_math_bwd.hpp)
// for the CPU tests: the rows one after the other, as spd_radam_kernel of sympa_amd/csrc/spd_bwd.hip runs them one per lane.
#include <cstdint>

#include "../../sympa_amd/csrc/spd_math_bwd.hpp"

extern "C" {

// x, m [b, n, n] and s [b] are updated in place, like the kernel's table, exp_avg and exp_avg_sq.  p1, p2: beta^t of this step.
// status: the or of the rows' status bits; bad_rows: rows with a bit set.
int sympa_hostsim_spd_radam(double* x, const double* g, double* m, double* s, int64_t b, int n, double lr, double beta1,
                            double beta2, double eps_adam, double wd, double coef, double p1, double p2, int32_t* status,
                            int32_t* bad_rows) {
    if (n < 1 || n > sympa::SPD_MAX_N) return -2;
    static thread_local sympa::SpdRowWork w;
    int st_all = 0, bad = 0;
    for (int64_t i = 0; i < b; ++i) {
        int st = 0;
        sympa::spd_row_radam(w, x + i * n * n, g + i * n * n, m + i * n * n, s[i], n, lr, beta1, beta2, eps_adam, wd, coef, p1, p2, st);
        st_all |= st;
        bad += st != 0;
    }
    if (status != nullptr) *status = st_all;
    if (bad_rows != nullptr) *bad_rows = bad;
    return 0;
}

}  // extern "C"
