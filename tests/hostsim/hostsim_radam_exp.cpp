// TEST INFRASTRUCTURE ONLY (CPU).  The geodesic RiemannianAdam row (sympa::radam_exp_row; sympa_amd/csrc/siegel_radam_exp_math.hpp)
// compiled with g++ for dims 1..8 and the upper / bounded models, next to the other hostsim libraries, which stay as they are.
// Nothing in sympa_amd/ loads this library.
#include <cmath>
#include <cstdint>
#include "../../sympa_amd/csrc/siegel_radam_exp_math.hpp"

namespace {

// x, grad, m [b,2,n,n], s [b] -> out_x (after projx), out_m [b,2,n,n], out_s [b]; moved[0] = rows projx moved
template <int N, int MODEL>
int run(const double* x, const double* grad, const double* m, const double* s, int64_t b, double lr, double b1, double b2,
        double eps_adam, double wd, double pow1, double pow2, double coef, double eps, double* out_x, double* out_m, double* out_s,
        int32_t* moved, int32_t* status) {
    int st = 0, mv = 0;
    constexpr int64_t ROW = 2 * N * N;
    for (int64_t i = 0; i < b; ++i) {
        sympa::CMat<N> z, g, mm;
        sympa::load_full<N>(x + i * ROW, z);
        sympa::load_full<N>(grad + i * ROW, g);
        sympa::load_full<N>(m + i * ROW, mm);
        double sn;
        mv += sympa::radam_exp_row<N, MODEL>(z, g, mm, s[i], sn, lr, b1, b2, eps_adam, wd, pow1, pow2, coef, eps, st) ? 1 : 0;
        sympa::store_full<N>(out_x + i * ROW, z);
        sympa::store_full<N>(out_m + i * ROW, g);
        out_s[i] = sn;
    }
    if (moved) *moved = mv;
    if (status) *status = st;
    return 0;
}
}  // namespace

extern "C" int sympa_hostsim_radam_exp(const double* x, const double* grad, const double* m, const double* s, int64_t b, int n,
                                       int model, double lr, double b1, double b2, double eps_adam, double wd, double pow1,
                                       double pow2, double coef, double eps, double* out_x, double* out_m, double* out_s,
                                       int32_t* moved, int32_t* status) {
    if (model != sympa::MODEL_UPPER && model != sympa::MODEL_BOUNDED) return -1;
#define CALL(N)                                                                                                                  \
    case N:                                                                                                                      \
        return model == sympa::MODEL_UPPER                                                                                       \
                   ? run<N, sympa::MODEL_UPPER>(x, grad, m, s, b, lr, b1, b2, eps_adam, wd, pow1, pow2, coef, eps, out_x, out_m,  \
                                                out_s, moved, status)                                                            \
                   : run<N, sympa::MODEL_BOUNDED>(x, grad, m, s, b, lr, b1, b2, eps_adam, wd, pow1, pow2, coef, eps, out_x, out_m, \
                                                  out_s, moved, status);
    switch (n) {
        CALL(1) CALL(2) CALL(3) CALL(4) CALL(5) CALL(6) CALL(7) CALL(8)
        default: return -2;
    }
#undef CALL
}
