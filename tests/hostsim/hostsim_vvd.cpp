// TEST INFRASTRUCTURE ONLY (CPU).  The backward of the vector-valued distance (sympa::pair_backward_vvd, sympa_amd/csrc/
// siegel_math_bwd.hpp) compiled with g++ for dims 1..16 and the three Siegel models, next to hostsim.cpp and hostsim_dual.cpp,
// which stay as they are.  Nothing in sympa_amd/ loads this library.
#include <cmath>
#include <cstdint>
#include "../../sympa_amd/csrc/siegel_math.hpp"
#include "../../sympa_amd/csrc/siegel_math_bwd.hpp"
#include "../../sympa_amd/csrc/siegel_table_math.hpp"

namespace {

template <int N, int MODEL>
int run(const double* z1, const double* z2, const double* gv, int64_t b, double eps, double* g1, double* g2, double* v,
        int32_t* status) {
    int st = 0;
    for (int64_t i = 0; i < b; ++i) {
        sympa::CMat<N> a, c, ga, gc;
        sympa::load_point<N>(z1 + i * 2 * N * N, a);
        sympa::load_point<N>(z2 + i * 2 * N * N, c);
        sympa::pair_backward_vvd<N, MODEL>(a, c, gv + i * N, 1.0 / eps, ga, gc, v ? v + i * N : nullptr, st);
        sympa::store_full<N>(g1 + i * 2 * N * N, ga);
        sympa::store_full<N>(g2 + i * 2 * N * N, gc);
    }
    if (status) *status = st;
    return 0;
}

template <int N>
int run_n(int model, const double* z1, const double* z2, const double* gv, int64_t b, double eps, double* g1, double* g2, double* v,
          int32_t* status) {
    if (model == sympa::MODEL_UPPER) return run<N, sympa::MODEL_UPPER>(z1, z2, gv, b, eps, g1, g2, v, status);
    if (model == sympa::MODEL_BOUNDED) return run<N, sympa::MODEL_BOUNDED>(z1, z2, gv, b, eps, g1, g2, v, status);
    if (model == sympa::MODEL_DUAL) return run<N, sympa::MODEL_DUAL>(z1, z2, gv, b, eps, g1, g2, v, status);
    return -1;
}
}  // namespace

// z1, z2 [b,2,n,n], gv [b,n] (cotangent on the ascending v) -> g1, g2 [b,2,n,n], v [b,n] (may be null), status bits
extern "C" int sympa_hostsim_vvd_bwd(const double* z1, const double* z2, const double* gv, int64_t b, int n, int model, double eps,
                                     double* g1, double* g2, double* v, int32_t* status) {
#define CALL(N) case N: return run_n<N>(model, z1, z2, gv, b, eps, g1, g2, v, status);
    switch (n) {
        CALL(1) CALL(2) CALL(3) CALL(4) CALL(5) CALL(6) CALL(7) CALL(8)
        CALL(9) CALL(10) CALL(11) CALL(12) CALL(13) CALL(14) CALL(15) CALL(16)
        default: return -2;
    }
#undef CALL
}
