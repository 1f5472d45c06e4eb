// TEST INFRASTRUCTURE ONLY (CPU).  The exponential / logarithm maps and the geodesic RiemannianSGD row (sympa::expmap_row,
// logmap_pair, rsgd_exp_row; sympa_amd/csrc/siegel_expmap_math.hpp) compiled with g++ for dims 1..8 and the upper / bounded
// models, next to the other hostsim libraries, which stay as they are.  Nothing in sympa_amd/ loads this library.
#include <cmath>
#include <cstdint>
#include "../../sympa_amd/csrc/siegel_expmap_math.hpp"

namespace {

// op 0: out = expmap(a, c);  op 1: out = logmap(a, c);  op 2: out = rsgd_exp_row(a, grad = c), moved[i] = the clamp moved the row
template <int N, int MODEL>
int run(int op, const double* a, const double* c, int64_t b, double lr, double wd, double eps, double* out, int32_t* moved,
        int32_t* status) {
    int st = 0;
    constexpr int64_t ROW = 2 * N * N;
    for (int64_t i = 0; i < b; ++i) {
        sympa::CMat<N> x, y, r;
        sympa::load_full<N>(a + i * ROW, x);
        sympa::load_full<N>(c + i * ROW, y);
        if (op == 0) {
            sympa::expmap_row<N, MODEL>(x, y, r, st);
        } else if (op == 1) {
            sympa::logmap_pair<N, MODEL>(x, y, r, st);
        } else {
            const bool m = sympa::rsgd_exp_row<N, MODEL>(x, y, lr, wd, eps, st);
            if (moved) moved[i] = m ? 1 : 0;
            r = x;
        }
        sympa::store_full<N>(out + i * ROW, r);
    }
    if (status) *status = st;
    return 0;
}

template <int N>
int run_n(int op, int model, const double* a, const double* c, int64_t b, double lr, double wd, double eps, double* out,
          int32_t* moved, int32_t* status) {
    if (model == sympa::MODEL_UPPER) return run<N, sympa::MODEL_UPPER>(op, a, c, b, lr, wd, eps, out, moved, status);
    if (model == sympa::MODEL_BOUNDED) return run<N, sympa::MODEL_BOUNDED>(op, a, c, b, lr, wd, eps, out, moved, status);
    return -1;
}
}  // namespace

// a, c [b,2,n,n] -> out [b,2,n,n]; moved [b] (op 2, may be null); status bits
extern "C" int sympa_hostsim_expmap(int op, const double* a, const double* c, int64_t b, int n, int model, double lr, double wd,
                                    double eps, double* out, int32_t* moved, int32_t* status) {
    if (op < 0 || op > 2) return -3;
#define CALL(N) case N: return run_n<N>(op, model, a, c, b, lr, wd, eps, out, moved, status);
    switch (n) {
        CALL(1) CALL(2) CALL(3) CALL(4) CALL(5) CALL(6) CALL(7) CALL(8)
        default: return -2;
    }
#undef CALL
}
