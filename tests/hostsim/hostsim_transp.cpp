// TEST INFRASTRUCTURE ONLY (CPU).  The parallel transport rows (sympa::transp_exp_row, expmap_transp_row, transp_pair;
// sympa_amd/csrc/siegel_transp_math.hpp) compiled with g++ for dims 1..8 and the upper / bounded models, next to the other
// hostsim libraries, which stay as they are.  Nothing in sympa_amd/ loads this library.
#include <cmath>
#include <cstdint>
#include "../../sympa_amd/csrc/siegel_transp_math.hpp"

namespace {

// op 0: out_v = transp_exp(a, u = c, v);  op 1: the same and out_y = expmap(a, c);  op 2: out_v = transp(a, y = c, v)
template <int N, int MODEL>
int run(int op, const double* a, const double* c, const double* v, int64_t b, double* out_y, double* out_v, int32_t* status) {
    int st = 0;
    constexpr int64_t ROW = 2 * N * N;
    for (int64_t i = 0; i < b; ++i) {
        sympa::CMat<N> x, y, w, ry, rv;
        sympa::load_full<N>(a + i * ROW, x);
        sympa::load_full<N>(c + i * ROW, y);
        sympa::load_full<N>(v + i * ROW, w);
        if (op == 0) {
            sympa::transp_exp_row<N, MODEL>(x, y, w, rv, st);
        } else if (op == 1) {
            sympa::expmap_transp_row<N, MODEL>(x, y, w, ry, rv, st);
            sympa::store_full<N>(out_y + i * ROW, ry);
        } else {
            sympa::transp_pair<N, MODEL>(x, y, w, rv, st);
        }
        sympa::store_full<N>(out_v + i * ROW, rv);
    }
    if (status) *status = st;
    return 0;
}

template <int N>
int run_n(int op, int model, const double* a, const double* c, const double* v, int64_t b, double* out_y, double* out_v,
          int32_t* status) {
    if (model == sympa::MODEL_UPPER) return run<N, sympa::MODEL_UPPER>(op, a, c, v, b, out_y, out_v, status);
    if (model == sympa::MODEL_BOUNDED) return run<N, sympa::MODEL_BOUNDED>(op, a, c, v, b, out_y, out_v, status);
    return -1;
}
}  // namespace

// a, c, v [b,2,n,n] -> out_v [b,2,n,n], out_y [b,2,n,n] (op 1 only); status bits
extern "C" int sympa_hostsim_transp(int op, const double* a, const double* c, const double* v, int64_t b, int n, int model,
                                    double* out_y, double* out_v, int32_t* status) {
    if (op < 0 || op > 2) return -3;
#define CALL(N) case N: return run_n<N>(op, model, a, c, v, b, out_y, out_v, status);
    switch (n) {
        CALL(1) CALL(2) CALL(3) CALL(4) CALL(5) CALL(6) CALL(7) CALL(8)
        default: return -2;
    }
#undef CALL
}
