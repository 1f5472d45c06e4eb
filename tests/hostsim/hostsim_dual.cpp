// TEST INFRASTRUCTURE ONLY (CPU).  The compact dual model's arithmetic (sympa_amd/csrc/*_math*.hpp, MODEL_DUAL) compiled with g++,
// next to hostsim.cpp, which stays as it is: forward (templated dims 1..8 and runtime-n dims 1..16), packed forward, backward and
// the table rows.  Nothing in sympa_amd/ loads this library.
#include <cmath>
#include <cstdint>
#include "../../sympa_amd/csrc/siegel_math.hpp"
#include "../../sympa_amd/csrc/siegel_math_bwd.hpp"
#include "../../sympa_amd/csrc/siegel_table_math.hpp"
#include "../../sympa_amd/csrc/siegel_math_generic.hpp"

namespace {
constexpr int DUAL = sympa::MODEL_DUAL;

template <int N>
int run(const double* z1, const double* z2, int64_t b, int metric, const double* w, double eps, double* out, double* vvd,
        int32_t* status) {
    int st = 0;
    for (int64_t i = 0; i < b; ++i)
        out[i] = sympa::pair_distance<N, DUAL>(z1 + i * 2 * N * N, z2 + i * 2 * N * N, metric, w, 1.0 / eps,
                                               vvd ? vvd + i * N : nullptr, st);
    if (status) *status = st;
    return 0;
}

template <int N>
int run_packed(const double* z1, const double* z2, int64_t b, int metric, const double* w, double eps, double* out,
               int32_t* status) {
    int st = 0;
    for (int64_t i = 0; i < b; ++i) {
        sympa::CMat<N> a, c, e;
        sympa::load_point<N>(z1 + i * 2 * N * N, a);
        sympa::load_point<N>(z2 + i * 2 * N * N, c);
        double p1[sympa::PointPack<N, DUAL>::LEN], p2[sympa::PointPack<N, DUAL>::LEN];
        const bool ok1 = sympa::pack_point<N, DUAL>(a, p1);
        const bool ok2 = sympa::pack_point<N, DUAL>(c, p2);
        sympa::e_from_packed<N, DUAL>(p1, p2, e);
        out[i] = sympa::distance_from_e<N, DUAL>(e, ok1 && ok2, metric, w, 1.0 / eps, nullptr, st);
    }
    if (status) *status = st;
    return 0;
}

template <int N>
int run_bwd(const double* z1, const double* z2, const double* go, int64_t b, int metric, const double* w, double eps,
            double* out, double* g1, double* g2, double* gw, int32_t* status) {
    int st = 0;
    double gwacc[N];
    for (int k = 0; k < N; ++k) gwacc[k] = 0.0;
    for (int64_t i = 0; i < b; ++i) {
        sympa::CMat<N> a, c, ga, gc;
        sympa::load_point<N>(z1 + i * 2 * N * N, a);
        sympa::load_point<N>(z2 + i * 2 * N * N, c);
        out[i] = sympa::pair_backward<N, DUAL>(a, c, metric, w, 1.0 / eps, go[i], ga, gc, gwacc, st);
        sympa::store_full<N>(g1 + i * 2 * N * N, ga);
        sympa::store_full<N>(g2 + i * 2 * N * N, gc);
    }
    for (int k = 0; k < N; ++k) gw[k] = gwacc[k];
    if (status) *status = st;
    return 0;
}

template <int N>
int run_table(int op, const double* z, const double* g, double* out, int64_t b, double lr, double wd, double eps,
              int32_t* projected) {
    int st = 0, moved = 0;
    for (int64_t i = 0; i < b; ++i) {
        sympa::CMat<N> a, gg, r;
        sympa::load_full<N>(z + i * 2 * N * N, a);
        if (g) sympa::load_full<N>(g + i * 2 * N * N, gg);
        if (op == 2) {
            sympa::egrad2rgrad<N, DUAL>(a, gg, r);
            sympa::store_full<N>(out + i * 2 * N * N, r);
        } else {
            const bool m = (op == 0) ? sympa::projx<N, DUAL>(a, eps, st) : sympa::rsgd_row<N, DUAL>(a, gg, lr, wd, eps, st);
            moved += m ? 1 : 0;
            sympa::store_full<N>(out + i * 2 * N * N, a);
        }
    }
    if (projected) *projected = moved;
    return st;
}
}  // namespace

#define SYMPA_DIMS_1_8(CALL) \
    switch (n) { \
        case 1: return CALL(1); case 2: return CALL(2); case 3: return CALL(3); case 4: return CALL(4); \
        case 5: return CALL(5); case 6: return CALL(6); case 7: return CALL(7); case 8: return CALL(8); \
        default: return -2; \
    }

extern "C" int sympa_hostsim_dual_dist(const double* z1, const double* z2, int64_t b, int n, int metric, const double* w,
                                       double eps, double* out, double* vvd, int32_t* status) {
#define CALL(N) run<N>(z1, z2, b, metric, w, eps, out, vvd, status)
    SYMPA_DIMS_1_8(CALL)
#undef CALL
}

extern "C" int sympa_hostsim_dual_dist_packed(const double* z1, const double* z2, int64_t b, int n, int metric, const double* w,
                                              double eps, double* out, int32_t* status) {
#define CALL(N) run_packed<N>(z1, z2, b, metric, w, eps, out, status)
    SYMPA_DIMS_1_8(CALL)
#undef CALL
}

extern "C" int sympa_hostsim_dual_dist_generic(const double* z1, const double* z2, int64_t b, int n, int metric, const double* w,
                                               double eps, double* out, double* vvd, int32_t* status) {
    if (n < 1 || n > sympa::GENERIC_MAX_N) return -2;
    int st = 0;
    sympa::GenericWork work;
    for (int64_t i = 0; i < b; ++i)
        out[i] = sympa::pair_distance_generic(work, z1 + i * 2 * n * n, z2 + i * 2 * n * n, n, DUAL, metric, w, 1.0 / eps,
                                              vvd ? vvd + i * n : nullptr, st);
    if (status) *status = st;
    return 0;
}

extern "C" int sympa_hostsim_dual_dist_bwd(const double* z1, const double* z2, const double* go, int64_t b, int n, int metric,
                                           const double* w, double eps, double* out, double* g1, double* g2, double* gw,
                                           int32_t* status) {
#define CALL(N) run_bwd<N>(z1, z2, go, b, metric, w, eps, out, g1, g2, gw, status)
    SYMPA_DIMS_1_8(CALL)
#undef CALL
}

// op: 0 projx, 1 rsgd step (out = new rows), 2 egrad2rgrad
extern "C" int sympa_hostsim_dual_table(int op, int n, const double* z, const double* g, double* out, int64_t b, double lr,
                                        double wd, double eps, int32_t* projected) {
#define CALL(N) run_table<N>(op, z, g, out, b, lr, wd, eps, projected)
    SYMPA_DIMS_1_8(CALL)
#undef CALL
}

// the fp64 arctangent primitive by itself
extern "C" void sympa_hostsim_dual_atan2(const double* s, const double* c, int64_t b, double* out) {
    for (int64_t i = 0; i < b; ++i) out[i] = sympa::d_atan2_pos(s[i], c[i]);
}
