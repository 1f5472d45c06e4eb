// g++ build of the spd exponential map, logarithm, geodesic and geodesic RSGD row (sympa_amd/csrc/spd_expmap_math.hpp, DESIGN.md
// section 28) for the CPU tests: the rows one after the other, as the kernels of sympa_amd/csrc/spd_expmap.hip run them one per lane.
#include <cstdint>

#include "../../sympa_amd/csrc/spd_expmap_math.hpp"

extern "C" {

// kind: 0 expmap (p2 = u), 1 logmap (p2 = y), 2 geodesic (p2 = y, parameter t).  status: the or of the rows' status bits;
// bad_rows: rows with a bit set.
int sympa_hostsim_spd_map(int kind, const double* x, const double* p2, double t, int64_t b, int n, double* out, int32_t* status,
                          int32_t* bad_rows) {
    if (n < 1 || n > sympa::SPD_MAX_N) return -2;
    if (kind < 0 || kind > 2) return -1;
    static thread_local sympa::SpdExpWork w;
    int st_all = 0, bad = 0;
    for (int64_t i = 0; i < b; ++i) {
        int st = 0;
        sympa::spd_map_row(w, kind, x + i * n * n, p2 + i * n * n, t, n, out + i * n * n, st);
        st_all |= st;
        bad += st != 0;
    }
    if (status != nullptr) *status = st_all;
    if (bad_rows != nullptr) *bad_rows = bad;
    return 0;
}

// x [b, n, n] is updated in place, like the kernel's table
int sympa_hostsim_spd_rsgd_exp(double* x, const double* g, int64_t b, int n, double lr, double wd, double coef, int32_t* status,
                               int32_t* bad_rows) {
    if (n < 1 || n > sympa::SPD_MAX_N) return -2;
    static thread_local sympa::SpdExpWork w;
    double xs[sympa::SPD_MAX_N * sympa::SPD_MAX_N];
    int st_all = 0, bad = 0;
    for (int64_t i = 0; i < b; ++i) {
        int st = 0;
        sympa::spd_row_rsgd_exp(w, xs, x + i * n * n, g + i * n * n, n, lr, wd, coef, st);
        st_all |= st;
        bad += st != 0;
    }
    if (status != nullptr) *status = st_all;
    if (bad_rows != nullptr) *bad_rows = bad;
    return 0;
}

}  // extern "C"
