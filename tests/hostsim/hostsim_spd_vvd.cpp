// TEST INFRASTRUCTURE ONLY (CPU).  The SPD model's vector-valued distance and its backward (sympa::spd_pair_vvd, sympa_amd/csrc/
// spd_math.hpp; sympa::spd_pair_backward_vvd, spd_math_bwd.hpp) compiled with g++, runtime n = 1..16, next to hostsim.cpp,
// which stays as it is.  Nothing in sympa_amd/ loads this library.
#include <cmath>
#include <cstdint>
#include "../../sympa_amd/csrc/spd_math_bwd.hpp"

// x, y [b,n,n] -> v [b,n] ascending, status bits
extern "C" int sympa_hostsim_spd_vvd_fwd(const double* x, const double* y, int64_t b, int n, double* v, int32_t* status) {
    if (n < 1 || n > sympa::SPD_MAX_N) return -2;
    int st = 0;
    sympa::SpdWork w;
    for (int64_t i = 0; i < b; ++i) sympa::spd_pair_vvd(w, x + i * n * n, y + i * n * n, n, v + i * n, st);
    if (status) *status = st;
    return 0;
}

// x, y [b,n,n], gv [b,n] (cotangent on the ascending v) -> gx, gy [b,n,n], v [b,n] (may be null), status bits
extern "C" int sympa_hostsim_spd_vvd_bwd(const double* x, const double* y, const double* gv, int64_t b, int n, double* gx, double* gy,
                                         double* v, int32_t* status) {
    if (n < 1 || n > sympa::SPD_MAX_N) return -2;
    int st = 0;
    sympa::SpdBwdWork w;
    for (int64_t i = 0; i < b; ++i)
        sympa::spd_pair_backward_vvd(w, x + i * n * n, y + i * n * n, n, gv + i * n, gx + i * n * n, gy + i * n * n,
                                     v ? v + i * n : nullptr, st);
    if (status) *status = st;
    return 0;
}
