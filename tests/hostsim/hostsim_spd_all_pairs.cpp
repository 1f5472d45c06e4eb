// TEST INFRASTRUCTURE ONLY (CPU).  One entry of the SPD model's all-pairs distance matrix (sympa::spd_pair_metric, sympa_amd/csrc/
// spd_math.hpp: what spd_all_pairs_generic_kernel runs per lane) compiled with g++, runtime n = 1..16, beside
// sympa::spd_pair_distance for the bit-for-bit comparison.  Nothing in sympa_amd/ loads this library.
#include <cmath>
#include <cstdint>
#include "../../sympa_amd/csrc/spd_math.hpp"

// x, y [b,n,n] -> out [b] under metric 0 / 1 / 2 (riem / fone / finf), status bits (or-ed over the batch)
extern "C" int sympa_hostsim_spd_pair_metric(const double* x, const double* y, int64_t b, int n, int metric, double* out, int32_t* status) {
    if (n < 1 || n > sympa::SPD_MAX_N || metric < 0 || metric > 2) return -2;
    int st = 0;
    sympa::SpdWork w;
    for (int64_t i = 0; i < b; ++i) out[i] = sympa::spd_pair_metric(w, x + i * n * n, y + i * n * n, n, metric, st);
    if (status) *status = st;
    return 0;
}

// the same pairs through spd_pair_distance
extern "C" int sympa_hostsim_spd_pair_distance(const double* x, const double* y, int64_t b, int n, double* out, int32_t* status) {
    if (n < 1 || n > sympa::SPD_MAX_N) return -2;
    int st = 0;
    sympa::SpdWork w;
    for (int64_t i = 0; i < b; ++i) out[i] = sympa::spd_pair_distance(w, x + i * n * n, y + i * n * n, n, st);
    if (status) *status = st;
    return 0;
}
