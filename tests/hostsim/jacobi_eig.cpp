// TEST INFRASTRUCTURE ONLY (CPU).  The eigenvalue stage of the dims <= 4 forward kernels on its own:
// herm_eigenvalues_jacobi<N> of sympa_amd/csrc/siegel_math.hpp, compiled with g++, on Hermitian matrices the caller
// supplies (tests/test_jacobi_round_cpu.py).  A library of its own next to hostsim.cpp; nothing in sympa_amd/ loads it.
#include <cstdint>
#include "../../sympa_amd/csrc/siegel_math.hpp"

namespace {
// a: [b, 2, n, n] fp64, real and imaginary plane of a Hermitian matrix (the upper triangle is read); eig: [b, n] in
// the order the iteration leaves them; conv: [b], 1 where the certificate held before the sweep cap
template <int N>
void run(const double* a, int64_t b, double* eig, int32_t* conv) {
    for (int64_t i = 0; i < b; ++i) {
        const double* re = a + i * 2 * N * N;
        const double* im = re + N * N;
        sympa::Herm<N> h;
        for (int j = 0; j < N; ++j) {
            h.d[j] = re[j * N + j];
            for (int k = 0; k < N; ++k) {
                h.re[j][k] = (j < k) ? re[j * N + k] : 0.0;
                h.im[j][k] = (j < k) ? im[j * N + k] : 0.0;
            }
        }
        conv[i] = sympa::herm_eigenvalues_jacobi<N>(h) ? 1 : 0;
        for (int j = 0; j < N; ++j) eig[i * N + j] = h.d[j];
    }
}
}  // namespace

extern "C" int sympa_hostsim_jacobi_eig(const double* a, int64_t b, int n, double* eig, int32_t* conv) {
    switch (n) {
        case 3: run<3>(a, b, eig, conv); return 0;
        case 4: run<4>(a, b, eig, conv); return 0;
        default: return -2;
    }
}
