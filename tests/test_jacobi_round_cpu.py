"""The eigenvalue stage of the dims <= 4 forward (herm_eigenvalues_jacobi<N> of csrc/siegel_math.hpp: for n = 4 whole rounds
of the round-robin order with the cosines deferred, the certificate handing |h_pq|^2 to the finishing sweep) on the CPU build
of the header (tests/hostsim/jacobi_eig.cpp), against numpy.linalg.eigvalsh of the same matrices.

4 096 random Hermitian positive matrices per class, n = 3 and 4:
  generic    H = A^H A, A complex Gaussian;
  graded     H = U diag(lambda) U^H, lambda spaced evenly in the logarithm from 1 down to 1e-6, U Haar unitary;
  clustered  H = U diag(lambda) U^H, lambda = 1, 1 + 1e-10, 0.3 (and 0.3 (1 + 1e-10) for n = 4).
The error is max |lambda_got - lambda_want| / ||H||_2, for the graded class max |lambda_got - lambda_want| / lambda_want.

The bound of each case is four times (two bits for a reordering of roundings) what the iteration measured on these very
matrices BEFORE the round form went in: PARENT below, measured once by running this file as a script against a build of
jacobi_eig.cpp over the header of the commit before (python tests/test_jacobi_round_cpu.py <library>).  In the graded class
the figure is the floor both sides share, not the iteration's: forming U diag(lambda) U^H in fp64 and eigvalsh itself are
accurate to ~1e-16 ||H||, which is ~1e-10 of the smallest eigenvalue."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 4096
CLASSES = ("generic", "graded", "clustered")

# worst error of the parent commit's iteration on the matrices of matrices(n, cls): see the docstring
PARENT = {
    (3, "generic"): 1.281e-15,
    (3, "graded"): 3.619e-10,
    (3, "clustered"): 1.110e-15,
    (4, "generic"): 2.032e-14,
    (4, "graded"): 3.566e-10,
    (4, "clustered"): 1.110e-15,
}
SLACK = 4.0


def _unitary(rng, b, n):
    a = rng.standard_normal((b, n, n)) + 1j * rng.standard_normal((b, n, n))
    q, r = np.linalg.qr(a)
    d = np.diagonal(r, axis1=-2, axis2=-1)
    return q * (d / np.abs(d))[:, None, :]       # Haar: fix the phases of R's diagonal


def matrices(n, cls):
    """[COUNT, n, n] complex Hermitian, the same for every caller."""
    rng = np.random.default_rng(1000 * n + CLASSES.index(cls))
    if cls == "generic":
        a = rng.standard_normal((COUNT, n, n)) + 1j * rng.standard_normal((COUNT, n, n))
        h = np.conj(a.transpose(0, 2, 1)) @ a
    else:
        if cls == "graded":
            lam = 10.0 ** (-6.0 * np.arange(n) / (n - 1))
        else:
            lam = np.array([1.0, 1.0 + 1e-10, 0.3, 0.3 * (1.0 + 1e-10)][:n])
        u = _unitary(rng, COUNT, n)
        perm = np.stack([rng.permutation(n) for _ in range(COUNT)])
        h = (u * lam[perm][:, None, :]) @ np.conj(u.transpose(0, 2, 1))
    return 0.5 * (h + np.conj(h.transpose(0, 2, 1)))


def build_lib():
    """tests/hostsim/jacobi_eig.cpp over the tree's header, built on demand with g++ (as helpers.hostsim does)."""
    d = os.path.join(ROOT, "tests", "hostsim")
    so = os.path.join(d, "libsympa_jacobi_eig.so")
    srcs = [os.path.join(d, "jacobi_eig.cpp"), os.path.join(ROOT, "sympa_amd", "csrc", "siegel_math.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, srcs[0]], cwd=d)
    return so


def jacobi_eig(lib, h):
    b, n, _ = h.shape
    a = np.ascontiguousarray(np.stack((h.real, h.imag), 1), dtype=np.float64)
    eig = np.zeros((b, n))
    conv = np.zeros(b, np.int32)
    P = ctypes.c_void_p
    rc = lib.sympa_hostsim_jacobi_eig(P(a.ctypes.data), ctypes.c_int64(b), n, P(eig.ctypes.data), P(conv.ctypes.data))
    assert rc == 0, rc
    return np.sort(eig, axis=1), conv


def worst_error(lib, n, cls):
    h = matrices(n, cls)
    want = np.linalg.eigvalsh(h)
    got, conv = jacobi_eig(lib, h)
    assert conv.all(), f"{int((conv == 0).sum())} matrices hit the sweep cap"
    assert np.isfinite(got).all()
    scale = want if cls == "graded" else np.abs(want).max(axis=1, keepdims=True)
    return float((np.abs(got - want) / scale).max())


@pytest.fixture(scope="module")
def lib():
    return ctypes.CDLL(build_lib())


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("n", [3, 4])
def test_eigenvalues_within_four_times_the_parent(lib, n, cls):
    err = worst_error(lib, n, cls)
    bound = SLACK * PARENT[(n, cls)]
    print(f"n = {n} {cls}: worst error {err:.3e}, parent {PARENT[(n, cls)]:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_classes_are_what_they_say():
    for n in (3, 4):
        w = np.linalg.eigvalsh(matrices(n, "graded"))
        assert np.allclose(w[:, 0] / w[:, -1], 1e-6, rtol=1e-6)
        w = np.linalg.eigvalsh(matrices(n, "clustered"))
        assert np.allclose((w[:, -1] - w[:, -2]) / w[:, -1], 1e-10, rtol=1e-3)
        assert (np.linalg.eigvalsh(matrices(n, "generic")) > 0).all()


if __name__ == "__main__":
    the_lib = ctypes.CDLL(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else build_lib())
    for nn in (3, 4):
        for c in CLASSES:
            print(f"    ({nn}, \"{c}\"): {worst_error(the_lib, nn, c):.3e},")
