"""The corners of the joint rotation parameters of the n = 4 round (jacobi_round_angles of csrc/siegel_math.hpp: one reciprocal
square root of P = C_A C_B = 4 cos^2 A cos^2 B serves both rotations of a round) on the CPU build of the header
(tests/hostsim/jacobi_eig.cpp, the library of tests/test_jacobi_round_cpu.py), against numpy.linalg.eigvalsh of the same
matrices.  Error: max |lambda_got - lambda_want| / ||H||_2.

  zero        the zero matrix: every guard is active (beta = delta = 0 on every pivot).  Exact zeros, conv set.
  diagonal    beta = 0 on every pivot, C_A = C_B = 2 (P = 4): the eigenvalues come back bit for bit.
  equal       H = d I + B, B Hermitian with zero diagonal: delta = 0 on every pivot of the first round, 45 degrees, C = 1.
  mixed       diag(x, y) (+) [[d, b], [conj b, d]] and its images under the index permutations that put the two pivots into
              each of the three rounds, either way round: one pivot of the round has delta = 0 (C = 1), the other beta = 0
              (C = 2).  Among them x = y: that pivot has beta = delta = 0.
  up, down    the generic class of test_jacobi_round_cpu.matrices(4, .), its first 256 matrices, times 2^400 and 2^-400 (exact
              scalings): the arguments of the two per-rotation reciprocal square roots move by 2^+-800, P stays in [1, 4].
  up300, down300   the same matrices times 2^300 and 2^-300, inside the range of the commit before (below).

The zero and diagonal cases are exact conditions.  The bound of every other case is four times (two bits for a reordering of
roundings, the rule of test_jacobi_round_cpu.py) what the iteration measured on these very matrices BEFORE the joint form went
in: PARENT below, measured once by running this file as a script against a build of jacobi_eig.cpp over the header of the
commit before (python tests/test_jacobi_joint_angle_cpu.py <library>).

The case `up` has no figure of its own on the commit before: at 2^400 that header returns NaN for all 256 matrices, and not
because of its rounds.  Its finishing shift formed a^2 * delta first, a cubic in ||H|| (||H|| ~ 30 * 2^400 = 8e121, a^2 ~ 1e-10
delta^2 after three sweeps: ~1e356, past the fp64 range; from ||H|| ~ 1e103 on).  The mirror image is its figure of `down`, 2.3e-9:
there a^2 * delta underflowed to zero and the shift was dropped.  The finishing shift now forms a^2 * (delta / (delta^2 + a^2))
(jacobi_diag_update), which has neither limit.  The scaling by 2^400 is exact and nothing in the iteration may see it, so the
reference for `up` is what the commit before gives on the very same matrices where it is in range, unscaled and at 2^+-300: 1.355e-15
in all three, digit for digit, and the bound is four times that as everywhere else.  up300 and down300 pin that band."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_jacobi_round_cpu import build_lib, jacobi_eig, matrices  # noqa: E402

MEASURED = ("equal", "mixed", "up", "down", "up300", "down300")
# worst error of the parent commit's iteration (two reciprocal square roots per rotation) on the matrices of cases(): see the
# docstring
PARENT = {
    "equal": 1.221e-15,
    "mixed": 8.147e-16,
    "up": 1.355e-15,              # the parent's figure on the same matrices inside its range (docstring); NaN at 2^400 itself
    "down": 2.318e-09,
    "up300": 1.355e-15,
    "down300": 1.355e-15,
}
SLACK = 4.0
SCALED = 256

# the pairs of pivots of the three rounds of the round-robin order, A then B
ROUNDS = (((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2)))


def diagonal_matrices():
    rng = np.random.default_rng(41)
    d = rng.standard_normal((64, 4)) * 10.0 ** rng.integers(-3, 4, (64, 4))
    d[:8, 1] = d[:8, 0]              # repeated entries: delta = 0 as well on that pivot
    d[8:12, :] = d[8:12, :1]         # a multiple of the identity
    d[12:16, 2] = 0.0
    d[16:20] = np.abs(d[16:20])
    h = np.zeros((64, 4, 4), complex)
    h[:, range(4), range(4)] = d
    return h


def equal_diagonal_matrices():
    rng = np.random.default_rng(42)
    b = rng.standard_normal((256, 4, 4)) + 1j * rng.standard_normal((256, 4, 4))
    b[:32] = np.exp(1j * np.angle(b[:32]))                          # equal moduli
    b[32:64] = np.abs(b[32:64])                                     # real
    b = np.triu(b, 1)
    b = b + np.conj(b.transpose(0, 2, 1))
    d = np.repeat(np.array([0.0, 1.0, -3.5, 1e3]), 64)
    return b + d[:, None, None] * np.eye(4)


def mixed_matrices():
    rng = np.random.default_rng(43)
    out = []
    for k in range(32):
        x, y, d = rng.standard_normal(3) * 10.0 ** rng.integers(-2, 3, 3)
        if k < 8:
            y = x                                                   # the beta = 0 pivot has delta = 0 as well
        b = (rng.standard_normal() + 1j * rng.standard_normal()) * 10.0 ** rng.integers(-2, 3)
        for first, second in itertools.chain(ROUNDS, [(s, f) for f, s in ROUNDS]):
            h = np.zeros((4, 4), complex)
            (i, j), (p, q) = first, second                          # (i, j): beta = 0;  (p, q): delta = 0
            h[i, i], h[j, j] = x, y
            h[p, p] = h[q, q] = d
            h[p, q], h[q, p] = b, np.conj(b)
            out.append(h)
    return np.stack(out)


def cases(name):
    """[count, 4, 4] complex Hermitian, the same for every caller."""
    if name == "zero":
        return np.zeros((3, 4, 4), complex)
    if name == "diagonal":
        return diagonal_matrices()
    if name == "equal":
        return equal_diagonal_matrices()
    if name == "mixed":
        return mixed_matrices()
    return matrices(4, "generic")[:SCALED] * 2.0 ** {"up": 400, "down": -400, "up300": 300, "down300": -300}[name]


def worst_error(lib, name):
    h = cases(name)
    want = np.linalg.eigvalsh(h)
    got, conv = jacobi_eig(lib, h)
    assert conv.all(), f"{int((conv == 0).sum())} matrices hit the sweep cap"
    assert np.isfinite(got).all()
    return float((np.abs(got - want) / np.abs(want).max(axis=1, keepdims=True)).max())


@pytest.fixture(scope="module")
def lib():
    return ctypes.CDLL(build_lib())


def test_zero_matrix_gives_exact_zeros(lib):
    got, conv = jacobi_eig(lib, cases("zero"))
    assert conv.all()
    assert np.isfinite(got).all() and (got == 0.0).all()


def test_diagonal_matrices_come_back_bit_for_bit(lib):
    h = cases("diagonal")
    got, conv = jacobi_eig(lib, h)
    assert conv.all()
    want = np.sort(np.diagonal(h, axis1=1, axis2=2).real, axis=1)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", MEASURED)
def test_corner_within_four_times_the_parent(lib, name):
    err = worst_error(lib, name)
    bound = SLACK * PARENT[name]
    print(f"{name}: worst error {err:.3e}, parent {PARENT[name]:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_cases_are_what_they_say():
    h = cases("equal")
    assert (np.diagonal(h, axis1=1, axis2=2) == np.diagonal(h, axis1=1, axis2=2)[:, :1]).all()
    assert (np.abs(h[:, 0, 1]) > 0).all() and (np.abs(h[:, 2, 3]) > 0).all()
    assert np.allclose(np.abs(h[:32][:, np.triu_indices(4, 1)[0], np.triu_indices(4, 1)[1]]), 1.0, rtol=1e-15)
    h = cases("mixed")
    assert h.shape[0] == 32 * 6
    for k, (first, second) in enumerate(itertools.chain(ROUNDS, [(s, f) for f, s in ROUNDS])):
        m = h[k::6]
        (i, j), (p, q) = first, second
        assert (m[:, i, j] == 0).all() and (m[:, p, p] == m[:, q, q]).all() and (np.abs(m[:, p, q]) > 0).all()
        assert sorted((i, j, p, q)) == [0, 1, 2, 3]
    assert np.array_equal(cases("up") * 2.0 ** -800, cases("down"))        # exact scalings of the same matrices


if __name__ == "__main__":
    the_lib = ctypes.CDLL(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else build_lib())
    for c in MEASURED:
        try:
            print(f"    \"{c}\": {worst_error(the_lib, c):.3e},")
        except AssertionError as e:
            print(f"    \"{c}\": no figure ({e or 'non-finite eigenvalues'})")
