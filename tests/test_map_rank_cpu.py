"""CPU (`-m "not gpu"`): the exact rational reference of tests/map_reference.py against hand-computed rows, and the numpy
restatement sympa_amd.metrics.host_average_precision against that reference on the keys, degrees, shapes and wrapper cases the GPU
test (tests/test_map_rank_gpu.py) runs through the kernel, with fp64 and with fp32 keys.  This proves the cases and the bound
|got - AP| <= (deg + 2) eps64 AP without the kernel.

Worst |got - AP| / ((deg + 2) eps64 AP) over every row (host_average_precision, x86-64 numpy):
    keys     fp64 0.0615   fp32 0.216
    degrees  fp64 0.188    fp32 0.188
    shapes   fp64 0.2      fp32 0.2
    wrapper  fp64 0.151    fp32 0.151"""
import math
from fractions import Fraction

import numpy as np
import pytest

from sympa_amd.metrics import host_average_precision
from tests import map_reference as mr

NAN = float("nan")


def host_rows(case, fp32):
    """host_average_precision over the block's rows: the block squared up with zero rows, which have no neighbours."""
    dtype = np.float32 if fp32 else np.float64
    d = np.zeros((case.N, case.N), dtype=dtype)
    with np.errstate(over="ignore", under="ignore"):
        d[case.row_begin:case.row_begin + case.R] = case.rows.astype(dtype)
    ap = host_average_precision(d, case.rowptr, case.cols)
    outside = np.ones(case.N, dtype=bool)
    outside[case.row_begin:case.row_begin + case.R] = False
    assert np.isnan(ap[outside]).all()
    return ap[case.row_begin:case.row_begin + case.R]


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("family", ["keys", "degrees", "shapes", "wrapper"])
def test_host_restatement_equals_the_exact_reference_on_every_row(family, fp32):
    worst = 0.0
    for case, want in zip(mr.FAMILIES[family](), mr.reference(family, fp32)):
        worst = max(worst, mr.compare(host_rows(case, fp32), case, want))
    mr.report(family, fp32, worst, "host_average_precision")


def test_reference_reproduces_hand_computed_ties():
    """The rows of tests/test_map_cpu.py::TIE_MATRIX, ranked by hand."""
    rows = [
        ([0.0, 1.0, 1.0, 0.0, NAN, 10.0], [2, 4], Fraction(1, 2) * (Fraction(1, 3) + Fraction(2, 5))),   # 3, 1, 2, 5, 4
        ([-0.0, 0.0, 0.0, 2.0, 1.0, 10.0], [2, 3], Fraction(1, 2) * (Fraction(1, 2) + Fraction(2, 4))),  # 0, 2, 4, 3, 5
        ([3.0, 0.0, 0.0, 3.0, 0.0, 10.0], [0, 1], Fraction(1, 2) * (1 + Fraction(2, 3))),                # 1, 4, 0, 3, 5
        ([NAN, NAN, NAN, 0.0, NAN, 10.0], [1], Fraction(1, 3)),                                          # 5, 0, 1, 2, 4
        ([5.0, 4.0, 3.0, 2.0, 0.0, 10.0], [0], Fraction(1, 4)),                                          # 3, 2, 1, 0, 5
        ([1.0, 1.0, 1.0, 1.0, 1.0, 0.0], [], None),
    ]
    for i, (values, nbrs, want) in enumerate(rows):
        for fp32 in (False, True):
            assert mr.reference_ap(values, i, nbrs, fp32) == want


def test_reference_key_rule_per_width():
    # fp64: column 2 is closer; fp32: a tie, broken by column index
    v = [0.0, 1.0 + 1e-12, 1.0]
    assert mr.reference_ap(v, 0, [1], False) == Fraction(1, 2) and mr.reference_ap(v, 0, [1], True) == 1
    # above FLT_MAX ties a true inf in fp32 only; NaN stays behind both
    v = [0.0, float("inf"), 1e39, NAN, 3.5e38]
    assert mr.reference_ap(v, 0, [1], False) == Fraction(1, 3) and mr.reference_ap(v, 0, [1], True) == 1
    assert mr.reference_ap(v, 0, [3], False) == Fraction(1, 4) and mr.reference_ap(v, 0, [3], True) == Fraction(1, 4)
    # 1e-40 is an fp32 subnormal (stays above 0), 1e-46 an fp32 zero (ties -0 and +0)
    v = [5.0, 1e-46, 1e-40, -0.0, 0.0]
    assert mr.reference_ap(v, 0, [1], False) == Fraction(1, 3) and mr.reference_ap(v, 0, [1], True) == 1
    assert mr.reference_ap(v, 0, [2], False) == Fraction(1, 4) and mr.reference_ap(v, 0, [2], True) == Fraction(1, 4)
    # fp32 half-way points round to even: 1 + 2^-24 -> 1, 1 + 3 * 2^-24 -> 1 + 2^-22
    v = [0.0, 1.0 + 2.0 ** -24, 1.0, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -22]
    assert mr.reference_ap(v, 0, [1], True) == 1 and mr.reference_ap(v, 0, [4], True) == Fraction(1, 4)
    assert mr.reference_ap(v, 0, [1], False) == Fraction(1, 2) and mr.reference_ap(v, 0, [3], True) == Fraction(1, 3)
    # self is left out whatever its value, also as a CSR entry
    assert mr.reference_ap([NAN, 2.0, 1.0], 0, [0, 1], False) == Fraction(1, 2)
    assert mr.reference_ap([7.0, 2.0, 1.0], 0, [0], False) is None


def test_cases_hold_what_they_are_meant_to():
    (keys,) = mr.keys_cases()
    spec = mr.special_keys()
    for r in range(72):                      # every special once among and once outside the neighbours
        nb = set(keys.nbrs(r).tolist()) - {r}
        row = keys.rows[r]
        for s in spec:
            hit = [k for k in range(keys.N) if k != r and (row[k] == s and math.copysign(1, row[k]) == math.copysign(1, s)
                                                           or (math.isnan(s) and math.isnan(row[k])))]
            assert any(k in nb for k in hit) and any(k not in nb for k in hit), (r, s)
    (deg,) = mr.degrees_cases()
    have = {}
    for r in range(deg.R):
        have.setdefault(deg.degree(r), 0)
        have[deg.degree(r)] += 1
    assert all(have.get(d, 0) >= 3 for d in mr.DEGREES)
    assert deg.R * deg.N < deg.N * deg.N and deg.row_begin > 0            # a row block, never the square matrix
    shapes = mr.shapes_cases()
    assert {c.N for c in shapes} == set(mr.SHAPE_NS)
    for c in shapes:
        assert c.R == min(c.N, 6) and c.row_begin in (0, c.N - c.R) and c.ld - c.N in (0, 1, 3) and c.off in (0, 1)
        assert max(c.degree(r) for r in range(c.R)) == c.N - 1
