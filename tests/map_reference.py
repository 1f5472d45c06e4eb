"""An exact reference for the ranking behind mean average precision (csrc/map_rank.hip, metrics.host_average_precision) and the
seeded cases the CPU and GPU tests share.  Pure Python over fractions.Fraction: no numpy sort, nothing from sympa_amd.metrics.

Rule (include/sympa_hip.h, sympa_map_rows): the columns k != i of row i are ordered by (isnan, value + 0.0, k) -- ascending value,
-0 as +0, NaN after every number, ties by column -- after fp32 keys have rounded every value with np.float32 (IEEE: gradual
underflow, overflow to inf).  With the neighbours (the row's CSR entries other than i) at the 1-based positions r_1 < ... < r_deg of
that order, AP = (1 / deg) sum_t t / r_t as a Fraction; None (NaN) for a row without a neighbour other than itself.

Bound of every comparison (compare()), derived, not measured:  |got - AP| <= (deg + 2) eps64 AP  -- deg correctly rounded
quotients, deg - 1 additions of positive terms in order, one final division.  A row whose neighbours are all the other columns
must be 1.0 exactly.  Every row of every case is compared.

Cases (each a row block [R, ld] of an N-column matrix with its CSR; built once, read-only):
  keys    N = 96, all rows: NaN, +-0, +-inf, 1e39 and 3.5e38 (above FLT_MAX), 1e-40 (fp32 subnormal), +-1e-46 (fp32 zero), pairs
          one fp64 ulp apart, 1 + j 2^-30 (equal in fp32), fp32 half-way points, each planted once among and once outside the
          neighbours of a row; constant and quantised rows; neighbours nearest / farthest / tied with non-neighbours at lower and
          at higher columns; self entries in the CSR; a zero, non-zero or NaN diagonal.
  degrees N = 2600, one block of rows at row_begin = 1111: every degree of DEGREES under three of the five value patterns, LDS and
          wide rows interleaved, wide rows r and r + 16 with the larger degree first and with the smaller first.
  shapes  the streaming pass: N of SHAPE_NS x the first and the last min(N, 6) rows x a 16-byte and an 8-byte aligned base x
          ld in {N, N + 1, N + 3} with -1.0 / NaN in the padding columns.
  wrapper N = 300, square fp32-valued matrix, degrees 0..40 (MeanAveragePrecisionMetric.average_precisions)."""
import functools
import math
from fractions import Fraction

import numpy as np

EPS64 = float(np.finfo(np.float64).eps)
LDS_CAP = 1024                     # SYMPA_MAP_LDS_CAP (tests/test_abi.py pins the header's value; the GPU test asserts it)
DEGREES_N = 2600
DEGREES_ROW_BEGIN = 1111
DEGREES = [0, 1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1026, 2047, 2048, 2049, DEGREES_N - 1]
PATTERNS = ["distinct", "nearest", "farthest", "quantised", "constant"]
SHAPE_NS = [1, 2, 3, 4, 5, 7, 8, 9, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 2050]
NAN, INF = float("nan"), float("inf")


# ---- the reference ---------------------------------------------------------------------------------------------------------
def round_keys(values, fp32):
    """The row as Python floats, through np.float32 first for fp32 keys."""
    v = np.asarray(values, dtype=np.float64)
    if fp32:
        with np.errstate(over="ignore", under="ignore"):
            v = v.astype(np.float32).astype(np.float64)
    return v.tolist()


def reference_ap(values, i, nbrs, fp32):
    """Exact AP (Fraction) of row i with the distances `values` and the neighbour columns `nbrs`; None for no neighbour."""
    v = round_keys(values, fp32)
    nb = set(int(c) for c in nbrs) - {i}
    if not nb:
        return None
    # NaN compares false with everything, so a tuple holding it would not order: its slot is a constant behind the isnan flag
    order = sorted((math.isnan(v[k]), 0.0 if math.isnan(v[k]) else v[k] + 0.0, k) for k in range(len(v)) if k != i)
    total, t = Fraction(0), 0
    for pos, key in enumerate(order, 1):
        if key[2] in nb:
            t += 1
            total += Fraction(t, pos)
    assert t == len(nb), "a neighbour column lies outside the row"
    return total / t


# ---- cases -----------------------------------------------------------------------------------------------------------------
class Case:
    """Rows [row_begin, row_begin + R) of an N-column matrix in `flat` (fp64; the block starts at element `off`, leading
    dimension ld >= N) with the CSR (rowptr int64 [N + 1], cols int32) of all N rows."""

    def __init__(self, name, N, row_begin, block, rowptr, cols, ld=None, off=0, pad=None):
        R = block.shape[0]
        ld = N if ld is None else ld
        flat = np.zeros(off + R * ld, dtype=np.float64)
        view = flat[off:off + R * ld].reshape(R, ld)
        view[:, :N] = block
        if ld > N:
            view[:, N:] = pad
        self.name, self.N, self.row_begin, self.R, self.ld, self.off = name, N, row_begin, R, ld, off
        self.flat, self.rowptr, self.cols = flat, np.asarray(rowptr, dtype=np.int64), np.asarray(cols, dtype=np.int32)
        for a in (self.flat, self.rowptr, self.cols):
            a.flags.writeable = False

    @property
    def rows(self):
        return self.flat[self.off:self.off + self.R * self.ld].reshape(self.R, self.ld)[:, :self.N]

    def nbrs(self, r):
        g = self.row_begin + r
        return self.cols[self.rowptr[g]:self.rowptr[g + 1]]

    def degree(self, r):
        return len(set(self.nbrs(r).tolist()) - {self.row_begin + r})

    @property
    def max_degree(self):
        return int((self.rowptr[1:] - self.rowptr[:-1]).max())


def csr_of_block(N, row_begin, lists):
    """CSR over all N rows: `lists` for the block's rows (each sorted ascending), empty rows elsewhere."""
    rowptr = np.zeros(N + 1, dtype=np.int64)
    counts = np.zeros(N, dtype=np.int64)
    counts[row_begin:row_begin + len(lists)] = [len(x) for x in lists]
    rowptr[1:] = np.cumsum(counts)
    cols = np.concatenate([np.asarray(sorted(x), dtype=np.int32) for x in lists] + [np.zeros(0, dtype=np.int32)])
    return rowptr, cols


def others(N, i):
    return np.array([k for k in range(N) if k != i], dtype=np.int64)


def ranked(values, i, fp32=False):
    """Columns other than i in the order of the rule (the generators' own use: which columns are nearest / farthest)."""
    v = round_keys(values, fp32)
    return [k for _, _, k in sorted((math.isnan(v[k]), 0.0 if math.isnan(v[k]) else v[k] + 0.0, k)
                                    for k in range(len(v)) if k != i)]


def special_keys():
    x = 0.7371
    out = [NAN, 0.0, -0.0, INF, -INF, 1e39, 3.5e38, 1e-40, 1e-46, -1e-46, x, float(np.nextafter(x, 2.0))]
    out += [1.0 + j * 2.0 ** -30 for j in range(4)]                       # distinct in fp64, one value in fp32
    out += [1.0 + j * 2.0 ** -24 + 2.0 ** -25 for j in range(4)]          # between the fp32 grid and its half-way points
    out += [1.0 + (2 * j + 1) * 2.0 ** -24 for j in range(4)]             # exact fp32 half-way points: round to even
    return out


def random_keys(rng, n):
    """Positive and negative values, a part of them fp32 values with fp64 noise below the fp32 ulp (they collapse in fp32)."""
    v = rng.uniform(0.0, 3.0, n)
    neg = rng.random(n) < 0.1
    v[neg] = -v[neg]
    coarse = rng.random(n) < 0.3
    base = rng.choice(np.float32([0.5, 1.5, 2.25, 1.0]).astype(np.float64), n)
    v[coarse] = base[coarse] * (1.0 + rng.integers(0, 64, n)[coarse] * 2.0 ** -40)
    return v


@functools.lru_cache(maxsize=None)
def keys_cases():
    N = 96
    rng = np.random.default_rng(9601)
    spec = special_keys()
    block = np.zeros((N, N))
    lists = []
    for i in range(N):
        oth = others(N, i)
        v = random_keys(rng, N)
        if i < 72:                                                         # every special among and outside the neighbours
            deg = int(rng.integers(len(spec) + 4, 61))
            nb = rng.permutation(oth)[:deg]
            out = np.setdiff1d(oth, nb)
            v[rng.permutation(nb)[:len(spec)]] = spec
            v[rng.permutation(out)[:len(spec)]] = spec
            nb = nb.tolist() + ([i] if i % 8 == 5 else [])                 # a self entry among the others
        elif i < 80:                                                       # neighbours nearest (72..75) / farthest (76..79)
            v[rng.permutation(oth)[:len(spec)]] = spec
            k = [1, 5, 17, 40][i % 4]
            order = ranked(v, i)
            nb = order[:k] if i < 76 else order[-k:]
        elif i < 83:                                                       # constant: some, all others, all others and self
            v[:] = 2.5
            nb = [rng.permutation(oth)[:13].tolist(), oth.tolist(), list(range(N))][i - 80]
        elif i < 86:                                                       # 8 levels (85: 8 fp64 levels that are one fp32 value)
            levels = np.linspace(0.5, 4.0, 8) if i < 85 else 1.0 + np.arange(8) * 2.0 ** -30
            v = levels[rng.integers(0, 8, N)]
            nb = rng.permutation(oth)[:[7, 33, 20][i - 83]].tolist()
        elif i < 89:                                                       # neighbours tied with non-neighbours at lower / higher / both
            lo, mid, hi = np.arange(0, 30), np.arange(33, 63), np.arange(66, 96)
            nb_pool, tie_pool = [(hi, lo), (lo, hi), (mid, np.concatenate((lo, hi)))][i - 86]
            nb = rng.permutation(np.setdiff1d(nb_pool, [i]))[:10].tolist()
            tied = rng.permutation(np.setdiff1d(tie_pool, [i]))[:12]
            v[nb] = 1.25
            v[tied] = 1.25
        elif i == 89:
            nb = []
        elif i == 90:
            nb = [i]                                                       # the CSR holds only the row's own index
        else:                                                              # small degrees over scattered specials
            v[rng.permutation(oth)[:len(spec)]] = spec
            nb = rng.permutation(oth)[:[1, 2, 3, 16, 17][i - 91]].tolist()
        v[i] = [0.0, 7.25, NAN][i % 3] if i < 80 or i > 82 else 2.5        # self: zero, non-zero, NaN
        block[i] = v
        lists.append(nb)
    rowptr, cols = csr_of_block(N, 0, lists)
    return (Case("keys", N, 0, block, rowptr, cols),)


def pattern_row(rng, N, g, deg, pattern):
    oth = others(N, g)
    if pattern == "constant":
        v = np.full(N, 1.75)
    elif pattern == "quantised":
        v = np.linspace(0.25, 2.0, 8)[rng.integers(0, 8, N)]
    else:
        v = (rng.permutation(N) + rng.random(N) * 0.5) * 1e-3              # distinct in fp64
    v[g] = 0.0
    if pattern == "nearest":
        nb = ranked(v, g)[:deg]
    elif pattern == "farthest":
        nb = ranked(v, g)[N - 1 - deg:]
    else:
        nb = rng.permutation(oth)[:deg].tolist()
    assert len(nb) == deg
    return v, nb


@functools.lru_cache(maxsize=None)
def degrees_cases():
    N, b0 = DEGREES_N, DEGREES_ROW_BEGIN
    rng = np.random.default_rng(2600)
    specs = [(deg, PATTERNS[(j + k) % 5], None) for j, deg in enumerate(DEGREES) for k in range(3)]
    specs += [(0, "distinct", "only"), (7, "distinct", "among"), (N - 1, "quantised", "among")]
    specs += [(1100, "quantised", None), (1600, "distinct", None), (3, "distinct", None)]
    specs = [specs[k] for k in rng.permutation(len(specs))]

    def place(at, deg, pattern):                                           # bring a row of this degree to block row `at`
        k = next(k for k, s in enumerate(specs) if s[:2] == (deg, pattern) and s[2] is None and k not in fixed)
        specs[at], specs[k] = specs[k], specs[at]
        fixed.add(at)
    fixed = set()
    # the wide kernel's workgroup 3 ranks rows 3 and 19, workgroup 5 rows 5 and 21: larger degree first, smaller first
    place(3, N - 1, PATTERNS[DEGREES.index(N - 1) % 5]), place(19, 1025, PATTERNS[(DEGREES.index(1025) + 1) % 5])
    place(5, 1026, PATTERNS[DEGREES.index(1026) % 5]), place(21, 2049, PATTERNS[(DEGREES.index(2049) + 2) % 5])
    block = np.zeros((len(specs), N))
    lists = []
    for r, (deg, pattern, self_mode) in enumerate(specs):
        g = b0 + r
        v, nb = pattern_row(rng, N, g, deg, pattern)
        block[r] = v
        lists.append(nb + ([g] if self_mode else []))
    rowptr, cols = csr_of_block(N, b0, lists)
    case = Case("degrees", N, b0, block, rowptr, cols)
    wide = [r for r in range(case.R) if len(case.nbrs(r)) > LDS_CAP]
    assert len(wide) >= 20 and {3, 19, 5, 21} <= set(wide)
    assert len(case.nbrs(3)) > len(case.nbrs(19)) and len(case.nbrs(5)) < len(case.nbrs(21))
    assert any(r + 1 not in wide for r in wide) and any(r - 1 not in wide for r in wide)          # interleaved
    assert sum(len(case.nbrs(r)) == case.max_degree for r in range(case.R)) == 1                    # one longest row (N entries)
    return (case,)


@functools.lru_cache(maxsize=None)
def shapes_cases():
    rng = np.random.default_rng(2050)
    cases = []
    for N in SHAPE_NS:
        R = min(N, 6)
        for b0 in sorted({0, N - R}):
            block = rng.uniform(0.0, 10.0, (R, N))
            lists = []
            for r, deg in enumerate([1, 2, 3, 4, N - 1, 2][:R]):
                g = b0 + r
                block[r, g] = 0.0
                lists.append(rng.permutation(others(N, g))[:min(deg, N - 1)].tolist())
            rowptr, cols = csr_of_block(N, b0, lists)
            for off in (0, 1):                                             # 16-byte / 8-byte aligned base (a [1:] view of the buffer)
                for extra in (0, 1, 3):
                    pad = np.where(np.arange(extra) % 2 == 0, -1.0, NAN)   # smaller / larger than every real key
                    cases.append(Case(f"shapes-N{N}-b{b0}-off{off}-ld+{extra}", N, b0, block, rowptr, cols, ld=N + extra,
                                      off=off, pad=pad))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def wrapper_cases():
    """Square, fp32-valued: what MeanAveragePrecisionMetric.average_precisions takes as a float32 matrix."""
    N = 300
    rng = np.random.default_rng(300)
    block = rng.uniform(0.0, 4.0, (N, N)).astype(np.float32).astype(np.float64)
    block[::5] = np.round(block[::5] * 4) / 4                              # every fifth row quantised: ties
    np.fill_diagonal(block, 0.0)
    lists = [rng.permutation(others(N, i))[:i % 41].tolist() for i in range(N)]
    rowptr, cols = csr_of_block(N, 0, lists)
    return (Case("wrapper", N, 0, block, rowptr, cols),)


FAMILIES = {"keys": keys_cases, "degrees": degrees_cases, "shapes": shapes_cases, "wrapper": wrapper_cases}


@functools.lru_cache(maxsize=None)
def reference(family, fp32):
    """Per case of the family, the exact AP (Fraction or None) of every row of the block.  Computed once, shared."""
    return tuple(tuple(reference_ap(c.rows[r], c.row_begin + r, c.nbrs(r), fp32) for r in range(c.R)) for c in FAMILIES[family]())


# ---- comparison ------------------------------------------------------------------------------------------------------------
def compare(got, case, want):
    """Every row of the block: the NaN pattern, |got - AP| <= (deg + 2) eps64 AP in exact arithmetic, 1.0 exactly when every
    other column is a neighbour.  Returns the worst ratio to the bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (case.R,), (case.name, got.shape)
    worst = 0.0
    for r in range(case.R):
        g, deg, where = float(got[r]), case.degree(r), f"{case.name} row {case.row_begin + r} (block row {r})"
        if want[r] is None:
            assert math.isnan(g), f"{where}: no neighbour, got {g!r} for NaN"
            continue
        assert not math.isnan(g), f"{where}: got NaN for {float(want[r])!r} (degree {deg})"
        assert math.isfinite(g), f"{where}: got {g!r}"
        err, bound = abs(Fraction(g) - want[r]), (deg + 2) * Fraction(EPS64) * want[r]
        assert err <= bound, f"{where}: got {g!r}, exact {float(want[r])!r}, degree {deg}: error {float(err / bound):.3g} of the bound"
        if deg == case.N - 1:
            assert g == 1.0, f"{where}: every other column is a neighbour, got {g!r}"
        worst = max(worst, float(err / bound))
    return worst


def report(family, fp32, worst, what):
    print(f"[map-rank] {what} {family} {'fp32' if fp32 else 'fp64'} keys: worst |got - AP| / ((deg + 2) eps64 AP) = {worst:.3g}",
          flush=True)
