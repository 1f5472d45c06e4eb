"""GPU: csrc/map_rank.hip (ops.map_rows, MeanAveragePrecisionMetric) against the exact rational reference of
tests/map_reference.py on the cases tests/test_map_rank_cpu.py proves on the host: the key rule with fp64 and with fp32 keys,
every degree class of the LDS and of the workspace kernel in one call, the streaming pass at every head / trip / tail length,
alignment and leading dimension; call splitting and workspace reuse bit for bit; the error contract of include/sympa_hip.h.

Bound of every row: |got - AP| <= (deg + 2) eps64 AP (map_reference.compare).  Worst ratio to it over every row, MI355X:
    keys     fp64 0.0645   fp32 0.216
    degrees  fp64 0.188    fp32 0.188
    shapes   fp64 0.2      fp32 0.2
    wrapper  from_csr (degrees, fp64) 0.188   fp32 slabs of 1 and of 7 rows 0.151   csr(N > num_nodes, fp64) 0.142

Not covered: more than 65 536 rows in one call (the LDS kernel's grid-stride loop).  row_count <= num_rows <= ld makes the
smallest such matrix 34 GB."""
import numpy as np
import pytest
import torch

from sympa_amd import ops
from sympa_amd.metrics import MeanAveragePrecisionMetric
from tests import map_reference as mr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -7.0


def device_block(case):
    """(the whole buffer, the [R, N] view of the block inside it with leading dimension ld) on the device."""
    flat = torch.tensor(case.flat, device=DEV)
    rows = flat[case.off:case.off + case.R * case.ld].view(case.R, case.ld)[:, :case.N]
    assert rows.data_ptr() % 16 == 8 * case.off
    return flat, rows


def device_csr(case):
    return torch.tensor(case.rowptr, device=DEV), torch.tensor(case.cols, device=DEV)


def run(case, rows, nbrs, float32, max_degree=None, chunk=None, workspace=None):
    """ops.map_rows over the block in calls of `chunk` rows (one call by default) into a sentinel-filled out."""
    out = torch.full((case.R,), SENTINEL, dtype=torch.float64, device=DEV)
    chunk = case.R if chunk is None else chunk
    max_degree = case.max_degree if max_degree is None else max_degree
    for b in range(0, case.R, chunk):
        ops.map_rows(rows[b:b + chunk], case.row_begin + b, nbrs, float32=float32, out=out[b:b + chunk], workspace=workspace,
                     max_degree=max_degree)
    got = out.cpu().numpy()
    assert not (got == SENTINEL).any(), f"{case.name}: rows {np.flatnonzero(got == SENTINEL).tolist()} were not written"
    return got


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def status_words():
    return ops._status_buf(DEV).tolist()


@pytest.fixture(autouse=True)
def clean_status():
    ops._status_buf(DEV).zero_()
    yield
    ops._status_buf(DEV).zero_()


# ---- the reference comparison ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("float32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("family", ["keys", "degrees", "shapes"])
def test_kernel_equals_the_exact_reference_on_every_row(family, float32):
    assert ops.MAP_LDS_CAP == mr.LDS_CAP
    worst = 0.0
    for case, want in zip(mr.FAMILIES[family](), mr.reference(family, float32)):
        flat, rows = device_block(case)
        got = run(case, rows, device_csr(case), float32)
        worst = max(worst, mr.compare(got, case, want))
        assert same_bits(flat.cpu().numpy(), case.flat), f"{case.name}: the distance buffer (padding included) changed"
    assert ops.check_status(DEV) == (0, 0)
    mr.report(family, float32, worst, "ops.map_rows")


# ---- call splitting ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("float32", [False, True], ids=["fp64", "fp32"])
def test_split_calls_and_a_reused_workspace_give_the_same_bits(float32):
    (case,) = mr.degrees_cases()
    _, rows = device_block(case)
    nbrs = device_csr(case)
    whole = run(case, rows, nbrs, float32)
    mr.compare(whole, case, mr.reference("degrees", float32)[0])
    need = ops.map_workspace_bytes(case.N, case.max_degree)
    assert need > 0
    for chunk in (1, 15, 16, 17, case.R):
        assert same_bits(run(case, rows, nbrs, float32, chunk=chunk), whole), f"calls of {chunk} rows"
        # the caller's workspace, never cleared between the calls and full of stale words before the first
        ws = torch.full((need // 4,), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
        assert same_bits(run(case, rows, nbrs, float32, chunk=chunk, workspace=ws), whole), f"calls of {chunk} rows, one workspace"
    assert ops.check_status(DEV) == (0, 0)


# ---- the error contract ------------------------------------------------------------------------------------------------------
def lds_and_wide_row(case, clean):
    """An LDS row and a wide row whose clean AP is not the trivial 1.0."""
    lens = [len(case.nbrs(r)) for r in range(case.R)]
    lds = next(r for r, n in enumerate(lens) if 8 <= n <= mr.LDS_CAP and clean[r] < 1.0)
    wide = next(r for r, n in enumerate(lens) if mr.LDS_CAP + 1 < n < case.max_degree and clean[r] < 1.0)
    return lds, wide


@pytest.mark.parametrize("float32", [False, True], ids=["fp64", "fp32"])
def test_out_of_range_entries_make_their_rows_nan_and_leave_the_rest(float32):
    (case,) = mr.degrees_cases()
    _, rows = device_block(case)
    rowptr, cols = device_csr(case)
    clean = run(case, rows, (rowptr, cols), float32)
    assert ops.check_status(DEV) == (0, 0)
    lds, wide = lds_and_wide_row(case, clean)
    assert not np.isnan(clean[[lds, wide]]).any()
    bad = cols.clone()
    bad[int(case.rowptr[case.row_begin + lds]) + 3] = case.N                 # one past the last column
    bad[int(case.rowptr[case.row_begin + wide + 1]) - 2] = -1
    got = run(case, rows, (rowptr, bad), float32)
    assert status_words() == [ops.ST_BAD_INDEX, 2]
    print(f"[map-rank] planted rows: clean {clean[[lds, wide]].tolist()}, with a bad entry {got[[lds, wide]].tolist()}", flush=True)
    assert np.isnan(got[lds]) and np.isnan(got[wide])
    keep = np.ones(case.R, dtype=bool)
    keep[[lds, wide]] = False
    assert same_bits(got[keep], clean[keep])
    with pytest.raises(IndexError):
        ops.check_status(DEV)
    assert ops.check_status(DEV) == (0, 0)


@pytest.mark.parametrize("family", ["keys", "degrees"], ids=["lds", "wide"])
def test_a_row_longer_than_max_degree_is_nan_and_flagged(family):
    (case,) = mr.FAMILIES[family]()
    _, rows = device_block(case)
    nbrs = device_csr(case)
    clean = run(case, rows, nbrs, False)
    longest = [r for r in range(case.R) if len(case.nbrs(r)) == case.max_degree]
    assert len(longest) == 1 and not np.isnan(clean[longest[0]])
    got = run(case, rows, nbrs, False, max_degree=case.max_degree - 1)
    assert status_words() == [ops.ST_BAD_INDEX, 1]
    assert np.isnan(got[longest[0]])
    keep = np.arange(case.R) != longest[0]
    assert same_bits(got[keep], clean[keep])
    with pytest.raises(IndexError):
        ops.check_status(DEV)
    assert ops.check_status(DEV) == (0, 0)


def test_a_rowptr_that_decreases_across_a_row_is_nan_and_flagged():
    """The last row of the block: rowptr steps back by one across it, every offset still inside cols."""
    (case,) = mr.degrees_cases()
    _, rows = device_block(case)
    rowptr, cols = device_csr(case)
    clean = run(case, rows, (rowptr, cols), False)
    last = case.row_begin + case.R - 1
    assert case.rowptr[last] >= 1
    bent = rowptr.clone()
    bent[last + 1] = bent[last] - 1
    assert 0 <= int(bent.min()) and int(bent.max()) <= cols.numel()
    got = run(case, rows, (bent, cols), False)
    assert status_words() == [ops.ST_BAD_INDEX, 1]
    assert np.isnan(got[-1]) and same_bits(got[:-1], clean[:-1])
    with pytest.raises(IndexError):
        ops.check_status(DEV)
    assert ops.check_status(DEV) == (0, 0)


# ---- MeanAveragePrecisionMetric ------------------------------------------------------------------------------------------------
def test_from_csr_ranks_the_degrees_rows_inside_a_square_matrix():
    (case,) = mr.degrees_cases()
    metric = MeanAveragePrecisionMetric.from_csr(*device_csr(case))
    assert metric.num_nodes == case.N and metric.max_degree == case.max_degree
    d = torch.zeros(case.N, case.N, dtype=torch.float64, device=DEV)
    d[case.row_begin:case.row_begin + case.R] = torch.from_numpy(np.ascontiguousarray(case.rows)).to(DEV)
    ap = metric.average_precisions(d).cpu().numpy()
    assert ops.check_status(DEV) == (0, 0)
    block = slice(case.row_begin, case.row_begin + case.R)
    worst = mr.compare(ap[block], case, mr.reference("degrees", False)[0])
    outside = np.ones(case.N, dtype=bool)
    outside[block] = False
    assert np.isnan(ap[outside]).all()                                      # rows without neighbours
    mr.report("degrees", False, worst, "from_csr + average_precisions")


@pytest.mark.parametrize("slab_rows", [1, 7])
def test_average_precisions_of_an_fp32_matrix_in_ragged_slabs(slab_rows):
    (case,) = mr.wrapper_cases()
    assert case.N % 7 != 0
    metric = MeanAveragePrecisionMetric.from_csr(*device_csr(case))
    d32 = torch.from_numpy(case.rows.astype(np.float32)).to(DEV)
    ap = metric.average_precisions(d32, max_block_bytes=slab_rows * 8 * case.N).cpu().numpy()
    assert ops.check_status(DEV) == (0, 0)
    worst = mr.compare(ap, case, mr.reference("wrapper", True)[0])
    mr.report("wrapper", True, worst, f"average_precisions, slabs of {slab_rows}")


def test_csr_for_more_rows_than_nodes_gives_nan_for_the_trailing_rows():
    (case,) = mr.wrapper_cases()
    extra = 10
    N = case.N + extra
    metric = MeanAveragePrecisionMetric.from_csr(*device_csr(case))
    rowptr, cols = metric.csr(N, DEV)
    assert rowptr.numel() == N + 1 and bool((rowptr[case.N:] == rowptr[case.N]).all()) and cols.numel() == case.cols.size
    rng = np.random.default_rng(310)
    block = rng.uniform(0.0, 4.0, (N, N))
    np.fill_diagonal(block, 0.0)
    wider = mr.Case("wrapper+10", N, 0, block, rowptr.cpu().numpy(), cols.cpu().numpy())
    want = tuple(mr.reference_ap(wider.rows[r], r, wider.nbrs(r), False) for r in range(N))
    assert all(w is None for w in want[case.N:])
    ap = metric.average_precisions(torch.from_numpy(block).to(DEV)).cpu().numpy()
    assert ops.check_status(DEV) == (0, 0)
    assert np.isnan(ap[case.N:]).all()
    worst = mr.compare(ap, wider, want)
    mr.report("wrapper", False, worst, "average_precisions, csr(N > num_nodes)")
