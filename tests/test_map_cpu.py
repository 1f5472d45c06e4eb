"""CPU (`-m "not gpu"`): the mean-average-precision layer of sympa_amd.metrics against the reference's rules
(sympa/metrics.py:25-63): the neighbour CSR, the host restatement of the ranking on the reference's own fixtures
(tests/golden/map_*.npz, tools/make_golden_map.py) and on hand-computed ties, and AverageDistortionMetric."""
import glob
import os
from collections import defaultdict

import numpy as np
import pytest
import torch
from torch.utils.data import TensorDataset

from sympa_amd import data, ops
from sympa_amd.metrics import AverageDistortionMetric, MeanAveragePrecisionMetric, host_average_precision
from tests.helpers import GOLDEN

MAP_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "map_*.npz")))


def reference_neighbors(ids, dists):
    """metrics.py:30-37, restated: the Python loop over every triple."""
    nb = defaultdict(set)
    for (src, dst), d in zip(ids.tolist(), dists.tolist()):
        if d == 1:
            nb[src].add(dst)
            nb[dst].add(src)
    return nb


def csr_as_sets(rowptr, cols):
    rowptr, cols = rowptr.tolist(), cols.tolist()
    return {i: set(cols[rowptr[i]:rowptr[i + 1]]) for i in range(len(rowptr) - 1) if rowptr[i + 1] > rowptr[i]}


@pytest.mark.parametrize("graph", ["grid3d-125", "tree-b3-h6", "margulis-71"])
def test_neighbor_csr_equals_the_reference_rule_on_the_config_graphs(graph):
    trip, _ = data.graph_triplets(data.named_graph(graph))
    ids, dists = trip[:, :2], trip[:, 2].to(torch.float32)       # train.py:93: a float32 distance tensor
    N = int(ids.max()) + 1
    rowptr, cols = ops.neighbor_csr(ids, dists, N)
    assert rowptr.dtype == torch.int64 and cols.dtype == torch.int32 and rowptr.numel() == N + 1
    if graph == "margulis-71":          # 12.7 M triples: the loop over the ones the rule keeps
        keep = dists == 1
        want = reference_neighbors(ids[keep], dists[keep])
    else:
        want = reference_neighbors(ids, dists)
    assert csr_as_sets(rowptr, cols) == dict(want)
    for i in range(N):                  # each row sorted and unique
        row = cols[rowptr[i]:rowptr[i + 1]]
        assert bool((row[1:] > row[:-1]).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_neighbor_csr_collapses_both_directions_and_repeats_and_takes_only_exact_ones(dtype):
    ids = torch.tensor([[0, 1], [1, 0], [0, 1], [2, 3], [3, 4], [4, 5], [5, 0], [2, 5], [6, 6]])
    dists = torch.tensor([1.0, 1.0, 1.0, 2.0, 1.0000001, 1.0, 1.0, 1.0, 1.0], dtype=dtype)
    rowptr, cols = ops.neighbor_csr(ids, dists, 8)
    want = reference_neighbors(ids, dists)
    assert csr_as_sets(rowptr, cols) == dict(want)
    assert want[0] == {1, 5} and 3 not in want[2] and 3 not in want[4] and want[6] == {6}
    m = MeanAveragePrecisionMetric(TensorDataset(ids, dists))
    assert m.neighbors == want
    assert m.max_degree == 3          # node 5: {0, 2, 4}


def test_neighbor_csr_rejects_ids_beyond_the_node_count():
    ids = torch.tensor([[0, 1], [1, 7]])
    with pytest.raises(IndexError):
        ops.neighbor_csr(ids, torch.ones(2), 7)
    with pytest.raises(IndexError):
        MeanAveragePrecisionMetric((ids, torch.ones(2))).calculate_metric(np.zeros((5, 5)))


@pytest.mark.parametrize("sfx", ["", "64"], ids=["float32", "float64"])
@pytest.mark.parametrize("path", MAP_FIXTURES, ids=[os.path.basename(p) for p in MAP_FIXTURES])
def test_host_metric_reproduces_the_reference_on_its_fixture(path, sfx):
    f = np.load(path)
    ids, dists = torch.from_numpy(f["ids"]), torch.from_numpy(f["dists"])
    m = MeanAveragePrecisionMetric(TensorDataset(ids, dists))
    matrix = torch.from_numpy(f["matrix" + sfx])
    assert matrix.dtype == (torch.float32 if sfx == "" else torch.float64)
    ap = m.average_precisions(matrix)
    want = f["ap" + sfx]
    assert np.isfinite(want).all()
    assert np.abs(ap - want).max() <= 1e-14 * np.abs(want).max()
    got = m.calculate_metric(matrix)
    assert abs(got - float(f["map" + sfx])) <= 1e-14 * abs(float(f["map" + sfx]))
    assert m.calculate_metric(f["matrix" + sfx]) == got                  # ndarray in, same answer


def test_fixtures_are_small_and_hold_the_reference_ranks():
    assert len(MAP_FIXTURES) >= 2
    for p in MAP_FIXTURES:
        assert os.path.getsize(p) < 512 * 1024
        f = np.load(p)
        assert len(f["nb_row"]) == len(f["nb_col"]) == len(f["nb_rank"]) > 0
        assert (f["nb_rank"] >= 1).all()


# planted ties: edges (0,2) (0,4) (1,2) (1,3); node 5 isolated
TIE_EDGES = torch.tensor([[0, 2], [0, 4], [1, 2], [1, 3], [2, 3]])
TIE_DISTS = torch.tensor([1.0, 1.0, 1.0, 1.0, 2.0])
NAN = float("nan")
TIE_MATRIX = np.array([
    [0.0, 1.0, 1.0, 0.0, NAN, 10.0],     # sorted: 3 (0.0), 1, 2 (tie at 1.0 by index), 5, 4 (NaN last)
    [-0.0, 0.0, 0.0, 2.0, 1.0, 10.0],    # -0 == +0: 0, 2 (tie by index), 4, 3, 5
    [3.0, 0.0, 0.0, 3.0, 0.0, 10.0],     # self-ties: 1, 4 at distance 0 like self; then 0, 3 (tie), 5
    [NAN, NAN, NAN, 0.0, NAN, 10.0],     # 5, then the NaNs by index: 0, 1, 2, 4
    [5.0, 4.0, 3.0, 2.0, 0.0, 10.0],     # 3, 2, 1, 0, 5
    [1.0, 1.0, 1.0, 1.0, 1.0, 0.0],      # no neighbours
])
# neighbours 0: {2, 4} at positions 3, 5;  1: {2, 3} at 2, 4;  2: {0, 1} at 1, 3;  3: {1} at 3;  4: {0} at 4;  5: none
TIE_AP = np.array([(1 / 3 + 2 / 5) / 2, (1 / 2 + 2 / 4) / 2, (1 / 1 + 2 / 3) / 2, 1 / 3, 1 / 4, NAN])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_restatement_follows_the_stable_tie_rule(dtype):
    m = MeanAveragePrecisionMetric((TIE_EDGES, TIE_DISTS))
    ap = m.average_precisions(TIE_MATRIX.astype(dtype))
    np.testing.assert_allclose(ap[:5], TIE_AP[:5], rtol=1e-15, atol=0)
    assert np.isnan(ap[5])
    assert np.isnan(m.calculate_metric(TIE_MATRIX.astype(dtype)))   # one isolated node: NaN, as np.mean([]) makes it


def test_host_restatement_key_precision_follows_the_matrix_dtype():
    ids, dists = torch.tensor([[0, 1]]), torch.tensor([1.0])
    d = np.array([[0.0, 1.0 + 1e-12, 1.0], [1.0, 0.0, 2.0], [1.0, 2.0, 0.0]])
    m = MeanAveragePrecisionMetric((ids, dists))
    assert m.average_precisions(d)[0] == 0.5                      # fp64 keys: column 2 is closer
    assert m.average_precisions(d.astype(np.float32))[0] == 1.0   # fp32 keys: a tie, broken by column index


def test_host_restatement_reads_self_first_whatever_its_value():
    rowptr = np.array([0, 1, 2])
    cols = np.array([1, 0], dtype=np.int32)
    d = np.array([[5.0, 1.0], [-3.0, 0.0]])
    np.testing.assert_array_equal(host_average_precision(d, rowptr, cols), [1.0, 1.0])


def test_average_distortion_metric_is_the_reference_formula():
    g = torch.Generator().manual_seed(3)
    gd = torch.randint(1, 9, (257, 1), generator=g).to(torch.float64)
    md = torch.rand(257, 1, generator=g, dtype=torch.float64) * 10
    got = AverageDistortionMetric().calculate_metric(gd, md)
    assert torch.equal(got, torch.abs(md - gd) / gd)
