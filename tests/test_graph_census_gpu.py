"""GPU: the census, ball-size and ball-selection kernels of csrc/graph_census.hip (ops.graph_hop_census_rows,
graph_ball_count_rows, graph_ball_select_rows), GraphDistances.census / radius_for_fraction / ball_sizes / sample_ball_pairs and
ScaledGraphDistances built on them, and tools/train_siegel.py --subsample / --scale_triplets -- against the numpy restatements
(graph.host_hop_census / host_ball_counts / host_ball_select) and the listed triplets.  Every comparison of counts, columns and
distances is exact.  Reference: train.py:86-93, sympa/utils.py:71-102."""
import functools
import os
import re
import sys

import networkx as nx
import numpy as np
import pytest
import torch

from sympa_amd import data, ops
from sympa_amd.graph import (GraphDistances, ScaledGraphDistances, WeightedGraphDistances, graph_csr, host_ball_counts,
                             host_ball_select, host_hop_census, host_hop_rows)
from tests import graph_weighted_cases as wc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
BIG = "product-cartesian-45500"


def two_components_and_an_isolated_node():
    g = nx.disjoint_union(nx.cycle_graph(9), nx.balanced_tree(2, 3))
    g.add_node(g.number_of_nodes())
    return g


GRAPHS = {
    "grid3d-125": lambda: data.named_graph("grid3d-125"),
    "two-components": two_components_and_an_isolated_node,
    "path-300": lambda: nx.path_graph(300),
    "star-500": lambda: nx.star_graph(500),
    "tree-b3-h6": lambda: data.named_graph("tree-b3-h6"),
    "path-1000": lambda: nx.path_graph(1000),
    "margulis-71": lambda: data.named_graph("margulis-71"),
}
WEIGHTED = [("grid-5x5x5", "ints"), ("geometric+cycle", "wide")]           # the second one has unreachable pairs


@functools.lru_cache(maxsize=None)
def csr_of(name):
    return graph_csr(GRAPHS[name]())[:2]


@functools.lru_cache(maxsize=None)
def host_rows_of(name):
    rowptr, cols = csr_of(name)
    out = host_hop_rows(rowptr, cols, 0, rowptr.numel() - 1)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def device_rows_of(name):
    """int32 [N, N] on the device, from the hop kernel; never written afterwards."""
    rowptr, cols = csr_of(name)
    rows = ops.graph_hop_rows(rowptr.to(DEV), cols.to(DEV), 0, rowptr.numel() - 1)
    assert torch.equal(rows.cpu(), torch.tensor(host_rows_of(name)))
    return rows


@functools.lru_cache(maxsize=None)
def listed_ball(name, radius):
    """(pairs int64 [S, 2], dist fp64 [S]) tensors: the ball of the listed triplets, lexicographic."""
    full = host_rows_of(name)
    iu, ju = np.triu_indices(full.shape[0], k=1)
    d = full[iu, ju]
    inside = (d > 0) & (d <= radius)
    return torch.from_numpy(np.stack((iu[inside], ju[inside]), 1)), torch.from_numpy(d[inside].astype(np.float64))


def census_of(rows, row_begin, num_bins):
    bins = torch.zeros(num_bins, dtype=torch.int64, device=DEV)
    ops.graph_hop_census_rows(rows, row_begin, bins)
    return bins.cpu()


@pytest.mark.parametrize("name", list(GRAPHS))
def test_census_equals_the_host_restatement(name):
    rows = device_rows_of(name)
    N = rows.shape[0]
    want = torch.from_numpy(host_hop_census(host_rows_of(name), 0, N))
    assert torch.equal(census_of(rows, 0, N), want)
    rowptr, cols = csr_of(name)
    c = GraphDistances(rowptr, cols, device=DEV, max_block_bytes=4 * N * 192).census()
    diameter = int(torch.nonzero(want).max())
    assert torch.equal(c.histogram, want[:diameter + 1]) and c.triplets == int(want.sum()) and c.diameter == diameter
    assert ops.check_status(DEV) == (0, 0)


def test_census_past_the_lds_bins_and_into_the_overflow_counter():
    rows = device_rows_of("path-1000")
    header = open(os.path.join(ROOT, "include", "sympa_hip.h")).read()
    lds_bins = int(re.search(r"#define SYMPA_GRAPH_CENSUS_LDS_BINS (\d+)", header).group(1))
    assert 1 <= lds_bins <= 512 and rows.max().item() == 999                 # distances beyond every LDS bin
    full = census_of(rows, 0, 1000)
    assert full.tolist() == [0] + [1000 - d for d in range(1, 1000)]
    got = census_of(rows, 0, 600)
    assert torch.equal(got, torch.from_numpy(host_hop_census(host_rows_of("path-1000"), 0, 600)))
    assert got[0].item() == sum(1000 - d for d in range(600, 1000)) and torch.equal(got[1:], full[1:600])
    few = census_of(rows, 0, 1)
    assert few.tolist() == [999 * 1000 // 2]


@pytest.mark.parametrize("name", ["tree-b3-h6", "two-components", "path-1000"])
def test_every_blocking_of_the_rows_gives_the_same_census(name):
    rows = device_rows_of(name)
    N = rows.shape[0]
    want = census_of(rows, 0, N)
    for size in (1, 63, 64, 65, N):                                        # 65: row_begin no multiple of 64
        bins = torch.zeros(N, dtype=torch.int64, device=DEV)
        for b in range(0, N, size):
            ops.graph_hop_census_rows(rows[b:b + size], b, bins)
        assert torch.equal(bins.cpu(), want), size
    # a leading dimension above N, the padding full of a value that would land in bin 1
    wide = torch.full((N, N + 35), 1, dtype=torch.int32, device=DEV)
    wide[:, :N] = rows
    assert torch.equal(census_of(wide[:, :N], 0, N), want)
    assert torch.equal(census_of(wide[100 % N:, :N], 100 % N, N), torch.from_numpy(
        host_hop_census(host_rows_of(name)[100 % N:], 100 % N, N)))


def radii_of(rows):
    finite = rows[np.isfinite(rows)] if rows.dtype == np.float64 else rows
    return (0.5, 1, 2, float(finite.max()), 1e9)


@pytest.mark.parametrize("name", ["grid3d-125", "two-components", "tree-b3-h6"])
def test_ball_counts_of_hop_rows_equal_the_host(name):
    rows, host = device_rows_of(name), host_rows_of(name)
    N = rows.shape[0]
    for radius in radii_of(host):
        want = torch.from_numpy(host_ball_counts(host, 0, radius))
        assert torch.equal(ops.graph_ball_count_rows(rows, 0, radius).cpu(), want), radius
        b = 65 % N
        out = torch.full((N,), -7, dtype=torch.int64, device=DEV)
        ops.graph_ball_count_rows(rows[b:b + 70], b, radius, upper_count=out[b:b + 70])
        assert torch.equal(out[b:b + 70].cpu(), want[b:b + 70]) and (out[:b] == -7).all() and (out[b + 70:] == -7).all()
    rowptr, cols = csr_of(name)
    gd = GraphDistances(rowptr, cols, device=DEV, max_block_bytes=4 * N * 64)
    assert torch.equal(gd.ball_sizes(2).cpu(), torch.from_numpy(host_ball_counts(host, 0, 2)))


@pytest.mark.parametrize("case", WEIGHTED, ids=["-".join(c) for c in WEIGHTED])
def test_ball_counts_and_selection_of_weighted_rows_equal_the_host(case):
    host = wc.dijkstra_of(*case)
    N = host.shape[0]
    assert (case[0] == "geometric+cycle") == bool(np.isinf(host).any())
    rows = torch.from_numpy(np.array(host)).to(DEV)
    wide = torch.full((N, N + 3), 0.25, dtype=torch.float64, device=DEV)
    wide[:, :N] = rows
    for radius in radii_of(host):
        want = host_ball_counts(host, 0, radius)
        assert torch.equal(ops.graph_ball_count_rows(rows, 0, radius).cpu(), torch.from_numpy(want)), radius
        assert torch.equal(ops.graph_ball_count_rows(wide[:, :N], 0, radius).cpu(), torch.from_numpy(want)), radius
        req_row = np.repeat(np.arange(N), want)[::-1].copy()
        first = np.cumsum(want) - want
        req_rank = (np.arange(want.sum()) - np.repeat(first, want))[::-1].copy()
        col, dist = ops.graph_ball_select_rows(wide[:, :N], 0, radius, torch.from_numpy(req_row).to(DEV),
                                               torch.from_numpy(req_rank).to(DEV))
        want_col, want_dist = host_ball_select(host, 0, radius, req_row, req_rank)
        assert (want_col >= 0).all()
        assert torch.equal(col.cpu(), torch.from_numpy(want_col)) and torch.equal(dist.cpu(), torch.from_numpy(want_dist)), radius
    assert ops.check_status(DEV) == (0, 0)


@pytest.mark.parametrize("name", ["grid3d-125", "two-components"])           # N = 125, 25: a partial last word of 64 columns
def test_ball_selection_returns_every_listed_column_by_row_and_rank(name):
    rows = device_rows_of(name)
    N = rows.shape[0]
    for radius in (1, 3, 1e9):
        pairs, dist = listed_ball(name, radius)
        u = torch.bincount(pairs[:, 0], minlength=N)
        first = torch.cumsum(u, 0) - u
        rank = torch.arange(pairs.shape[0]) - first[pairs[:, 0]]
        # every (row, rank) once, shuffled, then a slice of them again: unsorted and repeated requests
        perm = torch.from_numpy(np.random.default_rng(5).permutation(pairs.shape[0]))
        perm = torch.cat((perm, perm[:97]))
        col, d = ops.graph_ball_select_rows(rows, 0, radius, pairs[perm, 0].to(DEV), rank[perm].to(DEV))
        assert torch.equal(col.cpu(), pairs[perm, 1]) and torch.equal(d.cpu(), dist[perm]), radius
        # a block that starts at row 7
        sel = perm[pairs[perm, 0] >= 7]
        col, d = ops.graph_ball_select_rows(rows[7:], 7, radius, pairs[sel, 0].to(DEV), rank[sel].to(DEV))
        assert torch.equal(col.cpu(), pairs[sel, 1]) and torch.equal(d.cpu(), dist[sel]), radius
        assert ops.check_status(DEV) == (0, 0)
        # ranks u and u + 5 of every row, and two rows outside the block
        req_row = torch.cat((torch.arange(N), torch.arange(N), torch.tensor([N, -1])))
        req_rank = torch.cat((u, u + 5, torch.tensor([0, 0])))
        col, d = ops.graph_ball_select_rows(rows, 0, radius, req_row.to(DEV), req_rank.to(DEV))
        assert (col == -1).all() and torch.isnan(d).all()
        with pytest.raises(IndexError, match=rf"\({2 * N + 2} pairs flagged\)"):
            ops.check_status(DEV)
        assert ops.check_status(DEV) == (0, 0)


@pytest.mark.parametrize("name,radius", [("grid3d-125", 3), ("tree-b3-h6", 4)])
def test_sample_ball_pairs_draws_the_listed_elements_in_every_blocking(name, radius):
    rowptr, cols = csr_of(name)
    N = rowptr.numel() - 1
    pairs, dist = listed_ball(name, radius)
    one = GraphDistances(rowptr, cols, device=DEV)
    small = GraphDistances(rowptr, cols, device=DEV, max_block_bytes=4 * N * 64)
    assert one.block_rows >= N and small.block_rows == 64
    upper = one.ball_sizes(radius)
    assert int(upper.sum()) == pairs.shape[0]
    batch = 4096
    for batch_id in (0, 3):
        k = (data.keyed_u64(42, 12, batch_id * batch + np.arange(batch, dtype=np.uint64)) % np.uint64(pairs.shape[0])).astype(np.int64)
        ids, d = one.sample_ball_pairs(radius, batch, batch_id=batch_id, upper=upper)
        assert ids.is_cuda and ids.dtype == torch.int64 and d.dtype == torch.float64
        assert torch.equal(ids.cpu(), pairs[k]) and torch.equal(d.cpu(), dist[k])
        ids64, d64 = small.sample_ball_pairs(radius, batch, batch_id=batch_id)
        assert torch.equal(ids64, ids) and torch.equal(d64, d)
    assert ops.check_status(DEV) == (0, 0)


def test_sample_ball_pairs_of_a_weighted_graph():
    rowptr, cols, weights, _ = wc.csr_of("geometric+cycle", "wide")
    N = rowptr.numel() - 1
    gd = WeightedGraphDistances(rowptr, cols, weights, device=DEV, max_block_bytes=8 * N * 64)
    all_ids, all_d = gd.triplets()
    radius, size = gd.radius_for_fraction(0.1)
    inside = all_d <= radius
    assert size == int(inside.sum()) >= round(all_d.numel() * 0.1)
    assert gd.diameter() == float(all_d.max())
    k = (data.keyed_u64(9, 12, 1000 + np.arange(1000, dtype=np.uint64)) % np.uint64(size)).astype(np.int64)
    ids, d = gd.sample_ball_pairs(radius, 1000, batch_id=1, seed=9)
    assert torch.equal(ids.cpu(), all_ids[inside].cpu()[k]) and torch.equal(d.cpu(), all_d[inside].cpu()[k])
    one = WeightedGraphDistances(rowptr, cols, weights, device=DEV)
    ids1, d1 = one.sample_ball_pairs(radius, 1000, batch_id=1, seed=9)
    assert torch.equal(ids1, ids) and torch.equal(d1, d)
    assert ops.check_status(DEV) == (0, 0)


def make_model(manifold, metric, n, table, scale_init=1.5, scale_coef=1.0):
    from sympa_amd.model import Model

    class A:
        pass
    A.manifold, A.metric, A.dims, A.num_points = manifold, metric, n, table.shape[0]
    A.scale_coef, A.scale_init, A.train_scale = scale_coef, scale_init, False
    m = Model(A)
    with torch.no_grad():
        m.embeddings.embeds.data = table
    return m.to(DEV)


@pytest.mark.parametrize("name,manifold,metric,n", [("grid3d-125", "upper", "riem", 3), ("two-components", "bounded", "finf", 3)])
def test_scaled_labels_over_all_pairs_equal_evaluate_over_the_scaled_triplets(name, manifold, metric, n):
    """Both values are fp64 sums of the same T non-negative terms in different orders (the scaled rows hold the bits
    data.scale_triplet_distances gives), so they differ by at most T * 2^-53 relative: the bound of test_graph_hops_gpu.py."""
    rowptr, cols = csr_of(name)
    N = rowptr.numel() - 1
    trip, _ = data.graph_triplets(GRAPHS[name]())
    T = trip.shape[0]
    m = make_model(manifold, metric, n, data.trained_like_table(N, n, model=manifold, seed=3))
    labels = data.scale_triplet_distances(trip[:, 2])
    want = m.evaluate(trip[:, :2].contiguous().to(DEV), labels.to(DEV), 4096)
    gd = GraphDistances(rowptr, cols, device=DEV)
    diameter = gd.census().diameter
    assert diameter == int(trip[:, 2].max())
    scaled = ScaledGraphDistances(gd, diameter)
    got = m.evaluate_all_pairs(scaled)
    rel = abs(got - want) / abs(want)
    print(f"evaluate_all_pairs over scaled rows {got!r} evaluate {want!r} relative difference {rel:.3e} bound {T * 2.0 ** -53:.3e}")
    assert rel <= T * 2.0 ** -53
    assert got == m.evaluate_all_pairs(scaled, max_block_bytes=16 * N * 64)
    assert ops.check_status(DEV) == (0, 0)


def ordered_pair_histogram(graph):
    rowptr, cols, _ = graph_csr(graph)
    return np.bincount(host_hop_rows(rowptr, cols, 0, rowptr.numel() - 1).ravel())


def test_the_census_of_the_product_graph_of_configs3_is_the_convolution_of_its_factors():
    """The distances of a Cartesian product add, so the ordered-pair hop histogram of the product is the convolution of the
    factors' ordered-pair histograms; unordered pairs at d > 0 are half of it.  An oracle that shares no code with the kernels."""
    conv = np.convolve(ordered_pair_histogram(nx.balanced_tree(3, 5)), ordered_pair_histogram(nx.grid_graph(dim=[5, 5, 5])))
    assert conv[0] == 45500 and (conv[1:] % 2 == 0).all()
    want = conv // 2
    want[0] = 0
    rowptr, cols, _ = graph_csr(data.named_graph(BIG))
    gd = GraphDistances(rowptr, cols, device=DEV)
    c = gd.census()
    assert torch.equal(c.histogram, torch.from_numpy(want.astype(np.int64)))
    assert c.triplets == 1035102250 and c.diameter == 22 and c.histogram[1].item() == 154575
    assert gd.radius_for_fraction(0.01, census=c) == (5, 11770540)
    assert ops.check_status(DEV) == (0, 0)


def run_training(extra):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_siegel
    lines = []
    args = train_siegel.parser().parse_args(["--graph", "grid3d-125", "--dims", "2", "--epochs", "3", "--val_every", "3",
                                             "--batch_size", "512"] + extra)
    model, hist = train_siegel.train(args, log=lines.append)
    assert len(hist) == 1 and hist[0][0] == 3
    loss, distortion = hist[0][1], hist[0][2]
    assert np.isfinite(loss) and loss > 0.0 and np.isfinite(distortion) and distortion > 0.0
    return model, distortion, lines


def test_training_on_the_listed_subsample_with_scaled_labels_validates_on_all_triplets():
    model, distortion, _ = run_training(["--subsample", "0.25", "--scale_triplets"])
    trip, _ = data.graph_triplets(data.named_graph("grid3d-125"))
    assert trip.shape[0] == 7750
    want = model.evaluate(trip[:, :2].contiguous().to(DEV), data.scale_triplet_distances(trip[:, 2]).to(DEV), 512)
    assert abs(distortion - want) <= trip.shape[0] * 2.0 ** -53 * abs(want)


def test_training_on_pairs_sampled_from_the_ball_scores_all_pairs():
    model, distortion, lines = run_training(["--sampled-pairs", "2048", "--subsample", "0.25"])
    assert any("radius 3: 2131 pairs" in line for line in lines), lines
    trip, _ = data.graph_triplets(data.named_graph("grid3d-125"))
    want = model.evaluate(trip[:, :2].contiguous().to(DEV), trip[:, 2].to(torch.float64).to(DEV), 512)
    assert abs(distortion - want) <= trip.shape[0] * 2.0 ** -53 * abs(want)
