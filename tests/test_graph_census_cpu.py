"""CPU (`-m "not gpu"`): the numpy restatements behind the graph distance census and the ball sampling
(graph.host_hop_census / host_ball_counts / host_ball_select), GraphDistances.census / radius_for_fraction / ball_sizes /
sample_ball_pairs on a CPU device, data.subsample_triplets, and the argument validation of the three C-ABI entries of
csrc/graph_census.hip -- against brute force over the listed triplets (np.triu_indices of the full hop matrix).
Reference: train.py:86-93, sympa/utils.py:71-102."""
import ctypes
import functools

import networkx as nx
import numpy as np
import pytest
import torch

from sympa_amd import _lib, data
from sympa_amd.graph import (GraphDistances, WeightedGraphDistances, graph_csr, host_ball_counts, host_ball_select,
                             host_hop_census, host_hop_rows)
from tests import graph_weighted_cases as wc


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
}
NAMES = list(GRAPHS)


@functools.lru_cache(maxsize=None)
def csr_of(name):
    return graph_csr(GRAPHS[name]())[:2]


@functools.lru_cache(maxsize=None)
def listed(name):
    """(full hop matrix, i, j, d) of the listed triplets, lexicographic; read-only."""
    rowptr, cols = csr_of(name)
    N = rowptr.numel() - 1
    full = host_hop_rows(rowptr, cols, 0, N)
    iu, ju = np.triu_indices(N, k=1)
    d = full[iu, ju].astype(np.int64)
    keep = d > 0
    out = full, iu[keep], ju[keep], d[keep]
    for a in out:
        a.setflags(write=False)
    return out


def brute_histogram(name):
    return np.bincount(listed(name)[3])


def brute_radius(name, F):
    """(r_F, |S_r|) from the sorted listed distances: the K-th smallest, and how many are no larger."""
    d = np.sort(listed(name)[3])
    K = round(d.size * F)
    return int(d[K - 1]), int((d <= d[K - 1]).sum())


@pytest.mark.parametrize("name", NAMES)
def test_host_census_equals_the_brute_force_histogram_in_every_blocking(name):
    full, _, _, d = listed(name)
    N = full.shape[0]
    want = brute_histogram(name)
    whole = host_hop_census(full, 0, N)
    assert whole.dtype == np.int64 and whole[0] == 0 and np.array_equal(np.trim_zeros(whole, "b"), want)
    for size in (1, 63, 100):
        bins = np.zeros(N, dtype=np.int64)
        for b in range(0, N, size):
            bins += host_hop_census(full[b:b + size], b, N)
        assert np.array_equal(bins, whole), size
    # bins the distances do not fit: the rest lands in the overflow counter
    few = host_hop_census(full, 0, 3)
    assert few[1:].tolist() == want[1:3].tolist() and few[0] == d.size - want[1:3].sum()


@pytest.mark.parametrize("name", NAMES)
def test_census_object_and_radius_on_a_cpu_graph_distances(name):
    rowptr, cols = csr_of(name)
    N = rowptr.numel() - 1
    gd = GraphDistances(rowptr, cols, max_block_bytes=4 * N * 64)             # 64-row blocks
    c = gd.census()
    want = brute_histogram(name)
    assert c.histogram.dtype == torch.int64 and c.histogram.tolist() == want.tolist()
    assert c.triplets == gd.count_triplets() == int(want.sum()) and c.diameter == want.size - 1
    for F in (0.01, 0.25, 0.5, 0.999, 1.0):
        assert gd.radius_for_fraction(F, census=c) == brute_radius(name, F), F
    with pytest.raises(ValueError):
        gd.radius_for_fraction(1e-9, census=c)
    with pytest.raises(ValueError):
        gd.radius_for_fraction(1.5, census=c)


def test_literal_values():
    h = brute_histogram("grid3d-125")
    assert h.sum() == 7750 and h.size - 1 == 12 and h[1:6].tolist() == [300, 705, 1126, 1401, 1416]
    gd = GraphDistances(*csr_of("grid3d-125"))
    c = gd.census()
    assert (c.triplets, c.diameter) == (7750, 12) and c.histogram[1:6].tolist() == [300, 705, 1126, 1401, 1416]
    assert gd.radius_for_fraction(0.25) == (3, 2131)
    c = GraphDistances(*csr_of("two-components")).census()
    assert (c.triplets, c.diameter) == (141, 6) and c.histogram[1:6].tolist() == [23, 28, 29, 29, 16]
    c = GraphDistances(*csr_of("path-300")).census()
    assert c.histogram.tolist() == [0] + [300 - d for d in range(1, 300)]
    star = GraphDistances(*csr_of("star-500"))
    c = star.census()
    assert c.histogram.tolist() == [0, 500, 124750]
    for F in (1.0, 0.5, 0.01, 501 / 125250, 500.6 / 125250):
        assert star.radius_for_fraction(F, census=c) == (2, 125250), F
    for F in (500 / 125250, 0.003, 1e-5):
        assert star.radius_for_fraction(F, census=c) == (1, 500), F


@pytest.mark.parametrize("name", NAMES)
def test_host_ball_counts_and_select_equal_the_listed_ball(name):
    full, iu, ju, d = listed(name)
    N = full.shape[0]
    for radius in (0.5, 1, 2, 3.5, int(d.max()), 1e9):
        inside = d <= radius
        want_u = np.bincount(iu[inside], minlength=N)
        u = host_ball_counts(full, 0, radius)
        assert u.dtype == np.int64 and np.array_equal(u, want_u), radius
        b = N // 3
        assert np.array_equal(host_ball_counts(full[b:b + 70], b, radius), want_u[b:b + 70])
        # every element of the ball by (row, rank), asked for in reversed order
        rows_of, cols_of, d_of = iu[inside][::-1], ju[inside][::-1], d[inside][::-1]
        first = np.cumsum(want_u) - want_u
        rank = np.flatnonzero(inside[inside])[::-1] - first[rows_of]
        col, dist = host_ball_select(full, 0, radius, rows_of, rank)
        assert np.array_equal(col, cols_of) and np.array_equal(dist, d_of.astype(np.float64)), radius
    # a rank the row does not have, a row outside the block
    u = host_ball_counts(full, 0, 2)
    col, dist = host_ball_select(full[:10], 0, 2, np.array([0, 0, 10, -1, 0]), np.array([u[0], u[0] + 5, 0, 0, -1]))
    assert col.tolist() == [-1] * 5 and np.isnan(dist).all()


def listed_ball(name, radius):
    _, iu, ju, d = listed(name)
    inside = d <= radius
    return np.stack((iu[inside], ju[inside]), 1), d[inside].astype(np.float64)


@pytest.mark.parametrize("name", ["grid3d-125", "two-components", "tree-b3-h6"])
def test_sample_ball_pairs_on_a_cpu_graph_distances_draws_the_listed_elements(name):
    rowptr, cols = csr_of(name)
    N = rowptr.numel() - 1
    one = GraphDistances(rowptr, cols)
    small = GraphDistances(rowptr, cols, max_block_bytes=4 * N * 64)
    for radius, batch, batch_id in ((1, 50, 0), (3, 700, 2), (2.5, 333, 7)):
        pairs, dist = listed_ball(name, radius)
        k = (data.keyed_u64(11, 12, batch_id * batch + np.arange(batch, dtype=np.uint64)) % np.uint64(len(dist))).astype(np.int64)
        ids, d = small.sample_ball_pairs(radius, batch, batch_id=batch_id, seed=11)
        assert ids.dtype == torch.int64 and d.dtype == torch.float64
        assert np.array_equal(ids.numpy(), pairs[k]) and np.array_equal(d.numpy(), dist[k])
        upper = one.ball_sizes(radius)
        assert int(upper.sum()) == len(dist)
        ids1, d1 = one.sample_ball_pairs(radius, batch, batch_id=batch_id, seed=11, upper=upper)
        assert torch.equal(ids1, ids) and torch.equal(d1, d)
    with pytest.raises(ValueError):
        one.sample_ball_pairs(0.5, 8)


def check_subsample(ids, dist, F):
    """The exact semantics on one list: K rows, the K smallest by (distance, position), in list order."""
    T = dist.shape[0]
    K = round(T * F)
    sub_ids, sub_d = data.subsample_triplets(ids, dist, F)
    assert sub_ids.shape[0] == sub_d.shape[0] == K
    r = np.sort(dist.numpy())[K - 1]
    assert (sub_d <= r).all()
    below = np.flatnonzero(dist.numpy() < r)
    at = np.flatnonzero(dist.numpy() == r)[:K - below.size]               # the first ones at the threshold, in list order
    keep = np.sort(np.concatenate((below, at)))
    assert torch.equal(sub_ids, ids[keep]) and torch.equal(sub_d, dist[keep])


@pytest.mark.parametrize("name", NAMES)
def test_subsample_triplets_keeps_the_shortest_and_breaks_ties_by_position(name):
    _, iu, ju, d = listed(name)
    trip = torch.from_numpy(np.stack((iu, ju, d), 1))
    gd = GraphDistances(*csr_of(name))
    for F in (0.01, 0.25, 0.6):
        sub = data.subsample_triplets(trip, None, F)
        r, _ = gd.radius_for_fraction(F)
        assert sub.dtype == torch.int64 and sub.shape == (round(trip.shape[0] * F), 3)
        assert int(sub[:, 2].max()) == r
        check_subsample(trip[:, :2], trip[:, 2].to(torch.float64), F)
        ids, dist = data.subsample_triplets(trip[:, :2], trip[:, 2].to(torch.float64), F)
        assert torch.equal(ids, sub[:, :2]) and torch.equal(dist, sub[:, 2].to(torch.float64))
    assert torch.equal(data.subsample_triplets(trip, None, 1.0), trip)
    with pytest.raises(ValueError):
        data.subsample_triplets(trip, None, 1e-9)
    with pytest.raises(ValueError):
        data.subsample_triplets(trip, None, 0.0)


@pytest.mark.parametrize("case", [("grid-5x5x5", "ints"), ("geometric+cycle", "wide"), ("heavy-edge-cycle", "fixed")])
def test_the_weighted_form(case):
    rowptr, cols, weights, _ = wc.csr_of(*case)
    N = rowptr.numel() - 1
    gd = WeightedGraphDistances(rowptr, cols, weights, max_block_bytes=8 * N * 64)
    ids, dist = gd.triplets()
    for F in (0.05, 0.5):
        check_subsample(ids, dist, F)
        K = round(dist.numel() * F)
        r = float(np.sort(dist.numpy())[K - 1])
        assert gd.radius_for_fraction(F) == (r, int((dist <= r).sum()))
    full, all_d = data.subsample_triplets(ids, dist, 1.0)
    assert torch.equal(full, ids) and torch.equal(all_d, dist)
    assert gd.diameter() == float(dist.max())
    # the ball through the fp64 rows
    radius = float(np.sort(dist.numpy())[dist.numel() // 7])
    inside = dist <= radius
    upper = gd.ball_sizes(radius)
    assert torch.equal(upper, torch.bincount(ids[inside, 0], minlength=N))
    k = (data.keyed_u64(42, 12, 3 * 200 + np.arange(200, dtype=np.uint64)) % np.uint64(int(inside.sum()))).astype(np.int64)
    got_ids, got_d = gd.sample_ball_pairs(radius, 200, batch_id=3, upper=upper)
    assert torch.equal(got_ids, ids[inside][k]) and torch.equal(got_d, dist[inside][k])
    with pytest.raises(MemoryError, match="explicit radius"):
        gd.radius_for_fraction(0.5, max_bytes=1024)
    with pytest.raises(NotImplementedError):
        gd.census()


def test_scaled_graph_distances_on_the_cpu():
    from sympa_amd.graph import ScaledGraphDistances
    full, iu, ju, d = listed("two-components")
    gd = GraphDistances(*csr_of("two-components"))
    rows = ScaledGraphDistances(gd, 6).rows(0, 25)
    assert rows.dtype == torch.float64 and (rows.diagonal() == 0).all()
    assert torch.equal(rows[torch.tensor(iu), torch.tensor(ju)], data.scale_triplet_distances(torch.tensor(d)))
    assert torch.isinf(rows[torch.from_numpy(full < 0)]).all() and torch.isfinite(rows[torch.from_numpy(full >= 0)]).all()


def test_argument_validation_without_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(64)   # never dereferenced: validation happens before any launch
    census, count, select = lib.sympa_graph_hop_census_rows, lib.sympa_graph_ball_count_rows, lib.sympa_graph_ball_select_rows
    # zero-size calls are no-ops
    assert census(one, 10, 0, 0, 10, one, 10, None) == 0
    assert count(one, 0, 10, 3, 0, 10, 2.0, one, None) == 0
    assert count(one, 1, 10, 3, 0, 10, 2.0, one, None) == 0
    assert select(one, 0, 10, 0, 0, 10, 2.0, one, one, 4, one, one, one, None) == 0
    assert select(one, 1, 10, 0, 5, 10, 2.0, one, one, 0, one, None, None, None) == 0
    # census
    assert census(None, 10, 0, 5, 10, one, 10, None) == -1              # null rows
    assert census(one, 10, 0, 5, 10, None, 10, None) == -1              # null bins
    assert census(one, 9, 0, 5, 10, one, 10, None) == -1                # ld < num_nodes
    assert census(one, 10, 0, -1, 10, one, 10, None) == -1              # negative count
    assert census(one, 10, -1, 5, 10, one, 10, None) == -1
    assert census(one, 10, 6, 5, 10, one, 10, None) == -1               # block past the last row
    assert census(one, 10, 0, 5, 0, one, 10, None) == -1                # no nodes
    assert census(one, 10, 0, 5, 10, one, 0, None) == -1                # num_bins < 1
    assert b"num_bins" in lib.sympa_last_error()
    # ball count
    assert count(None, 0, 10, 0, 5, 10, 2.0, one, None) == -1
    assert count(one, 0, 10, 0, 5, 10, 2.0, None, None) == -1
    assert count(one, 0, 9, 0, 5, 10, 2.0, one, None) == -1
    assert count(one, 0, 10, 0, -5, 10, 2.0, one, None) == -1
    assert count(one, 2, 10, 0, 5, 10, 2.0, one, None) == -1            # neither int32 nor fp64
    for radius in (float("nan"), -1.0, float("inf")):
        assert count(one, 0, 10, 0, 5, 10, radius, one, None) == -1
        assert count(one, 1, 10, 0, 5, 10, radius, one, None) == -1
        assert select(one, 0, 10, 0, 5, 10, radius, one, one, 4, one, one, one, None) == -1
    assert b"radius" in lib.sympa_last_error()
    # ball select
    assert select(None, 0, 10, 0, 5, 10, 2.0, one, one, 4, one, one, one, None) == -1
    assert select(one, 0, 10, 0, 5, 10, 2.0, None, one, 4, one, one, one, None) == -1
    assert select(one, 0, 10, 0, 5, 10, 2.0, one, None, 4, one, one, one, None) == -1
    assert select(one, 0, 10, 0, 5, 10, 2.0, one, one, 4, None, one, one, None) == -1
    assert select(one, 0, 9, 0, 5, 10, 2.0, one, one, 4, one, one, one, None) == -1
    assert select(one, 0, 10, 0, 5, 10, 2.0, one, one, -4, one, one, one, None) == -1
    assert select(one, 0, 10, 8, 5, 10, 2.0, one, one, 4, one, one, one, None) == -1
