"""CPU (`-m "not gpu"`): graph hop distances a block of rows at a time (sympa_amd/graph.py): the CSR of a networkx graph, the
numpy restatement of the bit-parallel BFS the kernel runs (csrc/graph_bfs.hip), GraphDistances on CPU tensors, and the argument
validation of the two C-ABI entries.  Reference: preprocess.py:101-126 (all-pairs hop distances), through data.graph_triplets."""
import ctypes
import functools

import networkx as nx
import numpy as np
import pytest
import torch

from sympa_amd import _lib, data, ops
from sympa_amd.graph import GraphDistances, graph_csr, host_hop_rows


def two_components_and_an_isolated_node():
    g = nx.disjoint_union(nx.cycle_graph(9), nx.balanced_tree(2, 3))
    g.add_node(g.number_of_nodes())
    return g


def networkx_rows(graph, sources):
    """int32 [len(sources), N] from networkx BFS over the graph relabelled the way graph_csr relabels it."""
    g = nx.convert_node_labels_to_integers(graph, ordering="sorted")
    out = np.full((len(sources), g.number_of_nodes()), -1, dtype=np.int32)
    for k, s in enumerate(sources):
        for v, d in nx.single_source_shortest_path_length(g, int(s)).items():
            out[k, v] = d
    return out


CASES = {
    "grid3d-125": (lambda: data.named_graph("grid3d-125"), None),
    "tree-b3-h6": (lambda: data.named_graph("tree-b3-h6"), 64),
    "margulis-71": (lambda: data.named_graph("margulis-71"), 16),
    "two-components": (two_components_and_an_isolated_node, None),
    "path-300": (lambda: nx.path_graph(300), None),
    "star-500": (lambda: nx.star_graph(500), None),
}


@functools.lru_cache(maxsize=None)
def csr_of(name):
    return graph_csr(CASES[name][0]())


def spread_sources(N, how_many):
    return np.arange(N) if how_many is None else np.unique(np.linspace(0, N - 1, how_many).astype(np.int64))


@pytest.mark.parametrize("name", list(CASES))
def test_host_rows_equal_networkx_bfs(name):
    rowptr, cols, _ = csr_of(name)
    N = rowptr.numel() - 1
    sources = spread_sources(N, CASES[name][1])
    want = networkx_rows(CASES[name][0](), sources)
    if CASES[name][1] is None:
        got = host_hop_rows(rowptr, cols, 0, N)
    else:
        got = np.concatenate([host_hop_rows(rowptr, cols, int(s), 1) for s in sources])
    np.testing.assert_array_equal(got, want)
    assert (got[np.arange(len(sources)), sources] == 0).all()


def test_margulis_csr_drops_the_self_loops_and_parallel_edges():
    g = data.named_graph("margulis-71")
    assert nx.number_of_selfloops(g) == 284
    rowptr, cols, id2node = csr_of("margulis-71")
    N = rowptr.numel() - 1
    assert N == 71 * 71 and id2node[0] == (0, 0)
    rows = np.repeat(np.arange(N), np.diff(rowptr.numpy()))
    c = cols.numpy()
    assert (rows != c).all()
    key = rows * N + c
    assert (np.diff(key) > 0).all()                                       # ascending and unique
    assert set(key.tolist()) == set((c * N + rows).tolist())              # symmetric
    simple = nx.Graph(nx.convert_node_labels_to_integers(g, ordering="sorted"))
    simple.remove_edges_from(list(nx.selfloop_edges(simple)))
    assert c.size == 2 * simple.number_of_edges()


def test_unreachable_nodes_are_minus_one_and_the_diagonal_zero():
    rowptr, cols, _ = csr_of("two-components")
    N = rowptr.numel() - 1
    got = host_hop_rows(rowptr, cols, 0, N)
    assert (np.diag(got) == 0).all()
    assert (got[:9, 9:] == -1).all() and (got[9:, :9] == -1).all()
    assert (got[N - 1, :N - 1] == -1).all() and (got[:N - 1, N - 1] == -1).all()
    assert got[:9, :9].max() == 4 and got[:9, :9].min() == 0


@pytest.mark.parametrize("name", ["grid3d-125", "two-components", "path-300"])
def test_blocking_of_the_sources_does_not_change_a_row(name):
    rowptr, cols, _ = csr_of(name)
    N = rowptr.numel() - 1
    full = host_hop_rows(rowptr, cols, 0, N)
    for size in (1, 7, 63, 65, 100):
        begins = range(0, N, size) if size > 1 else (0, N // 2, N - 1)
        for b in begins:
            r = min(size, N - b)
            np.testing.assert_array_equal(host_hop_rows(rowptr, cols, b, r), full[b:b + r])
    r = min(70, N - 3)                                                   # begin > 0, not a multiple of 64
    np.testing.assert_array_equal(host_hop_rows(rowptr, cols, 3, r), full[3:3 + r])


def test_a_column_outside_the_graph_is_skipped_on_the_host_too():
    rowptr, cols, _ = csr_of("grid3d-125")
    rp, c = rowptr.numpy().copy(), cols.numpy()
    c = np.concatenate((c[:rp[8]], [10 ** 6], c[rp[8]:])).astype(np.int32)      # one extra entry at the end of row 7
    rp[8:] += 1
    np.testing.assert_array_equal(host_hop_rows(rp, c, 0, 125), host_hop_rows(rowptr, cols, 0, 125))


@pytest.mark.parametrize("name", ["grid3d-125", "tree-b3-h6"])
def test_triplets_on_cpu_tensors_equal_graph_triplets(name):
    rowptr, cols, id2node = csr_of(name)
    want, want_ids = data.graph_triplets(data.named_graph(name))
    gd = GraphDistances(rowptr, cols, max_block_bytes=64 * 4 * (rowptr.numel() - 1) * 3)      # several blocks
    got = gd.triplets()
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert id2node == want_ids
    assert gd.count_triplets() == want.shape[0]


def test_pairs_match_a_lookup_in_the_triplets():
    rowptr, cols, _ = csr_of("grid3d-125")
    trip, _ = data.graph_triplets(data.named_graph("grid3d-125"))
    table = {(int(i), int(j)): int(d) for i, j, d in trip.tolist()}
    gd = GraphDistances(rowptr, cols, max_block_bytes=1)                                      # 64 rows per block
    assert gd.block_rows == 64
    ids = data.sample_pairs(125, 700, batch_id=3)
    got = gd.pairs(ids)
    assert got.dtype == torch.float64 and got.shape == (700,)
    want = [table[(min(i, j), max(i, j))] for i, j in ids.tolist()]
    assert got.tolist() == want
    assert gd.pairs(torch.tensor([[5, 5], [124, 0]])).tolist() == [0.0, 12.0]
    with pytest.raises(IndexError):
        gd.pairs(torch.tensor([[0, 125]]))


def test_pairs_across_components_are_infinite():
    rowptr, cols, _ = csr_of("two-components")
    gd = GraphDistances(rowptr, cols)
    got = gd.pairs(torch.tensor([[0, 4], [0, 9], [24, 0], [9, 10]]))
    assert got.tolist() == [4.0, float("inf"), float("inf"), 1.0]


def test_triplets_refuse_to_outgrow_their_budget():
    rowptr, cols, _ = csr_of("grid3d-125")
    gd = GraphDistances(rowptr, cols)
    with pytest.raises(MemoryError, match="7750 triplets"):
        gd.triplets(max_bytes=7750 * 24 - 1)
    assert gd.triplets(max_bytes=7750 * 24).shape == (7750, 3)


def test_neighbor_csr_equals_the_neighbour_sets_of_the_triplets():
    for name in ("grid3d-125", "margulis-71"):
        rowptr, cols, _ = csr_of(name)
        trip, _ = data.graph_triplets(data.named_graph(name))
        want = ops.neighbor_csr(trip[:, :2], trip[:, 2], rowptr.numel() - 1)
        got = GraphDistances(rowptr, cols).neighbor_csr()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32


def test_metric_from_csr_equals_the_metric_from_triplets():
    from sympa_amd.metrics import MeanAveragePrecisionMetric
    rowptr, cols, _ = csr_of("grid3d-125")
    trip, _ = data.graph_triplets(data.named_graph("grid3d-125"))
    a = MeanAveragePrecisionMetric((trip[:, :2], trip[:, 2].to(torch.float32)))
    b = MeanAveragePrecisionMetric.from_csr(*GraphDistances(rowptr, cols).neighbor_csr())
    assert a.num_nodes == b.num_nodes and a.max_degree == b.max_degree == 6
    assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.cols, b.cols) and a.neighbors == b.neighbors


def test_weighted_graph_is_refused_with_the_path_to_use():
    g = nx.path_graph(5)
    g[1][2]["weight"] = 2.5
    with pytest.raises(NotImplementedError, match="data.graph_triplets"):
        graph_csr(g)


def test_the_product_graph_has_its_name_and_its_45500_nodes():
    g = data.named_graph("product-cartesian-45500")
    assert g.number_of_nodes() == 45500
    rowptr, cols, id2node = graph_csr(g)
    assert rowptr.numel() == 45501 and id2node[0] == (0, (0, 0, 0))
    # 363 tree edges x 125 grid nodes + 300 grid edges x 364 tree nodes, both directions
    assert cols.numel() == 2 * (363 * 125 + 300 * 364)
    got = host_hop_rows(rowptr, cols, 45436, 64)
    np.testing.assert_array_equal(got[-2:], networkx_rows(g, [45498, 45499]))
    assert got.max() == 22 and got.min() == 0                  # tree diameter 10 + grid diameter 12, from a leaf-corner node


def test_header_declares_what_the_binding_lists():
    import os
    import re
    from tests.helpers import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sympa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sympa_[a-z_0-9]+)\s*\(", text))
    for s in ("sympa_graph_hops_workspace_bytes", "sympa_graph_hop_rows", "sympa_graph_distortion_rows"):
        assert s in declared and s in _lib.SYMBOLS and hasattr(_lib.load(), s)
    assert declared == set(_lib.SYMBOLS)


def test_argument_validation_without_gpu():
    lib = _lib.load()
    al = ctypes.c_void_p(64)       # never dereferenced: validation happens before any launch
    N, E = 100, 400
    assert lib.sympa_graph_hops_workspace_bytes(N, 1) == 24 * N
    assert lib.sympa_graph_hops_workspace_bytes(N, 64) == 24 * N
    assert lib.sympa_graph_hops_workspace_bytes(N, 65) == 48 * N
    assert lib.sympa_graph_hops_workspace_bytes(45500, 45500) == 711 * 24 * 45500
    assert lib.sympa_graph_hops_workspace_bytes(0, 5) == 0 and lib.sympa_graph_hops_workspace_bytes(N, 0) == 0
    ws = 48 * N

    def call(rowptr=al, cols=al, n=N, e=E, begin=0, count=100, out=al, stride=N, work=al, work_bytes=ws):
        return lib.sympa_graph_hop_rows(rowptr, cols, n, e, begin, count, out, stride, work, work_bytes, None, None)
    assert call(count=0) == 0                                   # an empty block is a no-op
    assert call(rowptr=None) == -1 and b"null" in lib.sympa_last_error()
    assert call(cols=None) == -1
    assert call(out=None) == -1
    assert call(work=None) == -1 and b"workspace" in lib.sympa_last_error()
    assert call(n=0) == -1 and call(n=-3) == -1
    assert call(e=-1) == -1
    assert call(begin=-1) == -1 and call(begin=1) == -1 and call(count=101) == -1 and call(count=-1) == -1
    assert b"source block" in lib.sympa_last_error()
    assert call(stride=N - 1) == -1 and b"row_stride" in lib.sympa_last_error()
    assert call(work_bytes=ws - 1) == -1 and b"workspace" in lib.sympa_last_error()
    assert call(work=ctypes.c_void_p(68)) == -1                 # not 8-byte aligned
    # the distortion rows
    d = lambda **k: lib.sympa_graph_distortion_rows(k.get("dist", al), k.get("ld", N), k.get("hops", al), k.get("ldh", N),  # noqa: E731
                                                    k.get("begin", 0), k.get("count", 10), k.get("n", N), k.get("s", al),
                                                    k.get("p", al), None)
    assert d(count=0) == 0
    assert d(dist=None) == -1 and d(hops=None) == -1 and d(s=None) == -1 and d(p=None) == -1
    assert d(n=0) == -1 and d(begin=95) == -1 and d(ld=N - 1) == -1 and d(ldh=N - 1) == -1


def test_product_path_refuses_cpu_tensors():
    rowptr, cols, _ = csr_of("grid3d-125")
    with pytest.raises(_lib.SympaHipError):
        ops.graph_hop_rows(rowptr, cols, 0, 125)
    with pytest.raises(_lib.SympaHipError):
        ops.graph_distortion_rows(torch.zeros(2, 125, dtype=torch.float64), torch.zeros(2, 125, dtype=torch.int32), 0)
