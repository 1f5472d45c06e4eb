"""CPU (`-m "not gpu"`): weighted shortest-path distances a block of rows at a time (sympa_amd/graph.py): the weighted CSR of a
networkx graph, the numpy restatement of the fixed point the kernel computes (csrc/graph_sssp.hip), WeightedGraphDistances on CPU
tensors, the .edges reader, and the argument validation of the three C-ABI entries.  Every comparison of rows is bit for bit: the
rows are the unique least fixed point of the relaxation, which is what Dijkstra from each source computes.
Reference: preprocess.py:76-86 (loader), 108-126 (weighted all-pairs distances), sympa/metrics.py:31-36 (neighbour sets)."""
import ctypes

import networkx as nx
import numpy as np
import pytest
import torch

from sympa_amd import _lib, data, ops
from sympa_amd.graph import (GraphDistances, WeightedGraphDistances, graph_csr, host_hop_rows, host_weighted_rows,
                             weighted_graph_csr)
from tests.graph_weighted_cases import CASE_IDS, CASES, csr_of, dijkstra_of, graph_of


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def assert_same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} of {got.size} entries differ"


@pytest.mark.parametrize("name,kind", CASES, ids=CASE_IDS)
def test_host_rows_equal_scipy_dijkstra_bit_for_bit(name, kind):
    rowptr, cols, weights, _ = csr_of(name, kind)
    N = rowptr.numel() - 1
    got = host_weighted_rows(rowptr, cols, weights, 0, N)
    assert_same_bits(got, dijkstra_of(name, kind))
    assert (np.diag(got) == 0).all() and not np.signbit(np.diag(got)).any()


def test_zero_weight_edges_equal_networkx_dijkstra():
    rowptr, cols, weights, _ = csr_of("zero-weights", "fixed")
    assert (weights == 0).sum() > 20 and not np.signbit(weights.numpy()).any()          # -0.0 was taken as 0
    g = nx.convert_node_labels_to_integers(graph_of("zero-weights", "fixed"), ordering="sorted")
    N = g.number_of_nodes()
    want = np.full((N, N), np.inf)
    for s in range(N):
        for v, d in nx.single_source_dijkstra_path_length(g, s).items():
            want[s, v] = d
    got = host_weighted_rows(rowptr, cols, weights, 0, N)
    assert_same_bits(got, want)
    assert (got == 0).sum() > N                                                        # pairs at distance 0 besides the diagonal


def test_the_lightest_route_is_not_the_hop_nearest_one():
    rowptr, cols, weights, _ = csr_of("heavy-edge-cycle", "fixed")
    got = host_weighted_rows(rowptr, cols, weights, 0, 64)
    assert got[0, 63] == 63.0 and got[63, 0] == 63.0 and got[0, 32] == 32.0 and got[10, 50] == 40.0


@pytest.mark.parametrize("name,kind", [("grid-5x5x5", "wide"), ("geometric+cycle", "unit"), ("path-300", "ints")])
def test_blocking_of_the_sources_does_not_change_a_row(name, kind):
    rowptr, cols, weights, _ = csr_of(name, kind)
    N = rowptr.numel() - 1
    full = dijkstra_of(name, kind)
    for size in (1, 7, 63, 65, 100):
        begins = range(0, N, size) if size > 1 else (0, N // 2, N - 1)
        for b in begins:
            r = min(size, N - b)
            assert_same_bits(host_weighted_rows(rowptr, cols, weights, b, r), full[b:b + r])
    r = min(70, N - 3)                                                   # begin > 0, not a multiple of 64
    assert_same_bits(host_weighted_rows(rowptr, cols, weights, 3, r), full[3:3 + r])


def test_rows_are_not_symmetrised():
    """Row i is summed from i and row j from j: with weights over six decades the two sums of one path differ in the last bits."""
    rowptr, cols, weights, _ = csr_of("grid-5x5x5", "wide")
    got = host_weighted_rows(rowptr, cols, weights, 0, 125)
    asym = int((bits(got) != bits(got.T)).sum())
    print(f"{asym} of {got.size} entries differ from their transpose")
    assert asym > 0
    assert np.allclose(got, got.T, rtol=1e-14, atol=0)
    assert_same_bits(got, dijkstra_of("grid-5x5x5", "wide"))           # every row equals Dijkstra from its own source
    gd = WeightedGraphDistances(rowptr, cols, weights)
    i, j = np.argwhere(bits(got) != bits(got.T))[0]
    assert gd.pairs(torch.tensor([[i, j], [j, i]])).tolist() == [got[i, j], got[j, i]]


def test_unreachable_nodes_are_inf_and_the_diagonal_zero():
    rowptr, cols, weights, _ = csr_of("geometric+cycle", "ints")
    got = host_weighted_rows(rowptr, cols, weights, 0, 190)
    assert (np.diag(got) == 0).all()
    assert np.isinf(got[:150, 150:]).all() and np.isinf(got[150:, :150]).all() and np.isfinite(got[150:, 150:]).all()


def test_margulis_csr_drops_the_self_loops_and_parallel_edges():
    g = graph_of("margulis-12", "unit")
    assert g.is_multigraph() and nx.number_of_selfloops(g) > 0
    rowptr, cols, weights, id2node = csr_of("margulis-12", "unit")
    N = rowptr.numel() - 1
    assert N == 144 and id2node[0] == (0, 0)
    assert rowptr.dtype == torch.int64 and cols.dtype == torch.int32 and weights.dtype == torch.float64
    rows = np.repeat(np.arange(N), np.diff(rowptr.numpy()))
    c, w = cols.numpy().astype(np.int64), weights.numpy()
    assert (rows != c).all()
    assert (np.diff(rows * N + c) > 0).all()                             # ascending and unique
    simple = nx.Graph(nx.convert_node_labels_to_integers(g, ordering="sorted"))
    simple.remove_edges_from(list(nx.selfloop_edges(simple)))
    assert c.size == 2 * simple.number_of_edges()
    table = {(int(r), int(k)): float(x) for r, k, x in zip(rows, c, w)}
    for u, v, d in simple.edges(data=True):
        assert table[(u, v)] == table[(v, u)] == d["weight"]             # both directions, one weight: nx.Graph's survivor


def test_a_repeated_edge_keeps_its_last_weight():
    g = nx.Graph()
    g.add_edge("a", "b", weight=2.0)
    g.add_edge("b", "c", weight=1.0)
    g.add_edge("b", "a", weight=0.25)
    g.add_edge("c", "c", weight=9.0)
    rowptr, cols, weights, id2node = weighted_graph_csr(g)
    assert id2node == {0: "a", 1: "b", 2: "c"}
    assert rowptr.tolist() == [0, 1, 3, 4] and cols.tolist() == [1, 0, 2, 1] and weights.tolist() == [0.25, 0.25, 1.0, 1.0]


def test_graphs_that_are_not_weighted_throughout_are_refused():
    g = nx.path_graph(5)
    with pytest.raises(ValueError, match="graph_csr"):
        weighted_graph_csr(g)
    g[1][2]["weight"] = 2.5                                              # mixed: nx.is_weighted is False
    with pytest.raises(ValueError, match="graph_csr"):
        weighted_graph_csr(g)
    with pytest.raises(NotImplementedError, match="weighted_graph_csr"):
        graph_csr(g)
    nx.set_edge_attributes(g, 1.0, "weight")
    for bad in (float("nan"), -1.0, float("inf")):
        g[2][3]["weight"] = bad
        with pytest.raises(ValueError, match="finite and not negative"):
            weighted_graph_csr(g)
    g[2][3]["weight"] = 0.0
    assert weighted_graph_csr(g)[2].tolist().count(0.0) == 2


def test_bad_entries_are_skipped_on_the_host_too():
    rowptr, cols, weights, _ = csr_of("grid-5x5x5", "unit")
    want = dijkstra_of("grid-5x5x5", "unit")
    rp = rowptr.numpy().copy()
    at = rp[8]                                                           # extra entries at the end of row 7
    c = np.concatenate((cols.numpy()[:at], [10 ** 6, 3, 4, 5], cols.numpy()[at:])).astype(np.int32)
    w = np.concatenate((weights.numpy()[:at], [0.5, np.nan, -1.0, np.inf], weights.numpy()[at:]))
    rp[8:] += 4
    assert_same_bits(host_weighted_rows(rp, c, w, 0, 125), want)
    rp[-1] += 50                                                         # a row range past the entries is clamped
    assert_same_bits(host_weighted_rows(rp, c, w, 0, 125), want)


def test_load_edges_reads_what_the_reference_loader_reads(tmp_path):
    path = tmp_path / "toy.edges"
    path.write_text("a b\nb c 2.5\nc d 3\nd e x7\ne f 1e3\nf g -2\ng h .5\n  h   i\t0.125  trailing\n\nb c 4.\n")
    g = data.load_edges(path)
    assert isinstance(g, nx.Graph) and not g.is_multigraph() and g.name == "toy"
    assert data.load_edges(str(path), name="other").name == "other"
    got = {tuple(sorted((u, v))): d for u, v, d in g.edges(data=True)}
    assert got == {("a", "b"): {}, ("b", "c"): {"weight": 4.0}, ("c", "d"): {"weight": 3.0}, ("d", "e"): {}, ("e", "f"): {},
                   ("f", "g"): {}, ("g", "h"): {"weight": 0.5}, ("h", "i"): {"weight": 0.125}}
    assert not nx.is_weighted(g)
    path.write_text("0 1 1.5\n1 2 2\n")
    assert nx.is_weighted(data.load_edges(path))


def brute_force(name, kind):
    """(ids [T, 2], dist [T]) of every i < j with 0 < D[i][j] < inf taken from row i, and the distance-1.0 neighbour sets."""
    D = dijkstra_of(name, kind)
    N = D.shape[0]
    ids, dist, nbrs = [], [], [set() for _ in range(N)]
    for i in range(N):
        for j in range(N):
            if j > i and 0 < D[i, j] < np.inf:
                ids.append((i, j))
                dist.append(D[i, j])
            if i != j and D[i, j] == 1.0:
                nbrs[i].add(j)
                nbrs[j].add(i)
    return np.array(ids, dtype=np.int64).reshape(-1, 2), np.array(dist, dtype=np.float64), nbrs


@pytest.mark.parametrize("name,kind", [("grid-5x5x5", "ints"), ("geometric+cycle", "wide"), ("zero-weights", "fixed")])
def test_triplets_pairs_and_neighbours_on_cpu_tensors_equal_a_brute_force_construction(name, kind):
    rowptr, cols, weights, id2node = csr_of(name, kind)
    N = rowptr.numel() - 1
    want_ids, want_dist, want_nbrs = brute_force(name, kind)
    gd = WeightedGraphDistances(rowptr, cols, weights, max_block_bytes=1)                 # 64 rows per block: several blocks
    assert gd.block_rows == 64 and gd.rows(0, 3).dtype == torch.float64
    ids, dist = gd.triplets()
    assert ids.dtype == torch.int64 and dist.dtype == torch.float64
    assert np.array_equal(ids.numpy(), want_ids)
    assert_same_bits(dist.numpy(), want_dist)
    assert gd.count_triplets() == want_ids.shape[0]
    t_ids, t_dist, t_id2node = data.weighted_graph_triplets(graph_of(name, kind))
    assert torch.equal(t_ids, ids) and t_id2node == id2node
    assert_same_bits(t_dist.numpy(), want_dist)
    pairs = data.sample_pairs(N, 500, batch_id=2)
    D = dijkstra_of(name, kind)
    assert_same_bits(gd.pairs(pairs).numpy(), D[pairs[:, 0].numpy(), pairs[:, 1].numpy()])      # from the FIRST node's row
    with pytest.raises(IndexError):
        gd.pairs(torch.tensor([[0, N]]))
    nb_rowptr, nb_cols = gd.neighbor_csr()
    assert nb_rowptr.dtype == torch.int64 and nb_cols.dtype == torch.int32
    for i in range(N):
        assert nb_cols[nb_rowptr[i]:nb_rowptr[i + 1]].tolist() == sorted(want_nbrs[i])
    if kind == "ints":
        assert nb_cols.numel() > 0 and nb_cols.numel() != cols.numel()                   # distance exactly 1.0, not adjacency


def test_pairs_across_components_are_infinite():
    rowptr, cols, weights, _ = csr_of("geometric+cycle", "ints")
    got = WeightedGraphDistances(rowptr, cols, weights).pairs(torch.tensor([[0, 160], [170, 3], [5, 5]]))
    assert got.tolist() == [float("inf"), float("inf"), 0.0]


@pytest.mark.parametrize("build", [lambda: nx.grid_graph(dim=[5, 5, 5]), lambda: nx.balanced_tree(3, 5),
                                   lambda: nx.disjoint_union(nx.cycle_graph(9), nx.path_graph(4))])
def test_unit_weights_give_the_hop_rows(build):
    g = build()
    rowptr, cols, _ = graph_csr(g)
    nx.set_edge_attributes(g, 1.0, "weight")
    w_rowptr, w_cols, weights, _ = weighted_graph_csr(g)
    assert torch.equal(rowptr, w_rowptr) and torch.equal(cols, w_cols) and (weights == 1.0).all()
    N = rowptr.numel() - 1
    hops = host_hop_rows(rowptr, cols, 0, N).astype(np.float64)
    hops[hops < 0] = np.inf
    assert_same_bits(host_weighted_rows(rowptr, cols, weights, 0, N), hops)
    a, b = GraphDistances(rowptr, cols).neighbor_csr(), WeightedGraphDistances(rowptr, cols, weights).neighbor_csr()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_triplets_refuse_to_outgrow_their_budget():
    rowptr, cols, weights, _ = csr_of("grid-5x5x5", "ints")
    gd = WeightedGraphDistances(rowptr, cols, weights)
    with pytest.raises(MemoryError, match="7750 triplets"):
        gd.triplets(max_bytes=7750 * 24 - 1)
    ids, dist = gd.triplets(max_bytes=7750 * 24)
    assert ids.shape == (7750, 2) and dist.shape == (7750,)


def test_block_arithmetic():
    rowptr, cols, weights, _ = csr_of("tree-b3-h6", "ints")
    N = 1093
    gd = WeightedGraphDistances(rowptr, cols, weights, max_block_bytes=8 * N * 200)
    assert gd.block_rows == 192 == gd.rows_per_block(8 * N * 200)        # whole groups of 64 rows at 8 N bytes per row
    assert gd.rows_per_block(1) == 64 and gd.rows_per_block(1 << 40) == 1152
    assert gd.workspace_bytes() == 192 * (N + 1) * 8 and gd.workspace_bytes(1) == 8 * (N + 1) * 8 and gd.workspace_bytes(0) == 0
    with pytest.raises(ValueError):
        gd.rows(N - 3, 4)
    with pytest.raises(ValueError, match="weights"):
        WeightedGraphDistances(rowptr, cols, weights[:-1])
    seen = [(b, r.shape[0]) for b, r in gd.blocks()]
    assert seen == [(b, min(192, N - b)) for b in range(0, N, 192)]
    gd.release()


def test_float_triplets_survive_the_preprocessed_file(tmp_path):
    ids, dist, id2node = data.weighted_graph_triplets(graph_of("grid-5x5x5", "wide"))
    path = str(tmp_path / "preprocessed-data.pt")
    data.save_preprocessed(path, torch.cat((ids.to(torch.float64), dist[:, None]), 1), id2node)
    got_ids, got_dist, got_id2node = data.load_preprocessed(path)
    assert torch.equal(got_ids, ids) and got_id2node == id2node
    assert_same_bits(got_dist.numpy(), dist.numpy())


def test_graph_triplets_still_ignores_the_weights():
    g = graph_of("grid-5x5x5", "wide")
    plain, _ = data.graph_triplets(nx.grid_graph(dim=[5, 5, 5]))
    assert torch.equal(data.graph_triplets(g)[0], plain)


def test_header_declares_what_the_binding_lists():
    import os
    import re
    from tests.helpers import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sympa_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sympa_[a-z_0-9]+)\s*\(", text))
    for s in ("sympa_graph_weighted_workspace_bytes", "sympa_graph_weighted_rows", "sympa_graph_weighted_distortion_rows"):
        assert s in declared and s in _lib.SYMBOLS and hasattr(_lib.load(), s)
    assert declared == set(_lib.SYMBOLS)


def test_argument_validation_without_gpu():
    lib = _lib.load()
    al = ctypes.c_void_p(64)       # never dereferenced: validation happens before any launch
    N, E = 100, 400
    size = lib.sympa_graph_weighted_workspace_bytes
    assert size(N, 1) == size(N, 8) == 8 * (N + 1) * 8                  # sources in eights: [N][8] fp64 plane + one word per source
    assert size(N, 9) == 16 * (N + 1) * 8 and size(N, 100) == 104 * (N + 1) * 8
    assert size(45500, 320) == 320 * 45501 * 8
    assert size(0, 5) == 0 and size(-1, 5) == 0 and size(N, 0) == 0 and size(N, -2) == 0
    assert size(2 ** 31 - 1, 2 ** 31 - 1) == 2 ** 63 - 1                  # no int64 holds it: saturates, so every call is refused
    ws = size(N, 100)

    def call(rowptr=al, cols=al, weights=al, n=N, e=E, begin=0, count=100, out=al, stride=N, work=al, work_bytes=ws):
        return lib.sympa_graph_weighted_rows(rowptr, cols, weights, n, e, begin, count, out, stride, work, work_bytes, None, None)
    assert call(count=0) == 0                                   # an empty block is a no-op
    assert call(count=0, out=None, work=None, work_bytes=0) == 0
    assert call(rowptr=None) == -1 and b"null" in lib.sympa_last_error()
    assert call(cols=None) == -1
    assert call(weights=None) == -1 and b"null" in lib.sympa_last_error()
    assert call(out=None) == -1
    assert call(work=None) == -1 and b"workspace" in lib.sympa_last_error()
    assert call(n=0) == -1 and call(n=-3) == -1 and call(n=2 ** 31) == -1
    assert call(e=-1) == -1
    assert call(begin=-1) == -1 and call(begin=1) == -1 and call(count=101) == -1 and call(count=-1) == -1
    assert b"source block" in lib.sympa_last_error()
    assert call(stride=N - 1) == -1 and b"row_stride" in lib.sympa_last_error()
    assert call(work_bytes=ws - 1) == -1 and b"workspace" in lib.sympa_last_error()
    assert call(work_bytes=0) == -1 and call(work_bytes=-8) == -1
    assert call(work=ctypes.c_void_p(68)) == -1                 # not 8-byte aligned
    assert call(n=2 ** 31 - 1, count=2 ** 31 - 1, stride=2 ** 31 - 1, work_bytes=2 ** 63 - 1) == -1
    # the distortion rows
    d = lambda **k: lib.sympa_graph_weighted_distortion_rows(k.get("dist", al), k.get("ld", N), k.get("g", al), k.get("ldg", N),  # noqa: E731
                                                             k.get("begin", 0), k.get("count", 10), k.get("n", N), k.get("s", al),
                                                             k.get("p", al), None)
    assert d(count=0) == 0
    assert d(dist=None) == -1 and d(g=None) == -1 and d(s=None) == -1 and d(p=None) == -1
    assert d(n=0) == -1 and d(begin=95) == -1 and d(begin=-1) == -1 and d(ld=N - 1) == -1 and d(ldg=N - 1) == -1


def test_product_path_refuses_cpu_tensors():
    rowptr, cols, weights, _ = csr_of("grid-5x5x5", "ints")
    with pytest.raises(_lib.SympaHipError):
        ops.graph_weighted_rows(rowptr, cols, weights, 0, 125)
    with pytest.raises(_lib.SympaHipError):
        ops.graph_weighted_distortion_rows(torch.zeros(2, 125, dtype=torch.float64), torch.zeros(2, 125, dtype=torch.float64), 0)
