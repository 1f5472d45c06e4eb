"""Shared cases of tests/test_graph_weighted_cpu.py and tests/test_graph_weighted_gpu.py: small weighted graphs, their cleaned
CSR, and scipy's Dijkstra from every source over that CSR (computed once per case and never changed)."""
import functools

import networkx as nx
import numpy as np

from sympa_amd.graph import weighted_graph_csr

KINDS = ("ints", "wide", "unit")      # ints 1..5: massive ties; 10**U(-3, 3): the fold order matters; U(0.1, 1)


def draw(rng, kind, size):
    if kind == "ints":
        return rng.integers(1, 6, size).astype(np.float64)
    if kind == "wide":
        return 10.0 ** rng.uniform(-3.0, 3.0, size)
    return rng.uniform(0.1, 1.0, size)


def weigh(graph, kind, seed):
    """A copy of `graph` (same class: parallel edges and self-loops stay) with a seeded weight on every edge."""
    out = graph.__class__()
    out.add_nodes_from(graph.nodes())
    edges = list(graph.edges())
    for (u, v), w in zip(edges, draw(np.random.default_rng(seed), kind, len(edges))):
        out.add_edge(u, v, weight=float(w))
    return out


def geometric_and_cycle():
    return nx.disjoint_union(nx.random_geometric_graph(150, 0.14, seed=5), nx.cycle_graph(40))       # unreachable pairs


def heavy_edge_cycle(kind, seed):
    g = nx.cycle_graph(64)
    nx.set_edge_attributes(g, 1.0, "weight")
    g[0][63]["weight"] = 1000.0                # from 0, the hop-nearest route to 63 is not the lightest
    return g


def zero_weight_grid(kind, seed):
    g = nx.convert_node_labels_to_integers(nx.grid_2d_graph(9, 11))
    w = np.random.default_rng(seed).integers(0, 4, g.number_of_edges())      # about a quarter of the edges weigh exactly 0
    for (u, v), x in zip(list(g.edges()), w):
        g[u][v]["weight"] = float(x)
    g[0][1]["weight"] = -0.0
    return g


def seeded(build):
    return lambda kind, seed: weigh(build(), kind, seed)


GRAPHS = {
    "grid-5x5x5": (seeded(lambda: nx.grid_graph(dim=[5, 5, 5])), KINDS),
    "tree-b3-h6": (seeded(lambda: nx.balanced_tree(3, 6)), KINDS),           # N = 1 093: more than one stride of 1 024 lanes
    "path-300": (seeded(lambda: nx.path_graph(300)), KINDS),                 # N - 2 sweeps
    "geometric+cycle": (seeded(geometric_and_cycle), KINDS),
    "margulis-12": (seeded(lambda: nx.margulis_gabber_galil_graph(12)), KINDS),      # self-loops and parallel edges to clean
    "complete-70": (seeded(lambda: nx.complete_graph(70)), ("wide",)),      # dense rows, multi-hop shortest paths
    "heavy-edge-cycle": (heavy_edge_cycle, ("fixed",)),
    "zero-weights": (zero_weight_grid, ("fixed",)),
}
CASES = [(name, kind) for name, (_, kinds) in GRAPHS.items() for kind in kinds]
CASE_IDS = [f"{name}-{kind}" for name, kind in CASES]


@functools.lru_cache(maxsize=None)
def graph_of(name, kind):
    return GRAPHS[name][0](kind, 1000 + CASES.index((name, kind)))


@functools.lru_cache(maxsize=None)
def csr_of(name, kind):
    """(rowptr, cols, weights, id2node) CPU tensors of the case."""
    return weighted_graph_csr(graph_of(name, kind))


@functools.lru_cache(maxsize=None)
def dijkstra_of(name, kind):
    """fp64 [N, N] read-only: scipy's Dijkstra from every source over the case's cleaned CSR.  Row s is summed from s."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    rowptr, cols, weights, _ = csr_of(name, kind)
    N = rowptr.numel() - 1
    adj = csr_matrix((weights.numpy(), cols.numpy(), rowptr.numpy()), shape=(N, N))
    out = dijkstra(adj, directed=False, indices=np.arange(N))
    out.setflags(write=False)
    return out
