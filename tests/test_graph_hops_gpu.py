"""GPU: graph hop distances on the device (csrc/graph_bfs.hip through ops.graph_hop_rows and sympa_amd.graph.GraphDistances)
against the numpy restatement of the same algorithm (graph.host_hop_rows), networkx BFS and data.graph_triplets, and the
all-pairs distortion built on them (Model.evaluate_all_pairs) against Model.evaluate over the listed triplets.
Reference: preprocess.py:53-60,101-126, sympa/metrics.py:21, sympa/runner.py:124-135."""
import functools
import os
import re
import socket
import subprocess
import sys

import networkx as nx
import numpy as np
import pytest
import torch

from sympa_amd import data, ops
from sympa_amd.graph import GraphDistances, graph_csr, host_hop_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "gpu_graph_worker.py")
DEV = torch.device("cuda:0")
BIG = "product-cartesian-45500"


def two_components_and_an_isolated_node():
    g = nx.disjoint_union(nx.cycle_graph(9), nx.balanced_tree(2, 3))
    g.add_node(g.number_of_nodes())
    return g


GRAPHS = {
    "grid3d-125": lambda: data.named_graph("grid3d-125"),
    "tree-b3-h6": lambda: data.named_graph("tree-b3-h6"),
    "margulis-71": lambda: data.named_graph("margulis-71"),
    "two-components": two_components_and_an_isolated_node,
    "path-300": lambda: nx.path_graph(300),
    "star-500": lambda: nx.star_graph(500),
    "path-1000": lambda: nx.path_graph(1000),
    "star-5000": lambda: nx.star_graph(5000),
    BIG: lambda: data.named_graph(BIG),
}


@functools.lru_cache(maxsize=None)
def csr_of(name):
    return graph_csr(GRAPHS[name]())


@functools.lru_cache(maxsize=None)
def host_rows_of(name):
    rowptr, cols, _ = csr_of(name)
    return torch.from_numpy(host_hop_rows(rowptr, cols, 0, rowptr.numel() - 1))


def device_csr(name):
    rowptr, cols, _ = csr_of(name)
    return rowptr.to(DEV), cols.to(DEV)


def blocked_rows(rowptr, cols, size):
    """All rows through calls of `size` sources each, into a matrix pre-filled with a value the kernel never writes."""
    N = rowptr.numel() - 1
    out = torch.full((N, N), -7, dtype=torch.int32, device=DEV)
    for b in range(0, N, size):
        r = min(size, N - b)
        ops.graph_hop_rows(rowptr, cols, b, r, out=out[b:b + r])
    return out


@pytest.mark.parametrize("name", [n for n in GRAPHS if n != BIG])
def test_kernel_rows_equal_the_host_restatement(name):
    rowptr, cols = device_csr(name)
    N = rowptr.numel() - 1
    got = blocked_rows(rowptr, cols, N)
    assert ops.check_status(DEV) == (0, 0)
    assert torch.equal(got.cpu(), host_rows_of(name))


@pytest.mark.parametrize("name", ["tree-b3-h6", "two-components", "path-1000"])
def test_every_blocking_of_the_sources_gives_the_same_rows(name):
    rowptr, cols = device_csr(name)
    N = rowptr.numel() - 1
    want = host_rows_of(name)
    for size in (1, 63, 64, 65, 1000, N):
        assert torch.equal(blocked_rows(rowptr, cols, size).cpu(), want), size
    assert ops.check_status(DEV) == (0, 0)


def test_a_padded_output_keeps_its_padding():
    rowptr, cols = device_csr("grid3d-125")
    wide = torch.full((125, 160), -7, dtype=torch.int32, device=DEV)
    ops.graph_hop_rows(rowptr, cols, 0, 125, out=wide[:, :125])
    assert torch.equal(wide[:, :125].cpu(), host_rows_of("grid3d-125")) and (wide[:, 125:] == -7).all()


def test_a_planted_column_outside_the_graph_is_reported_and_changes_no_row():
    rowptr, cols, _ = csr_of("tree-b3-h6")
    rp, c = rowptr.numpy().copy(), cols.numpy()
    c = np.concatenate((c[:rp[41]], [rp.size + 5], c[rp[41]:])).astype(np.int32)       # one extra entry at the end of row 40
    rp[41:] += 1
    N = rp.size - 1
    got = ops.graph_hop_rows(torch.from_numpy(rp).to(DEV), torch.from_numpy(c).to(DEV), 0, N)
    with pytest.raises(IndexError, match=r"\(1 pairs flagged\)"):
        ops.check_status(DEV)
    assert ops.check_status(DEV) == (0, 0)
    assert torch.equal(got.cpu(), host_rows_of("tree-b3-h6"))


@pytest.mark.parametrize("name", ["grid3d-125", "tree-b3-h6", "margulis-71"])
def test_device_triplets_and_neighbours_equal_graph_triplets(name):
    rowptr, cols, id2node = csr_of(name)
    want, want_ids = data.graph_triplets(data.named_graph(name))
    N = rowptr.numel() - 1
    gd = GraphDistances(rowptr, cols, device=DEV, max_block_bytes=4 * N * 200)          # several ragged blocks
    got = gd.triplets()
    assert got.is_cuda and got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    assert id2node == want_ids
    nb = gd.neighbor_csr()
    want_nb = ops.neighbor_csr(want[:, :2].to(DEV), want[:, 2].to(DEV), N)
    assert torch.equal(nb[0], want_nb[0]) and torch.equal(nb[1], want_nb[1])
    assert ops.check_status(DEV) == (0, 0)


def test_pairs_on_the_device_equal_the_rows():
    rowptr, cols, _ = csr_of("two-components")
    gd = GraphDistances(rowptr, cols, device=DEV)
    got = gd.pairs(torch.tensor([[0, 4], [0, 9], [24, 0], [9, 10], [3, 3]]))
    assert got.is_cuda and got.tolist() == [4.0, float("inf"), float("inf"), 1.0, 0.0]


def test_the_product_graph_of_configs3_fits_and_is_right():
    rowptr, cols, _ = csr_of(BIG)
    N = rowptr.numel() - 1
    assert N == 45500
    block = 128 << 20
    gd = GraphDistances(rowptr, cols, device=DEV, max_block_bytes=block)
    csr_bytes = gd.rowptr.numel() * 8 + gd.cols.numel() * 4
    # 8 source rows against networkx BFS
    g = nx.convert_node_labels_to_integers(data.named_graph(BIG), ordering="sorted")
    sources = [0, 1, 124, 125, 20000, 33333, N - 2, N - 1]
    for s in sources:
        want = np.full(N, -1, dtype=np.int32)
        for v, d in nx.single_source_shortest_path_length(g, s).items():
            want[v] = d
        assert np.array_equal(gd.rows(s, 1).cpu().numpy()[0], want), s
    # sampled pairs: symmetric, and equal to the row values
    ids = data.sample_pairs(N, 10000, batch_id=1).to(DEV)
    d = gd.pairs(ids)
    assert torch.equal(d, gd.pairs(ids.flip(1)))
    assert d.min().item() >= 1.0 and d.max().item() <= 22.0
    for k in (0, 17, 4242, 9999):
        i, j = ids[k].tolist()
        assert gd.rows(i, 1)[0, j].item() == d[k].item()
    gd.release()
    # every row once, within the memory budget: one block + its workspace + the CSR
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    top = torch.zeros((), dtype=torch.int32, device=DEV)
    low = torch.zeros((), dtype=torch.int32, device=DEV)
    rows_seen = 0
    for b, rows in gd.blocks():
        top = torch.maximum(top, rows.max())
        low = torch.minimum(low, rows.min())
        rows_seen += rows.shape[0]
    top, low = int(top), int(low)
    peak = torch.cuda.max_memory_allocated() - base
    assert rows_seen == N
    assert top == 22 and low == 0                  # tree diameter 10 + grid diameter 12; connected: no -1
    workspace = ops.graph_hops_workspace_bytes(N, gd.block_rows)
    assert workspace == gd.workspace_bytes() == (gd.block_rows // 64) * 24 * N
    assert gd.block_rows * 4 * N <= block
    # (the CSR is resident before the measurement starts: it is part of `base` on both sides of the issue's bound)
    assert base >= csr_bytes and peak <= block + workspace + (64 << 20), (peak, block, workspace, csr_bytes)
    assert ops.check_status(DEV) == (0, 0)
    # ... and too many triplets to list: refused with the count
    with pytest.raises(MemoryError, match="1035102250 triplets"):
        gd.triplets()


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


def test_all_pairs_distortion_equals_evaluate_over_the_triplets():
    """tree-b3-h6, upper, riem, n = 4, trained-like table: T = 596 778 triplets.  Both values are fp64 sums of the same T
    non-negative terms in different orders, so they differ by at most T * 2^-53 relative (the worst-case reordering bound)."""
    rowptr, cols, _ = csr_of("tree-b3-h6")
    N = rowptr.numel() - 1
    trip, _ = data.graph_triplets(data.named_graph("tree-b3-h6"))
    T = trip.shape[0]
    assert T == 596778
    m = make_model("upper", "riem", 4, data.trained_like_table(N, 4, seed=3))
    want = m.evaluate(trip[:, :2].contiguous().to(DEV), trip[:, 2].to(torch.float64).to(DEV), 65536)
    gd = GraphDistances(rowptr, cols, device=DEV)
    got = m.evaluate_all_pairs(gd)
    rel = abs(got - want) / abs(want)
    print(f"evaluate_all_pairs {got!r} evaluate {want!r} relative difference {rel:.3e} bound {T * 2.0 ** -53:.3e}")
    assert rel <= T * 2.0 ** -53
    # two block sizes: bitwise
    small = m.evaluate_all_pairs(gd, max_block_bytes=12 * N * 128)
    odd = m.evaluate_all_pairs(GraphDistances(rowptr, cols, device=DEV, max_block_bytes=4 * N * 64), max_block_bytes=12 * N * 320)
    assert got == small == odd
    assert ops.check_status(DEV) == (0, 0)


def test_all_pairs_distortion_skips_unreachable_pairs():
    rowptr, cols, _ = csr_of("two-components")
    N = rowptr.numel() - 1
    trip, _ = data.graph_triplets(two_components_and_an_isolated_node())
    m = make_model("bounded", "finf", 3, data.trained_like_table(N, 3, model="bounded", seed=11))
    want = m.evaluate(trip[:, :2].contiguous().to(DEV), trip[:, 2].to(torch.float64).to(DEV), 64)
    got = m.evaluate_all_pairs(GraphDistances(rowptr, cols, device=DEV))
    assert abs(got - want) <= trip.shape[0] * 2.0 ** -53 * abs(want)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_give_bitwise_the_single_process_distortion(tmp_path):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["OMP_NUM_THREADS"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), WORKER, "distortion", str(tmp_path)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600, cwd=ROOT)
    assert proc.returncode == 0, proc.stderr.decode(errors="replace")[-3000:]
    got = torch.load(os.path.join(str(tmp_path), "distortion_w2.pt"))
    assert got["world"] == 2
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_graph_worker as w
    S = w.SHAPE
    gd = w.graph_distances(S["graph"], DEV, S["block_rows"])
    m = w.graph_model(S["manifold"], S["metric"], S["dims"], gd.num_nodes, S["seed"], DEV)
    assert got["distortion"] == m.evaluate_all_pairs(gd)


def test_sampled_pairs_training_runs_three_steps_in_a_child_process():
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_siegel.py"), "--graph", "grid3d-125", "--dims", "2",
           "--sampled-pairs", "192", "--batch_size", "64", "--epochs", "1", "--val_every", "1"]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert proc.returncode == 0, proc.stderr.decode(errors="replace")[-3000:]
    out = proc.stdout.decode()
    m = re.search(r"epoch\s+1\s+loss/triplet (\S+)\s+avg distortion (\S+)", out)
    assert m, out
    loss, distortion = float(m.group(1)), float(m.group(2))
    assert np.isfinite(loss) and loss > 0.0 and np.isfinite(distortion) and distortion > 0.0
