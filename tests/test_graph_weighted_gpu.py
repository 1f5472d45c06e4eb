"""GPU: weighted shortest-path distances on the device (csrc/graph_sssp.hip through ops.graph_weighted_rows and
sympa_amd.graph.WeightedGraphDistances) against the numpy restatement of the same fixed point (graph.host_weighted_rows), scipy's
Dijkstra and the merged hop kernel, and the all-pairs distortion built on them (Model.evaluate_all_pairs) against Model.evaluate
over the listed weighted triplets.  Rows are compared bit for bit: the result is unique.
Reference: preprocess.py:76-86,108-126, sympa/metrics.py:21, sympa/runner.py:124-135."""
import functools
import os
import re
import subprocess
import sys

import networkx as nx
import numpy as np
import pytest
import torch

from sympa_amd import data, ops
from sympa_amd.graph import GraphDistances, WeightedGraphDistances, graph_csr, host_weighted_rows, weighted_graph_csr
from tests.graph_weighted_cases import CASE_IDS, CASES, csr_of, dijkstra_of, graph_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
SENTINEL = -7.25                                     # a value the kernel never writes


@functools.lru_cache(maxsize=None)
def host_rows_of(name, kind):
    rowptr, cols, weights, _ = csr_of(name, kind)
    return torch.from_numpy(host_weighted_rows(rowptr, cols, weights, 0, rowptr.numel() - 1))


def device_csr(name, kind):
    rowptr, cols, weights, _ = csr_of(name, kind)
    return rowptr.to(DEV), cols.to(DEV), weights.to(DEV)


def same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64))


def blocked_rows(csr, size, begin=0):
    """Rows begin .. N - 1 through calls of `size` sources each, into a matrix pre-filled with the sentinel."""
    N = csr[0].numel() - 1
    out = torch.full((N - begin, N), SENTINEL, dtype=torch.float64, device=DEV)
    for b in range(begin, N, size):
        r = min(size, N - b)
        ops.graph_weighted_rows(*csr, b, r, out=out[b - begin:b - begin + r])
    return out


@pytest.mark.parametrize("name,kind", CASES, ids=CASE_IDS)
def test_kernel_rows_equal_the_host_restatement(name, kind):
    csr = device_csr(name, kind)
    got = blocked_rows(csr, csr[0].numel() - 1)
    assert ops.check_status(DEV) == (0, 0)
    assert same_bits(got, host_rows_of(name, kind))


@pytest.mark.parametrize("name,kind", [("tree-b3-h6", "wide"), ("complete-70", "wide")])
def test_kernel_rows_equal_scipy_dijkstra(name, kind):
    rowptr, cols, weights = device_csr(name, kind)
    N = rowptr.numel() - 1
    got = ops.graph_weighted_rows(rowptr, cols, weights, 0, N)
    assert same_bits(got, torch.from_numpy(np.array(dijkstra_of(name, kind))))
    assert ops.check_status(DEV) == (0, 0)


@pytest.mark.parametrize("name,kind", [("tree-b3-h6", "wide"), ("geometric+cycle", "unit"), ("path-300", "ints")])
def test_every_blocking_of_the_sources_gives_the_same_rows(name, kind):
    csr = device_csr(name, kind)
    N = csr[0].numel() - 1
    want = host_rows_of(name, kind)
    for size in (1, 63, 64, 65, N):
        assert same_bits(blocked_rows(csr, size), want), size
    assert same_bits(blocked_rows(csr, 61, begin=5), want[5:])           # src_begin neither 0 nor a multiple of a group
    assert ops.check_status(DEV) == (0, 0)


def test_the_workspace_keeps_the_sweeps_of_every_group():
    csr = device_csr("tree-b3-h6", "unit")
    N = csr[0].numel() - 1
    ws = torch.zeros(ops.graph_weighted_workspace_bytes(N, 13) // 8, dtype=torch.int64, device=DEV)
    got = ops.graph_weighted_rows(*csr, 7, 13, workspace=ws)
    assert same_bits(got, host_rows_of("tree-b3-h6", "unit")[7:20])
    sweeps = ws[-16:].tolist()                                           # one word per source behind the planes
    assert sweeps[:13] == ops.graph_weighted_sweeps(ws, N, 13).tolist()
    assert all(2 <= s <= N for s in sweeps[:13]) and sweeps[13:] == [0, 0, 0], sweeps
    assert all(sweeps[g] == sweeps[g // 8 * 8] for g in range(13))        # one count per group of 8 sources
    assert ops.check_status(DEV) == (0, 0)


def test_a_padded_output_keeps_its_padding():
    csr = device_csr("grid-5x5x5", "wide")
    wide = torch.full((125, 160), SENTINEL, dtype=torch.float64, device=DEV)
    ops.graph_weighted_rows(*csr, 0, 125, out=wide[:, :125])
    assert same_bits(wide[:, :125], host_rows_of("grid-5x5x5", "wide")) and (wide[:, 125:] == SENTINEL).all()
    tall = torch.full((130, 125), SENTINEL, dtype=torch.float64, device=DEV)
    ops.graph_weighted_rows(*csr, 20, 70, out=tall[3:])                  # rows beyond the block stay too
    assert same_bits(tall[3:73], host_rows_of("grid-5x5x5", "wide")[20:90])
    assert (tall[:3] == SENTINEL).all() and (tall[73:] == SENTINEL).all()


@pytest.mark.parametrize("name", ["tree-b3-h6", "two-components"])
def test_unit_weights_give_the_rows_of_the_hop_kernel(name):
    g = nx.balanced_tree(3, 6) if name == "tree-b3-h6" else nx.disjoint_union(nx.cycle_graph(9), nx.balanced_tree(2, 3))
    rowptr, cols, _ = graph_csr(g)
    nx.set_edge_attributes(g, 1.0, "weight")
    w_rowptr, w_cols, weights, _ = weighted_graph_csr(g)
    assert torch.equal(rowptr, w_rowptr) and torch.equal(cols, w_cols)
    N = rowptr.numel() - 1
    hops = ops.graph_hop_rows(rowptr.to(DEV), cols.to(DEV), 0, N).to(torch.float64)
    hops[hops < 0] = float("inf")
    got = ops.graph_weighted_rows(rowptr.to(DEV), cols.to(DEV), weights.to(DEV), 0, N)
    assert same_bits(got, hops)
    assert ops.check_status(DEV) == (0, 0)


def planted(name, kind, col, weight, row=40):
    """The case's CSR with one extra entry (col, weight) at the end of row `row`."""
    rowptr, cols, weights, _ = csr_of(name, kind)
    rp = rowptr.numpy().copy()
    at = rp[row + 1]
    c = np.concatenate((cols.numpy()[:at], [col], cols.numpy()[at:])).astype(np.int32)
    w = np.concatenate((weights.numpy()[:at], [weight], weights.numpy()[at:]))
    rp[row + 1:] += 1
    return torch.from_numpy(rp).to(DEV), torch.from_numpy(c).to(DEV), torch.from_numpy(w).to(DEV)


def test_a_planted_column_outside_the_graph_is_reported_and_changes_no_row():
    rowptr, cols, weights = planted("tree-b3-h6", "unit", 1093 + 5, 0.5)
    got = ops.graph_weighted_rows(rowptr, cols, weights, 0, 1093)
    with pytest.raises(IndexError, match=r"\(1 pairs flagged\)"):
        ops.check_status(DEV)
    assert ops.check_status(DEV) == (0, 0)
    assert same_bits(got, host_rows_of("tree-b3-h6", "unit"))


@pytest.mark.parametrize("weight", [float("nan"), -1.0, float("inf")])
def test_a_planted_bad_weight_is_reported_and_changes_no_row(weight):
    rowptr, cols, weights = planted("tree-b3-h6", "unit", 7, weight)      # a legal column: only the weight is wrong
    got = ops.graph_weighted_rows(rowptr, cols, weights, 0, 1093)
    assert ops._status_buf(DEV).tolist() == [ops.ST_NONFINITE, 1]
    with pytest.raises(AssertionError, match="1 pairs"):
        ops.check_status(DEV)
    assert ops.check_status(DEV) == (0, 0)
    assert same_bits(got, host_rows_of("tree-b3-h6", "unit"))


@pytest.mark.parametrize("name,kind", [("grid-5x5x5", "ints"), ("geometric+cycle", "wide"), ("tree-b3-h6", "unit")])
def test_device_triplets_pairs_and_neighbours_equal_the_cpu_tensor_results(name, kind):
    rowptr, cols, weights, _ = csr_of(name, kind)
    N = rowptr.numel() - 1
    cpu = WeightedGraphDistances(rowptr, cols, weights)
    gd = WeightedGraphDistances(rowptr, cols, weights, device=DEV, max_block_bytes=8 * N * 200)          # several ragged blocks
    assert gd.block_rows == min(192, -(-N // 64) * 64)
    ids, dist = gd.triplets()
    want_ids, want_dist = cpu.triplets()
    assert ids.is_cuda and dist.is_cuda and torch.equal(ids.cpu(), want_ids) and same_bits(dist, want_dist)
    assert gd.count_triplets() == want_ids.shape[0]
    pairs = data.sample_pairs(N, 2000, batch_id=4)
    got = gd.pairs(pairs)
    assert got.is_cuda and same_bits(got, cpu.pairs(pairs))
    nb, want_nb = gd.neighbor_csr(), cpu.neighbor_csr()
    assert torch.equal(nb[0].cpu(), want_nb[0]) and torch.equal(nb[1].cpu(), want_nb[1])
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


def test_all_pairs_distortion_equals_evaluate_over_the_weighted_triplets(monkeypatch):
    """Weighted tree-b3-h6 (weights U(0.1, 1)), upper, riem, n = 4, trained-like table: T = 596 778 triplets.  evaluate() and
    evaluate_all_pairs() are fp64 sums of the same T non-negative terms in different orders, so they differ by at most T * 2^-53
    relative (the worst-case reordering bound, the one the hop test uses)."""
    rowptr, cols, weights, _ = csr_of("tree-b3-h6", "unit")
    N = rowptr.numel() - 1
    ids, dist = WeightedGraphDistances(rowptr, cols, weights, device=DEV).triplets()
    T = ids.shape[0]
    assert T == 596778
    m = make_model("upper", "riem", 4, data.trained_like_table(N, 4, seed=3))
    want = m.evaluate(ids.contiguous(), dist, 65536)
    gd = WeightedGraphDistances(rowptr, cols, weights, device=DEV)
    got = m.evaluate_all_pairs(gd)
    rel = abs(got - want) / abs(want)
    print(f"evaluate_all_pairs {got!r} evaluate {want!r} relative difference {rel:.3e} bound {T * 2.0 ** -53:.3e}")
    assert rel <= T * 2.0 ** -53
    # two block sizes: bitwise
    small = m.evaluate_all_pairs(gd, max_block_bytes=16 * N * 128)
    odd = m.evaluate_all_pairs(WeightedGraphDistances(rowptr, cols, weights, device=DEV, max_block_bytes=8 * N * 64),
                               max_block_bytes=16 * N * 320)
    assert got == small == odd
    # the two halves distributed.row_shard gives two ranks, one after the other in this process: the zero-padded per-row vectors
    # each shard hands to the all-reduce (taken here in its place) add up, bit for bit, to those of the whole
    from sympa_amd import distributed as sd
    per = -(-N // 2)
    vectors = {}
    for shard in ((0, N), (0, per), (per, N - per)):
        monkeypatch.setattr(sd, "row_shard", lambda n, group=None: shard)
        monkeypatch.setattr(sd, "allreduce_row_shards", lambda t, group=None: vectors.setdefault(shard, []).append(t.clone()) or t)
        value = m.evaluate_all_pairs(gd, group="one process")
        if shard == (0, N):
            assert value == got
    monkeypatch.undo()
    for whole, a, b in zip(vectors[(0, N)], vectors[(0, per)], vectors[(per, N - per)]):
        assert (a[per:] == 0).all() and (b[:per] == 0).all() and torch.equal(a + b, whole)
    sums, pairs = vectors[(0, N)]
    assert sums.dtype == torch.float64 and pairs.dtype == torch.int64 and int(pairs.sum()) == T
    assert ops.check_status(DEV) == (0, 0)


def test_all_pairs_distortion_skips_unreachable_pairs():
    rowptr, cols, weights, _ = csr_of("geometric+cycle", "unit")
    N = rowptr.numel() - 1
    gd = WeightedGraphDistances(rowptr, cols, weights, device=DEV)
    ids, dist = gd.triplets()
    T = ids.shape[0]
    assert 0 < T < N * (N - 1) // 2 and torch.isfinite(dist).all()
    m = make_model("bounded", "finf", 3, data.trained_like_table(N, 3, model="bounded", seed=11))
    want = m.evaluate(ids.contiguous(), dist, 4096)
    got = m.evaluate_all_pairs(gd)
    assert abs(got - want) <= T * 2.0 ** -53 * abs(want)
    with pytest.raises(ValueError, match="nodes"):
        m.evaluate_all_pairs(WeightedGraphDistances(*csr_of("grid-5x5x5", "unit")[:3], device=DEV))


def test_the_hop_distances_still_take_their_own_path():
    """A GraphDistances goes through the int32 rows and ops.graph_distortion_rows as before; with unit weights the two paths sum
    the same terms row by row in the same order, so the two values are bitwise equal."""
    g = nx.grid_graph(dim=[5, 5, 5])
    rowptr, cols, _ = graph_csr(g)
    m = make_model("upper", "riem", 2, data.trained_like_table(125, 2, seed=5))
    hop = m.evaluate_all_pairs(GraphDistances(rowptr, cols, device=DEV))
    unit = m.evaluate_all_pairs(WeightedGraphDistances(rowptr, cols, torch.ones(cols.numel(), dtype=torch.float64), device=DEV))
    assert hop == unit


@pytest.mark.parametrize("extra", [[], ["--sampled-pairs", "192", "--batch_size", "64"]], ids=["listed", "sampled"])
def test_training_on_an_edges_file_runs_one_epoch_in_a_child_process(tmp_path, extra):
    g = nx.convert_node_labels_to_integers(graph_of("grid-5x5x5", "unit"), ordering="sorted")
    path = tmp_path / "weighted-grid.edges"
    path.write_text("".join(f"{u} {v} {d['weight']!r}\n" for u, v, d in g.edges(data=True)))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_siegel.py"), "--edges", str(path), "--dims", "2", "--epochs", "1",
           "--val_every", "1"] + extra
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert proc.returncode == 0, proc.stderr.decode(errors="replace")[-3000:]
    out = proc.stdout.decode()
    m = re.search(r"epoch\s+1\s+loss/triplet (\S+)\s+avg distortion (\S+)", out)
    assert m, out
    loss, distortion = float(m.group(1)), float(m.group(2))
    assert np.isfinite(loss) and loss > 0.0 and np.isfinite(distortion) and distortion > 0.0
