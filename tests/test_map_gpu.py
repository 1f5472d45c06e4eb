"""GPU: mean average precision on the device (csrc/map_rank.hip through ops.map_rows, Model.mean_average_precision) against the
numpy restatement of the same rule (sympa_amd.metrics.host_average_precision) and against the reference's own fixtures
(tests/golden/map_*.npz, tools/make_golden_map.py).  Reference: sympa/metrics.py:25-63, sympa/runner.py:137-154."""
import functools
import glob
import os
import socket
import subprocess
import sys
import time

import networkx as nx
import numpy as np
import pytest
import torch
from torch.utils.data import TensorDataset

from sympa_amd import data, ops
from sympa_amd.metrics import MeanAveragePrecisionMetric, host_average_precision
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "gpu_map_worker.py")
MAP_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "map_*.npz")))
DEV = torch.device("cuda:0")


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


@functools.lru_cache(maxsize=None)
def triples_of(graph):
    g = data.named_graph(graph) if isinstance(graph, str) else graph()
    trip, _ = data.graph_triplets(g)
    return trip[:, :2].contiguous(), trip[:, 2].to(torch.float32)


def csr_of(ids, dists, N, dev=DEV):
    m = MeanAveragePrecisionMetric((ids.to(dev), dists.to(dev)))
    return m, m.csr(N, dev)


def row_matrix(m):
    """The full matrix as row-oriented values: row i computed with i as the source (no mirrored half)."""
    if m.manifold.model_name == "spd":
        return m.distance_matrix()
    table = m.embeddings.embeds.detach()
    w = m.manifold.metric.weights if m.manifold.metric.kind.value == "wsum" else None
    return ops.all_pairs_dist(table, m.manifold.model_name, m.manifold.metric.kind.value, w, m.scale.detach(), m.scale_coef,
                              flags=ops.FLAG_NO_SYMMETRY)


def restated(rows, nbrs, float32):
    d = rows.cpu().numpy()
    d = d.astype(np.float32) if float32 else d
    return host_average_precision(d, nbrs[0].cpu().numpy(), nbrs[1].cpu().numpy())


def assert_ap_equal(got, want, rtol=1e-14):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), "NaN rows differ"
    if (~nan).any():
        err = np.abs(got[~nan] - want[~nan]) / np.abs(want[~nan])
        assert err.max() <= rtol, f"max rel err {err.max():.3e} at row {np.flatnonzero(~nan)[err.argmax()]}"


KERNEL_CASES = [
    ("grid3d-125", "upper", "riem", 2),
    ("grid3d-125", "bounded", "wsum", 12),
    ("tree-b3-h6", "upper", "finf", 4),
    ("tree-b3-h6", "bounded", "riem", 8),
    ("tree-b3-h6", "upper", "wsum", 12),
    ("margulis-71", "upper", "wsum", 8),
    ("margulis-71", "bounded", "finf", 4),
    ("grid3d-125", "bounded", "riem", 2),
]


@pytest.mark.parametrize("float32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("graph,model,metric,n", KERNEL_CASES)
def test_kernel_matches_the_stable_restatement_on_every_row(graph, model, metric, n, float32):
    ids, dists = triples_of(graph)
    N = int(ids.max()) + 1
    m = make_model(model, metric, n, data.trained_like_table(N, n, model=model, seed=5))
    _, nbrs = csr_of(ids, dists, N)
    rows = row_matrix(m)
    got = ops.map_rows(rows, 0, nbrs, float32=float32)
    ops.check_status(DEV)
    assert_ap_equal(got, restated(rows, nbrs, float32))


@pytest.mark.parametrize("float32", [False, True], ids=["fp64", "fp32"])
def test_kernel_matches_the_restatement_on_spd_n16(float32):
    ids, dists = triples_of(lambda: nx.balanced_tree(2, 6))
    N = int(ids.max()) + 1
    m = make_model("spd", "riem", 16, data.spd_table(N, 16, seed=3))
    _, nbrs = csr_of(ids, dists, N)
    rows = row_matrix(m)
    got = ops.map_rows(rows, 0, nbrs, float32=float32)
    ops.check_status(DEV)
    assert_ap_equal(got, restated(rows, nbrs, float32))


def host_ranks(rows, nb_row, nb_col, float32):
    d = rows.cpu().numpy()
    d = d.astype(np.float32) if float32 else d
    out = []
    for i, c in zip(nb_row, nb_col):
        order = np.argsort(d[i], kind="stable")
        order = np.concatenate(([i], order[order != i]))
        out.append(int(np.flatnonzero(order == c)[0]))
    return np.array(out)


@pytest.mark.parametrize("sfx", ["", "64"], ids=["float32", "float64"])
@pytest.mark.parametrize("path", MAP_FIXTURES, ids=[os.path.basename(p) for p in MAP_FIXTURES])
def test_model_map_reproduces_the_reference_fixture(path, sfx):
    f = np.load(path)
    model, metric = str(f["model"]), str(f["metric"])
    table = torch.from_numpy(f["table"])
    m = make_model(model, metric, table.shape[-1], table, float(f["scale_init"]), float(f["scale_coef"]))
    triples = TensorDataset(torch.from_numpy(f["ids"]).to(DEV), torch.from_numpy(f["dists"]).to(DEV))
    float32 = sfx == ""
    value, ap = m.mean_average_precision(triples, dtype=torch.float32 if float32 else torch.float64, return_rows=True)
    ops.check_status(DEV)
    assert_ap_equal(ap, f["ap" + sfx], rtol=1e-12)
    assert abs(value - float(f["map" + sfx])) <= 1e-12 * abs(float(f["map" + sfx]))
    # the reference's neighbour ranks, exactly, from the device's own rows
    ranks = host_ranks(row_matrix(m), f["nb_row"], f["nb_col"], float32)
    np.testing.assert_array_equal(ranks, f["nb_rank" + sfx])


@pytest.mark.parametrize("float32", [False, True], ids=["fp64", "fp32"])
def test_ties_from_duplicated_table_rows_follow_the_column_rule(float32):
    """Row 0 of a binary tree: 1 is a neighbour, 5 a bitwise duplicate of it (not a neighbour), 6 a duplicate of row 0 itself."""
    ids, dists = triples_of(lambda: nx.balanced_tree(2, 4))
    N = int(ids.max()) + 1
    table = data.trained_like_table(N, 2, seed=8)
    table[5] = table[1]
    table[6] = table[0]
    m = make_model("upper", "riem", 2, table)
    metric, nbrs = csr_of(ids, dists, N)
    assert 1 in metric.neighbors[0] and 5 not in metric.neighbors[0] and 6 not in metric.neighbors[0]
    rows = row_matrix(m)
    assert rows[0, 5].item() == rows[0, 1].item() and rows[0, 6].item() == 0.0
    got = ops.map_rows(rows, 0, nbrs, float32=float32)
    want = restated(rows, nbrs, float32)
    assert_ap_equal(got, want)
    # row 0: column 6 (distance 0, like self) comes first, the neighbour 1 ties 5 and wins by index
    assert got[0].item() == want[0]


@pytest.mark.parametrize("float32", [False, True], ids=["fp64", "fp32"])
def test_high_degree_hub_goes_through_the_workspace_path(float32):
    ids, dists = triples_of(lambda: nx.star_graph(ops.MAP_LDS_CAP + 300))
    N = int(ids.max()) + 1
    metric, nbrs = csr_of(ids, dists, N)
    assert metric.max_degree > ops.MAP_LDS_CAP and ops.map_workspace_bytes(N, metric.max_degree) > 0
    m = make_model("upper", "riem", 2, data.trained_like_table(N, 2, seed=6))
    rows = row_matrix(m)
    got = ops.map_rows(rows, 0, nbrs, float32=float32, max_degree=metric.max_degree)
    ops.check_status(DEV)
    assert_ap_equal(got, restated(rows, nbrs, float32))


def test_isolated_node_gives_nan_for_its_row_and_for_map():
    g = nx.path_graph(30)
    g.add_node(30)
    ids, dists = triples_of(lambda: g)
    assert int(ids.max()) == 29
    m = make_model("upper", "riem", 2, data.trained_like_table(31, 2, seed=2))
    value, ap = m.mean_average_precision((ids.to(DEV), dists.to(DEV)), return_rows=True)
    assert np.isnan(value) and torch.isnan(ap[30]) and not torch.isnan(ap[:30]).any()


@pytest.mark.parametrize("model,n", [("upper", 4), ("bounded", 12), ("spd", 16)])
def test_block_size_does_not_change_any_row(model, n):
    ids, dists = triples_of("tree-b3-h6" if model != "spd" else (lambda: nx.balanced_tree(3, 5)))
    N = int(ids.max()) + 1
    table = data.spd_table(N, n, seed=4) if model == "spd" else data.trained_like_table(N, n, model=model, seed=4)
    m = make_model(model, "riem", n, table)
    metric = MeanAveragePrecisionMetric((ids.to(DEV), dists.to(DEV)))
    one, ap1 = m.mean_average_precision(metric, return_rows=True)
    row_bytes = (40 if model == "spd" else 8) * N
    rows_per_block = N // 5 - 1                                  # >= 6 blocks, the last one ragged
    assert N % rows_per_block != 0
    many, ap2 = m.mean_average_precision(metric, max_block_bytes=rows_per_block * row_bytes, return_rows=True)
    assert torch.equal(ap1, ap2) and one == many


def test_scale_configs3_shape_stays_within_the_block_budget():
    """N = 45 500, n = 8 (configs[3]'s table) with a 256 MiB block: 62 blocks; neighbours from a 182 x 250 grid."""
    N, n, block = 45500, 8, 256 << 20
    W = 250
    i = torch.arange(N)
    right = torch.stack((i[(i % W) < W - 1], i[(i % W) < W - 1] + 1), 1)
    down = torch.stack((i[i + W < N], i[i + W < N] + W), 1)
    far = torch.stack((i, (i * 7919 + 13) % N), 1)              # graph distance 2: not neighbours
    ids = torch.cat((right, down, far)).to(DEV)
    dists = torch.cat((torch.ones(right.shape[0] + down.shape[0]), torch.full((N,), 2.0))).to(DEV)
    m = make_model("upper", "riem", n, data.trained_like_table(N, n, seed=42))
    metric = MeanAveragePrecisionMetric((ids, dists))
    metric.csr(N, DEV)
    del ids, dists
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    value, ap = m.mean_average_precision(metric, max_block_bytes=block, return_rows=True)
    elapsed = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated() - base
    from sympa_amd import _lib
    pack = _lib.load().sympa_all_pairs_workspace_bytes(N, n, 0)
    csr = sum(t.numel() * t.element_size() for t in metric.csr(N, DEV))
    assert peak <= block + csr + pack + 8 * N + (16 << 20), (peak, block, csr, pack)
    assert elapsed < 120.0, elapsed
    assert 0.0 < value <= 1.0 and not torch.isnan(ap).any()
    # spot rows against the restatement
    nbrs = metric.csr(N, DEV)
    for b in (0, 20000, N - 3):
        rows = m.distance_matrix(b, 3)
        d = rows.cpu().numpy().astype(np.float32)
        rp, cl = nbrs[0].cpu().numpy(), nbrs[1].cpu().numpy()
        for k in range(3):
            nb = cl[rp[b + k]:rp[b + k + 1]]
            order = np.argsort(d[k], kind="stable")
            order = order[order != b + k]
            r = np.flatnonzero(np.isin(order, nb)) + 1
            want = np.mean(np.arange(1, r.size + 1) / r)
            assert abs(ap[b + k].item() - want) <= 1e-14 * want


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_give_bitwise_the_single_process_result(tmp_path):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["OMP_NUM_THREADS"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), WORKER, "map", str(tmp_path)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600, cwd=ROOT)
    assert proc.returncode == 0, proc.stderr.decode(errors="replace")[-3000:]
    got = torch.load(os.path.join(str(tmp_path), "map_w2.pt"))
    assert got["world"] == 2
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gpu_map_worker as w
    S = w.SHAPE
    ids, dists = w.map_triples(S["graph"])
    N = int(ids.max()) + 1
    m = w.map_model(S["manifold"], S["metric"], S["dims"], N, S["seed"], DEV)
    value, ap = m.mean_average_precision((ids.to(DEV), dists.to(DEV)), dtype=torch.float32, return_rows=True)
    assert torch.equal(got["ap"], ap.cpu())
    assert got["map"] == value


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_runner_idiom_on_a_device_matrix_equals_the_host_answer(dtype):
    ids, dists = triples_of("grid3d-125")
    N = int(ids.max()) + 1
    m = make_model("bounded", "riem", 3, data.trained_like_table(N, 3, model="bounded", seed=9))
    metric = MeanAveragePrecisionMetric(TensorDataset(ids.to(DEV), dists.to(DEV)))
    dm = m.distance_matrix().to(dtype)
    on_device = metric.calculate_metric(dm)
    on_host = MeanAveragePrecisionMetric(TensorDataset(ids, dists)).calculate_metric(dm.cpu())
    assert abs(on_device - on_host) <= 1e-14 * abs(on_host)
    assert_ap_equal(metric.average_precisions(dm), metric.average_precisions(dm.cpu()))
