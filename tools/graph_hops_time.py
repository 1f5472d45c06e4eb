#!/usr/bin/env python3
"""Timing of the device graph hop distances (csrc/graph_bfs.hip, sympa_amd.graph.GraphDistances) on the GPU box.

  1. all rows of margulis-71 (N = 5 041) and of product-cartesian-45500 (N = 45 500) through the default 128 MiB row block:
     event-timed device time, median of 5, warm (one untimed pass first), and the effective written GB/s (4 N^2 bytes of rows
     written once) against the 8 TB/s HBM peak;
  2. the wall time of the scipy call inside data.graph_triplets (shortest_path over the same cleaned adjacency) for margulis-71
     on the same box, and the ratio;
  3. Model.evaluate_all_pairs wall time at configs[3] (upper, riem, n = 8, N = 45 500) on its own graph.

    python tools/graph_hops_time.py [--out profiles/graph_hops_time.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sympa_amd import data, ops  # noqa: E402
from sympa_amd.graph import GraphDistances, graph_csr  # noqa: E402
from sympa_amd.model import Model  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK_GBS = 8000.0


def all_rows_ms(gd, reps=5):
    def sweep():
        for _ in gd.blocks():
            pass
    sweep()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sweep()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times


def scipy_seconds(graph):
    """The shortest_path call of data.graph_triplets, on the adjacency it builds."""
    import networkx as nx
    from scipy.sparse.csgraph import shortest_path
    g = nx.convert_node_labels_to_integers(graph, ordering="sorted")
    adj = nx.to_scipy_sparse_array(nx.Graph(g), nodelist=range(g.number_of_nodes()), weight=None, format="csr")
    adj.setdiag(0)
    adj.eliminate_zeros()
    t0 = time.perf_counter()
    dist = shortest_path(adj, method="D", unweighted=True, directed=False)
    return time.perf_counter() - t0, int(dist[dist < float("inf")].max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_hops_time.json"))
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "hbm_peak_gbs": HBM_PEAK_GBS, "graphs": {}}
    for name in ("margulis-71", "product-cartesian-45500"):
        t0 = time.perf_counter()
        rowptr, cols, _ = graph_csr(data.named_graph(name))
        csr_s = time.perf_counter() - t0
        gd = GraphDistances(rowptr, cols, device=DEV)
        N = gd.num_nodes
        ms, all_ms = all_rows_ms(gd)
        ops.check_status(DEV)
        written = 4.0 * N * N
        gbs = written / (ms * 1e-3) / 1e9
        result["graphs"][name] = {
            "nodes": N, "csr_entries": int(cols.numel()), "graph_and_csr_build_s": round(csr_s, 3),
            "block_rows": gd.block_rows, "blocks": -(-N // gd.block_rows), "workspace_bytes": gd.workspace_bytes(),
            "all_rows_ms_median_of_5": round(ms, 3), "all_rows_ms": [round(t, 3) for t in all_ms],
            "written_bytes": int(written), "written_gbs": round(gbs, 1), "fraction_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
        print(f"{name}: N = {N}, {gd.block_rows} rows per block, all rows {ms:.3f} ms, {gbs:.1f} GB/s written "
              f"({100 * gbs / HBM_PEAK_GBS:.2f} % of {HBM_PEAK_GBS:.0f} GB/s)", flush=True)
        gd.release()
    secs, diameter = scipy_seconds(data.named_graph("margulis-71"))
    dev_ms = result["graphs"]["margulis-71"]["all_rows_ms_median_of_5"]
    result["scipy_margulis_71"] = {"shortest_path_wall_s": round(secs, 4), "diameter": diameter,
                                   "device_all_rows_ms": dev_ms, "scipy_over_device": round(secs * 1e3 / dev_ms, 1)}
    print(f"margulis-71: scipy shortest_path {secs:.3f} s, device rows {dev_ms:.3f} ms: {secs * 1e3 / dev_ms:.1f} x", flush=True)
    assert dev_ms < secs * 1e3, "the device rows of margulis-71 must take less time than the scipy call"

    # configs[3] scored on its own graph
    class A:
        manifold, metric, dims, num_points = "upper", "riem", 8, 45500
        scale_coef, scale_init, train_scale = 1.0, 1.0, False
    m = Model(A)
    with torch.no_grad():
        m.embeddings.embeds.data = data.trained_like_table(45500, 8, seed=42)
    m = m.to(DEV)
    rowptr, cols, _ = graph_csr(data.named_graph("product-cartesian-45500"))
    gd = GraphDistances(rowptr, cols, device=DEV)
    m.evaluate_all_pairs(gd)
    t0 = time.perf_counter()
    value = m.evaluate_all_pairs(gd)
    wall = time.perf_counter() - t0
    ops.check_status(DEV)
    result["evaluate_all_pairs_configs3"] = {"pairs": 45500 * 45499 // 2, "wall_s": round(wall, 3), "distortion": value}
    print(f"configs[3] evaluate_all_pairs: {wall:.3f} s over {45500 * 45499 // 2} pairs, distortion {value:.6f}", flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
