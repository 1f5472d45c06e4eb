#!/usr/bin/env python3
"""Timing of the device mean average precision (csrc/map_rank.hip, Model.mean_average_precision) on the GPU box.

  1. ranking kernel alone (ops.map_rows over one block of rows, fp32 keys): us per block and effective GB/s (bytes of the rows
     read once) against the 8 TB/s HBM peak, at N = 5 041 (margulis-71 neighbours) and N = 45 500 (a 182 x 250 grid);
     the default 128 MiB block and a 256 / 512 MiB one, each ranked right after the all-pairs kernel wrote it (warm: what
     Model.mean_average_precision does) and after a 1 GiB write elsewhere (cold: from HBM);
  2. end to end: Model.mean_average_precision wall time at the configs[1], [2], [3] shapes, and the same block loop with the
     distances only, whose ratio is the share of time spent on distances;
  3. A/B: the same ranking as a torch-only composition (stable torch.sort of each block + gathers + cumsum).

    python tools/map_time.py [--out profiles/map_time.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sympa_amd import data, ops  # noqa: E402
from sympa_amd.metrics import MeanAveragePrecisionMetric  # noqa: E402
from sympa_amd.model import Model  # noqa: E402

DEV = torch.device("cuda:0")
CONFIGS = {   # BASELINE.json shapes: (model, metric, dims, nodes)
    "configs[1] tree-b3-h6 upper riem n4": ("upper", "riem", 4, 1093),
    "configs[2] margulis-71 bounded finf n4": ("bounded", "finf", 4, 5041),
    "configs[3] cartesian upper riem n8": ("upper", "riem", 8, 45500),
}


def model_of(model, metric, n, N):
    class A:
        pass
    A.manifold, A.metric, A.dims, A.num_points = model, metric, n, N
    A.scale_coef, A.scale_init, A.train_scale = 1.0, 1.0, False
    m = Model(A)
    with torch.no_grad():
        m.embeddings.embeds.data = data.trained_like_table(N, n, model=model, seed=42)
    return m.to(DEV)


def edges_of(N):
    """Neighbour triples: the graph's edges for the config graphs, a 2-D grid of width 250 for N = 45 500."""
    import networkx as nx
    if N == 1093:
        g = nx.convert_node_labels_to_integers(nx.balanced_tree(3, 6), ordering="sorted")
    elif N == 5041:
        g = nx.convert_node_labels_to_integers(nx.Graph(nx.margulis_gabber_galil_graph(71)), ordering="sorted")
    else:
        g = nx.grid_2d_graph(N // 250, 250)
        g = nx.convert_node_labels_to_integers(g, ordering="sorted")
    e = torch.tensor([(a, b) for a, b in g.edges() if a != b], dtype=torch.int64)
    return e.to(DEV), torch.ones(e.shape[0], device=DEV)


def events_ms(fn, reps=5, before=None):
    out = []
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2]


def torch_rank(rows, b, rowptr, cols, deg):
    """AP of a block by a stable torch.sort of the fp32 keys (self forced first) and gathers."""
    R, N = rows.shape
    keys = rows.float()
    ar = torch.arange(R, device=rows.device)
    keys[ar, b + ar] = -float("inf")
    order = torch.sort(keys, dim=1, stable=True).indices[:, 1:]
    nb = torch.zeros(R, N, dtype=torch.bool, device=rows.device)
    lo = rowptr[b:b + R]
    cnt = rowptr[b + 1:b + R + 1] - lo
    rid = torch.repeat_interleave(ar, cnt)
    nb[rid, cols[lo[0]:lo[0] + cnt.sum()].long()] = True
    nb[ar, b + ar] = False
    hit = nb.gather(1, order).double()
    t = torch.cumsum(hit, 1)
    pos = torch.arange(1, N, device=rows.device, dtype=torch.float64)
    return (hit * t / pos).sum(1) / deg[b:b + R]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_time.json"))
    ap.add_argument("--skip-e2e-cfg3", action="store_true")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "rank_kernel": [], "e2e": [], "torch_ab": []}
    flush = torch.empty(1 << 27, dtype=torch.float64, device=DEV)           # 1 GiB
    for N, n in ((5041, 4), (45500, 8)):
        m = model_of("upper", "riem", n, N)
        ids, d = edges_of(N)
        metric = MeanAveragePrecisionMetric((ids, d))
        nbrs = metric.csr(N, DEV)
        table = m.embeddings.embeds.detach()
        ws = torch.empty(ops._lib.load().sympa_all_pairs_workspace_bytes(N, n, 0) // 8, dtype=torch.float64, device=DEV)
        for mib in (128, 256, 512):
            R = min(N, (mib << 20) // (8 * N))
            buf = torch.empty(R, N, dtype=torch.float64, device=DEV)
            out = torch.empty(R, dtype=torch.float64, device=DEV)

            def produce():
                ops.all_pairs_dist(table, "upper", "riem", None, m.scale.detach(), 1.0, 0, R, out=buf, workspace=ws,
                                   flags=ops.FLAG_NO_SYMMETRY)

            def rank():
                ops.map_rows(buf, 0, nbrs, float32=True, out=out, max_degree=metric.max_degree)
            produce()
            rank()
            warm = events_ms(rank, before=produce)
            cold = events_ms(rank, before=lambda: flush.fill_(1.0))
            gb = R * N * 8 / 1e9
            row = {"N": N, "block_MiB": round(R * N * 8 / 2**20, 1), "rows": R, "warm_us": round(warm * 1e3, 1),
                   "cold_us": round(cold * 1e3, 1), "warm_GBps": round(gb / (warm * 1e-3), 1),
                   "cold_GBps": round(gb / (cold * 1e-3), 1), "warm_frac_of_8TBps": round(gb / (warm * 1e-3) / 8000, 3),
                   "cold_frac_of_8TBps": round(gb / (cold * 1e-3) / 8000, 3)}
            res["rank_kernel"].append(row)
            print("rank", row, flush=True)
            if mib == 128:
                deg = (nbrs[0][1:] - nbrs[0][:-1]).double()
                tt = events_ms(lambda: torch_rank(buf, 0, nbrs[0], nbrs[1], deg), reps=3)
                want = torch_rank(buf, 0, nbrs[0], nbrs[1], deg)
                rank()
                agree = float(((want - out).abs() / out.abs()).max())
                row = {"N": N, "rows": R, "torch_sort_us": round(tt * 1e3, 1), "kernel_us": round(warm * 1e3, 1),
                       "speedup": round(tt / warm, 1), "max_rel_diff": agree}
                res["torch_ab"].append(row)
                print("torch A/B", row, flush=True)
            del buf, out
            torch.cuda.empty_cache()
    for name, (model, metric_name, n, N) in CONFIGS.items():
        if args.skip_e2e_cfg3 and N == 45500:
            continue
        m = model_of(model, metric_name, n, N)
        ids, d = edges_of(N)
        metric = MeanAveragePrecisionMetric((ids, d))
        m.mean_average_precision(metric)                                 # warm-up (allocations, pack)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value = m.mean_average_precision(metric)
        wall = time.perf_counter() - t0
        # the distances alone, same blocks
        table = m.embeddings.embeds.detach()
        R = max(1, (128 << 20) // (8 * N))
        buf = torch.empty(min(R, N), N, dtype=torch.float64, device=DEV)
        need = ops._lib.load().sympa_all_pairs_workspace_bytes(N, n, ops.MODEL_IDS[model])
        ws = torch.empty(need // 8, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(0, N, R):
            r = min(R, N - b)
            ops.all_pairs_dist(table, model, metric_name, None, m.scale.detach(), 1.0, b, r, out=buf[:r], workspace=ws,
                               flags=ops.FLAG_NO_SYMMETRY)
        torch.cuda.synchronize()
        dist_s = time.perf_counter() - t0
        row = {"config": name, "N": N, "map": value, "wall_s": round(wall, 4), "distances_s": round(dist_s, 4),
               "distance_share": round(dist_s / wall, 3)}
        res["e2e"].append(row)
        print("e2e", row, flush=True)
        del buf, ws
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
