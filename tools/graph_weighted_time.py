#!/usr/bin/env python3
"""Timing of the device weighted graph distances (csrc/graph_sssp.hip, sympa_amd.graph.WeightedGraphDistances) on the GPU box, on
product-cartesian-45500 (N = 45 500) with seeded weights U(0.5, 1.5) and again with every weight 1.0.

  rows-uniform / rows-unit   one default 128 MiB row block (event-timed device time, median of 5, warm) and all rows once, with
                             the sweeps the workgroups ran (min, median, max over the sources' groups);
  hops                       the hop kernel (csrc/graph_bfs.hip) over all rows of the same graph on the same box, for the ratio;
  scipy                      scipy's Dijkstra over 64 sampled sources of the uniform-weight graph on the box's CPU.

Every step runs in a child process of its own under its own time limit; the first step that fails ends the run.  Recorded
numbers only: nothing here is a threshold.

    python tools/graph_weighted_time.py [--out profiles/graph_weighted_time.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRAPH = "product-cartesian-45500"
# step -> time limit in seconds
STEPS = {"rows-uniform": 360, "rows-unit": 360, "hops": 180, "scipy": 300}


def weighted_csr(kind):
    import networkx as nx
    import numpy as np
    from sympa_amd import data
    from sympa_amd.graph import weighted_graph_csr
    g = data.named_graph(GRAPH)
    edges = list(g.edges())
    w = np.random.default_rng(0).uniform(0.5, 1.5, len(edges)) if kind == "uniform" else np.ones(len(edges))
    nx.set_edge_attributes(g, {e: float(x) for e, x in zip(edges, w)}, "weight")
    return weighted_graph_csr(g)[:3]


def median_ms(run, reps=5):
    import torch
    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return round(times[len(times) // 2], 3), [round(t, 3) for t in times]


def sweep_stats(sweeps):
    s = sorted(int(x) for x in sweeps)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1]}


def step_rows(kind):
    import torch
    from sympa_amd import ops
    from sympa_amd.graph import WeightedGraphDistances
    dev = torch.device("cuda:0")
    gd = WeightedGraphDistances(*weighted_csr(kind), device=dev)
    N, R = gd.num_nodes, min(gd.block_rows, gd.num_nodes)
    buf = gd._block_buffer()
    ms, all_ms = median_ms(lambda: gd.rows(0, R, out=buf))
    out = {"device": torch.cuda.get_device_name(0), "nodes": N, "csr_entries": int(gd.cols.numel()), "block_rows": R, "blocks": -(-N // R),
           "workgroups_per_block": -(-R // 8), "workspace_bytes": gd.workspace_bytes(), "first_block_ms_median_of_5": ms, "first_block_ms": all_ms}
    sweeps, per_block = [], []
    top = torch.zeros((), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(0, N, R):
        r = min(R, N - b)
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rows = gd.rows(b, r, out=buf)
        e.record()
        per_block.append((a, e))
        top = torch.maximum(top, rows.max())
        sweeps.append(ops.graph_weighted_sweeps(gd._ws, N, r).clone())
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ops.check_status(dev)
    block_ms = sorted(a.elapsed_time(e) for a, e in per_block[:-1] or per_block)          # the ragged last block aside
    out.update({"all_rows_ms_sum_of_blocks": round(sum(a.elapsed_time(e) for a, e in per_block), 3),
                "all_rows_wall_s_with_max_and_sweep_reads": round(wall, 3),
                "full_block_ms": {"min": round(block_ms[0], 3), "median": round(block_ms[len(block_ms) // 2], 3),
                                  "max": round(block_ms[-1], 3)},
                "sweeps_per_group": sweep_stats(torch.cat(sweeps)[::8].tolist()), "largest_distance": float(top)})
    return out


def step_hops():
    import torch
    from sympa_amd import data, ops
    from sympa_amd.graph import GraphDistances, graph_csr
    dev = torch.device("cuda:0")
    rowptr, cols, _ = graph_csr(data.named_graph(GRAPH))
    gd = GraphDistances(rowptr, cols, device=dev)

    def sweep():
        for _ in gd.blocks():
            pass
    ms, all_ms = median_ms(sweep, reps=3)
    ops.check_status(dev)
    return {"block_rows": gd.block_rows, "blocks": -(-gd.num_nodes // gd.block_rows), "all_rows_ms_median_of_3": ms,
            "all_rows_ms": all_ms}


def step_scipy():
    import numpy as np
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    rowptr, cols, weights = weighted_csr("uniform")
    N = rowptr.numel() - 1
    adj = csr_matrix((weights.numpy(), cols.numpy(), rowptr.numpy()), shape=(N, N))
    sources = np.sort(np.random.default_rng(1).choice(N, 64, replace=False))
    t0 = time.perf_counter()
    d = dijkstra(adj, directed=False, indices=sources)
    secs = time.perf_counter() - t0
    return {"sources": 64, "dijkstra_wall_s": round(secs, 4), "ms_per_source": round(secs * 1e3 / 64, 3),
            "all_rows_at_this_rate_s": round(secs / 64 * N, 1), "largest_distance": float(d.max())}


def run_step(name):
    if name.startswith("rows-"):
        return step_rows(name[5:])
    return {"hops": step_hops, "scipy": step_scipy}[name]()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_weighted_time.json"))
    ap.add_argument("--step", choices=list(STEPS), help="run one step in this process and print its JSON (what the driver starts)")
    ap.add_argument("--part", help="with --step: the file the step's JSON goes to")
    ap.add_argument("--only", help="comma-separated steps to run instead of all of them (the json then holds those alone)")
    args = ap.parse_args()
    if args.step:
        part = run_step(args.step)
        with open(args.part, "w") as f:
            json.dump(part, f)
        return
    result = {"graph": GRAPH, "weights": {"uniform": "numpy default_rng(0).uniform(0.5, 1.5) per edge", "unit": "1.0"}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS.items():
            if args.only and name not in args.only.split(","):
                continue
            part = os.path.join(tmp, name + ".json")
            t0 = time.perf_counter()
            # a fresh child per step, under its own time limit; a step that fails or hangs ends the run: nothing more is started
            proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--part", part], timeout=limit, cwd=ROOT)
            if proc.returncode != 0:
                raise SystemExit(f"step {name} ended with status {proc.returncode}: stopping")
            result[name] = json.load(open(part))
            print(f"{name}: {time.perf_counter() - t0:.1f} s  {json.dumps(result[name])}", flush=True)
    for kind in ("uniform", "unit"):
        if "rows-" + kind in result:
            result["device"] = result["rows-" + kind].pop("device")
            if "hops" in result:
                result.setdefault("weighted_over_hops_all_rows", {})[kind] = round(
                    result["rows-" + kind]["all_rows_ms_sum_of_blocks"] / result["hops"]["all_rows_ms_median_of_3"], 2)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
