#!/usr/bin/env python3
"""Timing of the graph distance census and the ball sampling (csrc/graph_census.hip through sympa_amd.graph.GraphDistances) on the
GPU box, on product-cartesian-45500 (N = 45 500, 65 row blocks of 128 MiB) and margulis-71 (N = 5 041, one block), in one process.

Every pass recomputes the hop rows block by block, so the rows pass alone is the floor of all of them:

  rows      (a) every row block once, nothing done with it;
  kernel    (b) GraphDistances.census(), ball_sizes(r) and one sample_ball_pairs(r, 1 048 576) with the sizes given;
  torch     (c) the same three reductions over the same row blocks written with torch ops, the formulations (b) replaces: a
            count_triplets-style mask with a bincount / a row sum, and for the selection a cumsum over the block's mask with a
            searchsorted of the requested positions.

r is the radius of the fraction 0.01 of the pairs.  The results of (b) and (c) are compared for equality before anything is timed.
Times are host clocks around work that ends in a device synchronise, warm, median of 5, the two forms alternating.  Recorded
numbers only: nothing here is a threshold.

    python tools/graph_census_time.py [--out profiles/graph_census_time.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRAPHS = ("product-cartesian-45500", "margulis-71")
FRACTION = 0.01
PAIRS = 1 << 20


def torch_census(gd):
    import torch
    N = gd.num_nodes
    bins = torch.zeros(N, dtype=torch.int64, device=gd.device)
    col = torch.arange(N, device=gd.device)
    for b, rows in gd.blocks():
        i = torch.arange(b, b + rows.shape[0], device=gd.device)
        bins += torch.bincount(rows[(rows > 0) & (col[None, :] > i[:, None])].to(torch.int64), minlength=N)
    return bins.cpu()


def torch_ball_sizes(gd, radius):
    import torch
    N = gd.num_nodes
    upper = torch.empty(N, dtype=torch.int64, device=gd.device)
    col = torch.arange(N, device=gd.device)
    for b, rows in gd.blocks():
        i = torch.arange(b, b + rows.shape[0], device=gd.device)
        upper[b:b + rows.shape[0]] = ((rows > 0) & (rows <= radius) & (col[None, :] > i[:, None])).sum(1)
    return upper


def torch_sample(gd, radius, batch, upper, batch_id=0, seed=42):
    """GraphDistances.sample_ball_pairs with the selection of a block written as cumsum + searchsorted."""
    import numpy as np
    import torch
    from sympa_amd import data
    N, dev = gd.num_nodes, gd.device
    prefix = torch.cumsum(upper, 0)
    size = int(prefix[-1])
    cnt = np.uint64(batch_id) * np.uint64(batch) + np.arange(batch, dtype=np.uint64)
    k = torch.from_numpy((data.keyed_u64(seed, 12, cnt) % np.uint64(size)).astype(np.int64)).to(dev)
    row = torch.searchsorted(prefix, k, right=True)
    rank = k - (prefix[row] - upper[row])
    ids = torch.empty(batch, 2, dtype=torch.int64, device=dev)
    dist = torch.empty(batch, dtype=torch.float64, device=dev)
    buf = gd._block_buffer()
    R = buf.shape[0]
    order = torch.argsort(row, stable=True)
    row_s, rank_s = row[order], rank[order]
    needed, counts = torch.unique_consecutive(row_s // R, return_counts=True)
    col = torch.arange(N, device=dev)
    start = 0
    for blk, end in zip(needed.tolist(), torch.cumsum(counts, 0).tolist()):
        b = blk * R
        rows = gd.rows(b, min(R, N - b), out=buf)
        i = torch.arange(b, b + rows.shape[0], device=dev)
        mask = (rows > 0) & (rows <= radius) & (col[None, :] > i[:, None])
        running = torch.cumsum(mask.flatten(), 0)                        # int64: ball columns up to and with each element
        before = prefix[row_s[start:end]] - upper[row_s[start:end]] - (prefix[b] - upper[b])
        at = torch.searchsorted(running, before + rank_s[start:end] + 1)
        ids[order[start:end], 1] = at % N
        dist[order[start:end]] = rows.flatten()[at].to(torch.float64)
        start = end
    ids[:, 0] = row
    return ids, dist


def median_ms(run, reps=5):
    import torch
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return round(times[len(times) // 2], 3), [round(t, 3) for t in times]


def measure(name, log):
    import torch
    from sympa_amd import data, ops
    from sympa_amd.graph import GraphDistances, graph_csr
    dev = torch.device("cuda:0")
    rowptr, cols, _ = graph_csr(data.named_graph(name))
    gd = GraphDistances(rowptr, cols, device=dev)
    N = gd.num_nodes

    def rows_pass():
        for _ in gd.blocks():
            pass

    # results first (this is the warm-up of every shape too)
    rows_pass()
    c = gd.census()
    radius, size = gd.radius_for_fraction(FRACTION, census=c)
    upper = gd.ball_sizes(radius)
    ids, dist = gd.sample_ball_pairs(radius, PAIRS, upper=upper)
    want = torch_census(gd)
    assert torch.equal(want[:c.diameter + 1], c.histogram) and int(want.sum()) == c.triplets, "census: kernel and torch differ"
    assert torch.equal(torch_ball_sizes(gd, radius), upper) and int(upper.sum()) == size, "ball sizes: kernel and torch differ"
    t_ids, t_dist = torch_sample(gd, radius, PAIRS, upper)
    assert torch.equal(t_ids, ids) and torch.equal(t_dist, dist), "ball draws: kernel and torch differ"
    assert ops.check_status(dev) == (0, 0)
    out = {"nodes": N, "block_rows": gd.block_rows, "blocks": -(-N // gd.block_rows), "triplets": c.triplets, "diameter": c.diameter,
           "fraction": FRACTION, "radius": radius, "ball_pairs": size, "sampled_pairs": PAIRS}
    log(f"{name}: {json.dumps(out)}")
    passes = {
        "rows": rows_pass,
        "kernel_census": gd.census, "torch_census": lambda: torch_census(gd),
        "kernel_ball_sizes": lambda: gd.ball_sizes(radius), "torch_ball_sizes": lambda: torch_ball_sizes(gd, radius),
        "kernel_sample": lambda: gd.sample_ball_pairs(radius, PAIRS, upper=upper),
        "torch_sample": lambda: torch_sample(gd, radius, PAIRS, upper),
    }
    # alternate the forms: one repetition of every pass per round
    times = {k: [] for k in passes}
    for _ in range(5):
        for k, run in passes.items():
            times[k].append(median_ms(run, reps=1)[0])
    ms = {}
    for k, v in times.items():
        ms[k] = {"median_ms": sorted(v)[len(v) // 2], "all_ms": v}
        log(f"{name}: {k} {ms[k]}")
    floor = ms["rows"]["median_ms"]
    out["passes"] = ms
    out["over_the_rows_pass_ms"] = {k: round(v["median_ms"] - floor, 3) for k, v in ms.items() if k != "rows"}
    out["kernel_no_slower_than_torch"] = {what: ms["kernel_" + what]["median_ms"] <= ms["torch_" + what]["median_ms"]
                                          for what in ("census", "ball_sizes", "sample")}
    gd.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_census_time.json"))
    ap.add_argument("--graphs", default=",".join(GRAPHS), help="comma-separated named graphs (default: both)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("graph_census_time.py measures on a GPU and found none")

    def log(line):
        print(line, flush=True)
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "host clock around a pass that ends in a device synchronise, warm, median of 5, forms alternating"}
    for name in args.graphs.split(","):
        result[name] = measure(name, log)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
