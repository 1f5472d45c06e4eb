#!/usr/bin/env python3
"""Time a row block of the spd all-pairs distance matrix through the new entry against the routes it replaces
 -> profiles/spd_all_pairs_time.json.

    python tools/spd_all_pairs_time.py [--out profiles/spd_all_pairs_time.json] [--quick] [--dims 9,10,11,14,15]

Routes, all over the same block of R rows of the same table:
  new_riem      ops.spd_all_pairs_dist(table, "riem", row_begin, R)             (sympa_spd_all_pairs_dist, no pair list)
  pairs_dense   ops.spd_model_forward(table, pairs) over the block's [R N, 2] pair list: the route Model.distance_matrix took
  pairs_packed  ops.spd_model_forward_packed over the same list, where ops.SPD_PACKED_DIMS has the n (the pack itself is made
                before the timing and is not counted: it is shared with forward())
  pair_list     building that pair list (arange, repeat_interleave, repeat, stack): what every block paid on top
  new_fone      ops.spd_all_pairs_dist(table, "fone", row_begin, R)
  vvd_fone      spd_metric(ops.spd_model_vvd_forward(table, pairs), "fone"): the only way to a Finsler block before
Shapes: R = 256 rows of N = 4 096 at n = 8, 12, 13, 16; R = 64 rows of N = 100 000 at n = 16.
Device time between events around the replay of a captured graph of REPEAT launches of one route, after a warm-up of every route;
the routes alternate inside one process and each figure is the median of ROUNDS rounds.  Before any timing the routes' values are
compared.  No ratio is a pass criterion; needs a GPU (no fallback)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sympa_amd import data, ops  # noqa: E402
from sympa_amd.manifolds.spd import spd_metric  # noqa: E402

SHAPES = ((8, 4096, 256), (12, 4096, 256), (13, 4096, 256), (16, 4096, 256), (16, 100000, 64))      # (n, table rows, block rows)
ROUNDS, REPEAT = 7, 4


def pair_list(begin, count, N, dev):
    rows = torch.arange(begin, begin + count, device=dev)
    cols = torch.arange(N, device=dev)
    return torch.stack((rows.repeat_interleave(N), cols.repeat(count)), 1)


def graph_of(fn):
    """fn REPEAT times as one captured graph (fn's tensors live in the graph's pool)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPEAT):
            fn()
    return g


def timed(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / REPEAT          # us per block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "spd_all_pairs_time.json"))
    ap.add_argument("--quick", action="store_true", help="the N = 4 096 shapes only")
    ap.add_argument("--dims", default=None, help="comma-separated n: R = 256 rows of N = 4 096 at these n instead of SHAPES")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spd_all_pairs_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "unit": "us per row block, device time between events around a graph replay",
           "rounds": ROUNDS, "launches_per_graph": REPEAT, "shapes": []}
    shapes = SHAPES[:4] if args.quick else SHAPES
    if args.dims:
        shapes = tuple((int(n), 4096, 256) for n in args.dims.split(","))
    for n, N, R in shapes:
        table = data.spd_table(N, n, seed=1).to(dev)
        begin = (N // 2) // 64 * 64 + 7                                          # an interior block that starts inside a tile
        pairs = pair_list(begin, R, N, dev)
        buf = torch.empty(R, N, dtype=torch.float64, device=dev)
        flat = torch.empty(R * N, dtype=torch.float64, device=dev)
        routes = {
            "new_riem": lambda: ops.spd_all_pairs_dist(table, "riem", row_begin=begin, row_count=R, out=buf),
            "pairs_dense": lambda: ops.spd_model_forward(table, pairs, out=flat),
            "pair_list": lambda: pair_list(begin, R, N, dev),
            "new_fone": lambda: ops.spd_all_pairs_dist(table, "fone", row_begin=begin, row_count=R, out=buf),
            "vvd_fone": lambda: spd_metric(ops.spd_model_vvd_forward(table, pairs), "fone"),
        }
        if n in ops.SPD_PACKED_DIMS:
            pk = ops.SpdPackedTable()
            pk.ensure(table)
            routes["pairs_packed"] = lambda: ops.spd_model_forward_packed(pk, pairs, out=flat)
        # values first (also the warm-up of every route)
        new_r = routes["new_riem"]().clone()
        old_r = routes["pairs_dense"]().reshape(R, N).clone()
        new_f = routes["new_fone"]().clone()
        old_f = routes["vvd_fone"]().reshape(R, N).clone()
        ops.check_status(dev)
        off = torch.ones(R, N, dtype=torch.bool, device=dev)
        off[torch.arange(R, device=dev), torch.arange(begin, begin + R, device=dev)] = False
        diff = {"riem_vs_pair_list_route_max_relative": float(((new_r - old_r).abs()[off] / old_r[off]).max()),
                "fone_vs_vvd_route_max_relative": float(((new_f - old_f).abs()[off] / old_f[off]).max())}
        del new_r, old_r, new_f, old_f, off
        graphs = {r: graph_of(fn) for r, fn in routes.items()}
        for g in graphs.values():
            g.replay()
        torch.cuda.synchronize(dev)
        times = {r: [] for r in graphs}
        for _ in range(ROUNDS):
            for r, g in graphs.items():                                          # the routes alternate
                times[r].append(timed(g))
        ops.check_status(dev)
        med = {r: statistics.median(times[r]) for r in graphs}
        parent = min(med["pairs_dense"], med.get("pairs_packed", float("inf")))
        row = {"n": n, "rows": N, "block_rows": R, "pairs": R * N, "median_us": med, "all_us": times,
               "new_riem_over_parent_kernel": med["new_riem"] / parent,
               "new_riem_over_parent_with_pair_list": med["new_riem"] / (parent + med["pair_list"]),
               "new_fone_over_vvd_fone": med["new_fone"] / med["vvd_fone"], "values": diff}
        out["shapes"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "all_us"}), flush=True)
        del graphs, routes, table, pairs, buf, flat
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
