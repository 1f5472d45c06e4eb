#!/usr/bin/env python3
"""Device time of the exponential / logarithm maps and of the RiemannianSGD step along the geodesic, next to the linear step
(sympa_rsgd_step, unchanged by the commit that added the maps) on the same tables, same process, interleaved:

    python tools/expmap_time.py [--rounds 40] [--out profiles/expmap_time.json]

Tables: bench.py's headline table (5 041 rows, n = 4) and 45 500 rows at n = 8 (data.trained_like_table), both models.  Rows per
table, each a hipGraph of 8 launches replayed `rounds` times, the rows alternating inside every round, device events around each
replay (the median is the figure, the minimum is printed next to it):
  logmap         sympa_logmap(table, table shuffled)
  expmap         sympa_expmap(table, those logarithms)
  rsgd_exp       sympa_rsgd_step_exp, lr = 1e-6 (the table barely moves over the replays), gradient = the fixed random symmetric rows
  rsgd_linear    sympa_rsgd_step on a copy, same gradient, same lr
Prints and writes median / min us per launch and the ratio rsgd_exp / rsgd_linear."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from sympa_amd import data, ops  # noqa: E402

LAUNCHES = 8


def graph_of(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(LAUNCHES):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def time_interleaved(graphs, rounds):
    out = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / LAUNCHES)
    return {k: sorted(v) for k, v in out.items()}


def rows_for(model, n, nodes, dev, rounds):
    table = data.trained_like_table(nodes, n, model=model).to(dev).contiguous()
    other = table[torch.randperm(nodes, device=dev)].contiguous()
    logs = ops.logmap(table, other, model)
    gen = torch.Generator(device=dev).manual_seed(3)
    grad = torch.randn(table.shape, dtype=torch.float64, device=dev, generator=gen)
    grad = (grad + grad.transpose(-1, -2)).contiguous()
    t_exp, t_lin = table.clone(), table.clone()
    work = {"logmap": lambda: ops.logmap(table, other, model),
            "expmap": lambda: ops.expmap(table, logs, model),
            "rsgd_exp": lambda: ops.rsgd_step_exp_(t_exp, grad, model, 1e-6),
            "rsgd_linear": lambda: ops.rsgd_step_(t_lin, grad, model, 1e-6)}
    t = time_interleaved({k: graph_of(f) for k, f in work.items()}, rounds)
    rec = {k: {"median_us": v[len(v) // 2], "min_us": v[0]} for k, v in t.items()}
    rec["ratio_rsgd_exp_over_linear"] = rec["rsgd_exp"]["median_us"] / rec["rsgd_linear"]["median_us"]
    torch.cuda.synchronize()
    ops.check_status(dev)
    print(f"{model} n={n} rows={nodes}: " + ", ".join(f"{k} {rec[k]['median_us']:.1f} us (min {rec[k]['min_us']:.1f})" for k in work) +
          f", rsgd_exp / rsgd_linear {rec['ratio_rsgd_exp_over_linear']:.2f}", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "expmap_time.py measures device time: it needs the GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "launches_per_replay": LAUNCHES, "rounds": args.rounds}
    for model in ops.EXPMAP_MODELS:
        res[f"{model}_n4_5041"] = rows_for(model, 4, 5041, dev, args.rounds)
        res[f"{model}_n8_45500"] = rows_for(model, 8, 45500, dev, args.rounds)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
