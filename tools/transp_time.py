#!/usr/bin/env python3
"""Device time of the parallel transport along geodesics (sympa_transp_exp / sympa_transp), same process, interleaved:

    python tools/transp_time.py [--rounds 40] [--limit 20] [--out profiles/transp_time.json]

Tables: those of tools/expmap_time.py -- bench.py's headline table (5 041 rows, n = 4) and 45 500 rows at n = 8
(data.trained_like_table), both models.  Rows per table, each a hipGraph of 8 launches replayed `rounds` times, the rows
alternating inside every round, device events around each replay (the median is the figure, the minimum is printed next to it):
  transp_exp          sympa_transp_exp(table, u, v) without out_y; u = logmap(table, table shuffled), v = fixed random symmetric rows
  transp_exp_point    the same with out_y: the point and the transported vector from one launch
  transp              sympa_transp(table, table shuffled, v)
  expmap_then_transp  sympa_expmap(table, u) followed by sympa_transp_exp(table, u, v) without out_y: what transp_exp_point replaces
Every launch and every replay runs under its own time limit (--limit seconds): the host polls the event behind it and, when the
limit passes, leaves the process at once with exit status 124 and starts nothing more on the device.
No ratio is promised; the numbers are recorded."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from sympa_amd import data, ops  # noqa: E402

LAUNCHES = 8
LIMIT = 20.0


def wait_for(event, what):
    t0 = time.monotonic()
    while not event.query():
        if time.monotonic() - t0 > LIMIT:
            print(f"{what}: not finished after {LIMIT:.0f} s; leaving, nothing more is started", flush=True)
            os._exit(124)
        time.sleep(2e-4)


def guarded(fn, what):
    fn()
    e = torch.cuda.Event()
    e.record()
    wait_for(e, what)


def graph_of(fn, what):
    for _ in range(3):
        guarded(fn, what)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(LAUNCHES):
            fn()
    guarded(g.replay, what + " (graph)")
    return g


def time_interleaved(graphs, rounds):
    out = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            wait_for(b, k)
            out[k].append(a.elapsed_time(b) * 1e3 / LAUNCHES)
    return {k: sorted(v) for k, v in out.items()}


def rows_for(model, n, nodes, dev, rounds):
    table = data.trained_like_table(nodes, n, model=model).to(dev).contiguous()
    other = table[torch.randperm(nodes, device=dev)].contiguous()
    logs = ops.logmap(table, other, model)
    gen = torch.Generator(device=dev).manual_seed(3)
    v = torch.randn(table.shape, dtype=torch.float64, device=dev, generator=gen)
    v = (v + v.transpose(-1, -2)).contiguous()

    def both():
        ops.expmap(table, logs, model)
        ops.transp_exp(table, logs, v, model)

    work = {"transp_exp": lambda: ops.transp_exp(table, logs, v, model),
            "transp_exp_point": lambda: ops.transp_exp(table, logs, v, model, return_point=True),
            "transp": lambda: ops.transp(table, other, v, model),
            "expmap_then_transp": both}
    tag = f"{model} n={n} rows={nodes}"
    t = time_interleaved({k: graph_of(f, f"{tag} {k}") for k, f in work.items()}, rounds)
    rec = {k: {"median_us": x[len(x) // 2], "min_us": x[0]} for k, x in t.items()}
    torch.cuda.synchronize()
    ops.check_status(dev)
    print(f"{tag}: " + ", ".join(f"{k} {rec[k]['median_us']:.1f} us (min {rec[k]['min_us']:.1f})" for k in work), flush=True)
    return rec


def main():
    global LIMIT
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--limit", type=float, default=LIMIT, help="seconds a single launch or replay may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    LIMIT = args.limit
    assert torch.cuda.is_available(), "transp_time.py measures device time: it needs the GPU"
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
