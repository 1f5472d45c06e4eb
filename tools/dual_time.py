#!/usr/bin/env python3
"""Device time of the compact dual model against the bounded model, same process, same device, same points, interleaved A/B:

    python tools/dual_time.py [--rounds 40] [--out profiles/dual_time.json]

Dual did not exist before its commit, so its yardstick is the bounded model: the two instruction streams differ in the sign of
the factor input and in the last step (n arctangents against n logarithms per pair).  Shapes: bench.py's configs, n = 4 at
65 536 pairs over 5 041 rows and n = 8 at 262 144 pairs over 45 500 rows (the bounded table of data.trained_like_table: its points
are points of both models).  Rows per shape, each a hipGraph of 8 launches replayed `rounds` times, the models alternating inside
every round, device events around each replay:
  forward        ops.model_forward (dense one-pair-per-lane kernel for both: the bounded packed table is not used)
  forward_vvd    sympa_siegel_dist_fwd on pre-gathered pairs with the vector-valued distance written
  train_step     ops.model_loss_backward (fused loss + backward, scatter; SYMPA_FLAG_GENERIC: the one-pair-per-lane kernel for
                 both models, the only family dual has) + ops.rsgd_step_
  runtime_n      n = 12, 65 536 pairs, SYMPA_FLAG_GENERIC: the runtime-n forward, whose model is a runtime argument (bounded
                 is timed on every build; run this tool on the parent build for its figure there)
Prints and writes median / min us per launch and the ratio dual / bounded.  A build without the dual model times bounded only."""
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
    """{name: sorted list of us per launch}, the graphs alternating inside every round."""
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


def rows_for(n, nodes, pairs, dev, rounds, models, generic_only=False):
    table = data.trained_like_table(nodes, n, model="bounded").to(dev).contiguous()
    trip = data.sample_pairs(nodes, pairs, 1).to(dev).contiguous()
    gd = torch.randint(1, 9, (pairs,), device=dev).to(torch.float64)
    z1, z2 = table[trip[:, 0]].contiguous(), table[trip[:, 1]].contiguous()
    work = {}
    for m in models:
        w = work[m] = {}
        if generic_only:
            w["runtime_n"] = lambda m=m: ops.siegel_dist_forward(z1, z2, m, "riem", flags=ops.FLAG_GENERIC)
            continue
        tab = table.clone()
        grad = torch.zeros_like(tab)
        loss = torch.zeros(1, dtype=torch.float64, device=dev)
        out = torch.empty(pairs, dtype=torch.float64, device=dev)
        w["forward"] = lambda m=m, out=out: ops.model_forward(table, trip, m, "riem", out=out)
        w["forward_vvd"] = lambda m=m: ops.siegel_dist_forward(z1, z2, m, "riem", return_vvd=True)

        def step(m=m, tab=tab, grad=grad, loss=loss):
            grad.zero_()
            ops.model_loss_backward(tab, trip, gd, grad, loss, m, "riem", loss_scale=1.0 / pairs, flags=ops.FLAG_GENERIC)
            ops.rsgd_step_(tab, grad, m, 1e-6)
        w["train_step"] = step
    res = {}
    for row in next(iter(work.values())):
        graphs = {m: graph_of(work[m][row]) for m in models}
        t = time_interleaved(graphs, rounds)
        rec = {m: {"median_us": t[m][len(t[m]) // 2], "min_us": t[m][0]} for m in models}
        if "dual" in rec:
            rec["ratio_dual_over_bounded"] = rec["dual"]["median_us"] / rec["bounded"]["median_us"]
        res[row] = rec
        print(f"n={n} pairs={pairs} {row}: " + ", ".join(
            f"{m} {rec[m]['median_us']:.1f} us (min {rec[m]['min_us']:.1f})" for m in models) +
            (f", dual / bounded {rec['ratio_dual_over_bounded']:.3f}" if "dual" in rec else ""), flush=True)
    torch.cuda.synchronize()
    ops.check_status(dev)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dual_time.py measures device time: it needs the GPU"
    dev = torch.device("cuda:0")
    models = ["bounded"] + (["dual"] if "dual" in ops.MODEL_IDS else [])
    res = {"device": torch.cuda.get_device_name(0), "launches_per_replay": LAUNCHES, "rounds": args.rounds, "models": models,
           "n4_65536": rows_for(4, 5041, 65536, dev, args.rounds, models),
           "n8_262144": rows_for(8, 45500, 262144, dev, args.rounds, models),
           "n12_65536": rows_for(12, 5041, 65536, dev, max(args.rounds // 4, 5), models, generic_only=True)}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
