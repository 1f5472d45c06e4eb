#!/usr/bin/env python3
"""Time a training-shaped step of the spd model through the vector-valued distance against the built-in distance routes
 -> profiles/spd_vvd_time.json.

    python tools/spd_vvd_time.py [--out profiles/spd_vvd_time.json] [--quick]

Three routes, each forward + AverageDistortionLoss + backward() into the table gradient, on the same table and triplets:
  vvd        Model.forward_vvd + spd_metric(v, "riem") + loss + backward()    (sympa_spd_model_vvd_forward / _backward)
  coop       Model.forward + loss + backward(), the backward forced to SYMPA_FLAG_COOP: the one-kernel sixteen-lanes form the vvd
             backward is built from (ops.spd_backward_rows is wrapped for the duration of this route only)
  default    Model.forward + loss + backward() as it dispatches by itself (the three-kernel form with a workspace at n >= 9, the
             two-rounds form at n = 8)
Shapes: n = 8 and n = 16 with 65 536 pairs, n = 16 with 1 048 576 pairs over 100 000 rows (BASELINE configs[4]).
Device time between events, after a warm-up of every route; the routes alternate inside one process and each figure is the median of
5 rounds.  Before any timing the table gradients of the three routes are compared (largest difference relative to the largest
gradient entry).  No ratio is a pass criterion; needs a GPU (no fallback)."""
import argparse
import functools
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from sympa_amd import data, ops  # noqa: E402
from sympa_amd.losses import AverageDistortionLoss  # noqa: E402
from sympa_amd.manifolds.spd import spd_metric  # noqa: E402
from sympa_amd.model import Model  # noqa: E402

SHAPES = ((8, 4096, 65536), (16, 4096, 65536), (16, 100000, 1048576))      # (n, table rows, pairs)
ROUTES = ("vvd", "coop", "default")
ROUNDS, REPEAT = 5, 4


def make(n, rows, pairs, dev, seed=1):
    class A:
        manifold, metric, dims, num_points = "spd", "riem", n, rows
        scale_coef, scale_init, train_scale = 1.0, 1.0, False
    m = Model(A)
    with torch.no_grad():
        m.embeddings.embeds.data = data.spd_table(rows, n, seed=seed)
    m = m.to(dev)
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, rows, (pairs,), generator=g)
    dst = (src + torch.randint(1, rows, (pairs,), generator=g)) % rows           # src != dst
    trip = torch.stack((src, dst), 1).to(dev)
    gd = torch.randint(1, 9, (pairs,), generator=g).to(torch.float64).to(dev)
    return m, trip, gd


def step(m, trip, gd, route):
    m.embeddings.embeds.grad = None
    if route == "vvd":
        d = spd_metric(m.forward_vvd(trip), "riem")
    else:
        d = m(trip)
    AverageDistortionLoss().calculate_loss(gd, d).backward()
    return m.embeddings.embeds.grad


def run_route(m, trip, gd, route):
    if route != "coop":
        return step(m, trip, gd, route)
    plain = ops.spd_backward_rows
    ops.spd_backward_rows = functools.partial(plain, flags=ops.FLAG_COOP)
    try:
        return step(m, trip, gd, route)
    finally:
        ops.spd_backward_rows = plain


def timed(m, trip, gd, route):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPEAT):
        run_route(m, trip, gd, route)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / REPEAT          # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "spd_vvd_time.json"))
    ap.add_argument("--quick", action="store_true", help="the two 65 536-pair shapes only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spd_vvd_time.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "unit": "us per step (forward + loss + backward), device time between events",
           "rounds": ROUNDS, "steps_per_round": REPEAT, "shapes": []}
    for n, rows, pairs in (SHAPES[:2] if args.quick else SHAPES):
        m, trip, gd = make(n, rows, pairs, dev)
        grads = {r: run_route(m, trip, gd, r).clone() for r in ROUTES}           # (also the warm-up of every route)
        ops.check_status(dev)
        top = float(grads["default"].abs().max())
        diff = {r: float((grads[r] - grads["default"]).abs().max()) / top for r in ("vvd", "coop")}
        for r in ROUTES:
            run_route(m, trip, gd, r)
        torch.cuda.synchronize(dev)
        times = {r: [] for r in ROUTES}
        for _ in range(ROUNDS):
            for r in ROUTES:                                                     # the routes alternate
                times[r].append(timed(m, trip, gd, r))
        ops.check_status(dev)
        med = {r: statistics.median(times[r]) for r in ROUTES}
        row = {"n": n, "rows": rows, "pairs": pairs, "median_us": med, "all_us": times,
               "vvd_over_coop": med["vvd"] / med["coop"], "vvd_over_default": med["vvd"] / med["default"],
               "table_gradient_max_difference_relative_to_the_largest_entry": diff}
        out["shapes"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "all_us"}), flush=True)
        del m, trip, gd, grads
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
