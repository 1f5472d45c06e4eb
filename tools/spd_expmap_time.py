"""Timing record of the spd exponential map, logarithm, geodesic and geodesic RSGD step: n in {4, 8, 16} at the
100 000-row table of configs[4] and at one small table (4 096 rows).  Per shape, in one run: sympa_spd_expmap, sympa_spd_logmap,
sympa_spd_geodesic, sympa_spd_rsgd_step_exp and, for comparison, the linear sympa_spd_rsgd_step of the same build on the same table
and gradient.  Every pass is a captured graph of LAUNCHES kernel launches timed with device events around its replay; the passes
alternate over ROUNDS rounds; median and minimum per launch are recorded.  No ratio is promised: the cost of the geodesic step over
the linear one is reported as found.  Bytes roof: 3 n^2 doubles per row (two read, one written) at 6.29 TB/s.

    python tools/spd_expmap_time.py [--out profiles/spd_expmap_time.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(n, rows) for n in (4, 8, 16) for rows in (100_000, 4_096)]
HBM_BYTES_PER_S = 6.29e12
LAUNCHES = 10
ROUNDS = 7


def measure(n, rows, log):
    import torch
    from sympa_amd import data, ops
    dev = torch.device("cuda:0")
    x = data.spd_table(rows, n, scale=0.3, seed=7).to(dev)
    y = data.spd_table(rows, n, scale=0.3, seed=8).to(dev)
    gen = torch.Generator().manual_seed(2)
    grad = torch.randn(rows, n, n, generator=gen, dtype=torch.float64)
    grad = (0.5 * (grad + grad.transpose(1, 2)) / n).to(dev)
    u = ops.spd_logmap(x, y)
    # results first: the maps invert each other and the two steps agree to second order in lr
    back = ops.spd_expmap(x, u)
    mid = ops.spd_geodesic(x, y, 0.5)
    errs = {"exp_of_log": float((back - y).abs().max() / y.abs().max()),
            "geodesic_half": float((mid - ops.spd_expmap(x, 0.5 * u)).abs().max() / mid.abs().max())}
    lr = 1e-3
    a, b = ops.spd_rsgd_step_exp_(x.clone(), grad, lr), ops.spd_rsgd_step_(x.clone(), grad, lr)
    errs["exp_step_against_linear_step"] = float((a - b).abs().max() / b.abs().max())
    assert ops.check_status(dev) == (0, 0)
    assert errs["exp_of_log"] < 1e-9 and errs["geodesic_half"] < 1e-9 and errs["exp_step_against_linear_step"] < 1e-3, errs
    t_exp, t_lin = x.clone(), x.clone()
    passes = {"expmap": lambda: ops.spd_expmap(x, u), "logmap": lambda: ops.spd_logmap(x, y),
              "geodesic": lambda: ops.spd_geodesic(x, y, 0.3),
              "rsgd_step_exp": lambda: ops.spd_rsgd_step_exp_(t_exp, grad, lr),        # (the table drifts by lr = 1e-3 steps: harmless)
              "rsgd_step_linear": lambda: ops.spd_rsgd_step_(t_lin, grad, lr)}
    graphs = {}
    side = torch.cuda.Stream(dev)
    for name, run in passes.items():
        run()                                          # warm: code objects, the self-check gate, the allocator
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(LAUNCHES):
                run()
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            g.replay()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / LAUNCHES)
    ms = {k: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "all_ms": [round(t, 5) for t in v]} for k, v in times.items()}
    roof_ms = rows * 3 * n * n * 8 / HBM_BYTES_PER_S * 1e3
    out = {"rows": rows, "n": n, "kernel": "sixteen lanes per row" if n >= 3 else "one row per lane", "checks": errs, "passes": ms,
           "exp_step_over_linear_step": round(ms["rsgd_step_exp"]["median_ms"] / ms["rsgd_step_linear"]["median_ms"], 2),
           "rows_per_second_exp_step": round(rows / ms["rsgd_step_exp"]["median_ms"] * 1e3),
           "bytes_roof_ms": round(roof_ms, 5), "exp_step_over_bytes_roof": round(ms["rsgd_step_exp"]["median_ms"] / roof_ms, 1)}
    log(f"spd n = {n} rows = {rows}: {json.dumps(out)}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spd_expmap_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spd_expmap_time.py measures on a GPU and found none")
    result = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S,
              "timing": f"device events around the replay of a captured graph of {LAUNCHES} launches, warm, {ROUNDS} rounds with the "
                        "passes alternating, median and minimum per launch"}
    for n, rows in SHAPES:
        result[f"spd-{n}-rows{rows}"] = measure(n, rows, lambda line: print(line, flush=True))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
