#!/usr/bin/env python3
"""Timing of the differentiable vector-valued distance on one MI355X, against the built-in metric route of the same shapes in the
same process:

  vvd      v = Model.forward_vvd(triplets) (sympa_model_vvd_forward), riem written in torch on v (torch.norm), the
           AverageDistortionLoss in torch, loss.backward() (torch's backward of the norm, then sympa_model_vvd_backward: one pair
           per lane, fp64 atomics into the dense table gradient);
  builtin  d = Model.forward(triplets) with metric riem (sympa_model_forward), the same loss in torch, loss.backward()
           (sympa_model_backward: the scalar adjoint; at n = 8 the split two-kernel form).

Shapes: upper n = 4 with 65 536 pairs of 5 041 rows, upper n = 8 with 262 144 pairs of 45 500 rows.  The two table gradients are
compared before anything is timed.  Times are device times between two events around a whole pass (forward + loss + backward),
warm, median of 5, the forms alternating.  Recorded numbers only: nothing here is a threshold.

    python tools/vvd_time.py [--out profiles/vvd_time.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((4, 5041, 65536), (8, 45500, 262144))        # (n, table rows, pairs)


def device_ms(run):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    run()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b), 4)


def spread_table(n, rows, dev):
    """A table as training leaves it: distances O(1) (the initial table has every point within 1e-3 of the base point)."""
    import torch
    g = torch.Generator().manual_seed(n)
    x = 0.3 * torch.randn(rows, n, n, generator=g, dtype=torch.float64)
    a = 0.3 * torch.randn(rows, n, n, generator=g, dtype=torch.float64)
    x, a = x.to(dev), a.to(dev)
    y = torch.matrix_exp(0.5 * (a + a.transpose(-1, -2)))
    return torch.stack((0.5 * (x + x.transpose(-1, -2)), 0.5 * (y + y.transpose(-1, -2))), 1).contiguous()


def measure(n, rows, pairs, log):
    import torch
    from sympa_amd import ops
    from sympa_amd.losses import AverageDistortionLoss
    from sympa_amd.model import Model
    dev = torch.device("cuda:0")

    class A:
        manifold, metric, num_points = "upper", "riem", rows
        scale_coef, scale_init, train_scale = 1.0, 1.0, False
    A.dims = n
    m = Model(A).to(dev)
    with torch.no_grad():
        m.embeddings.embeds.data = spread_table(n, rows, dev)
    emb = m.embeddings.embeds
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, rows, (pairs,), generator=g)
    dst = (src + 1 + torch.randint(0, rows - 1, (pairs,), generator=g)) % rows      # never src: torch's norm has no gradient at v = 0
    ids = torch.stack((src, dst), 1).to(dev)
    gd = torch.randint(1, 9, (pairs,), generator=g).to(torch.float64).to(dev)
    loss_fn = AverageDistortionLoss()

    def vvd():
        emb.grad = None
        d = torch.norm(m.forward_vvd(ids), dim=-1)
        loss_fn.calculate_loss(gd, d).backward()

    def builtin():
        emb.grad = None
        loss_fn.calculate_loss(gd, m(ids)).backward()

    # results first (the warm-up of both forms too)
    vvd()
    ga = emb.grad.clone()
    builtin()
    gb = emb.grad.clone()
    assert ops.check_status(dev) == (0, 0)
    err = float((ga - gb).abs().max() / gb.abs().max())
    assert err < 1e-9, err
    passes = {"vvd": vvd, "builtin": builtin}
    for run in passes.values():
        run()
    times = {k: [] for k in passes}
    for _ in range(5):
        for k, run in passes.items():
            times[k].append(device_ms(run))
    ms = {k: {"median_ms": sorted(v)[len(v) // 2], "all_ms": v} for k, v in times.items()}
    out = {"model": "upper", "dims": n, "rows": rows, "pairs": pairs, "table_megabytes": round(rows * 2 * n * n * 8 / 1e6, 1),
           "max_relative_difference_of_the_table_gradients": err, "passes": ms,
           "vvd_over_builtin": round(ms["vvd"]["median_ms"] / ms["builtin"]["median_ms"], 2)}
    log(f"upper n = {n}: {json.dumps(out)}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vvd_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vvd_time.py measures on a GPU and found none")

    def log(line):
        print(line, flush=True)
    result = {"device": torch.cuda.get_device_name(0),
              "timing": "device time between two events around forward + loss + backward, warm, median of 5, forms alternating"}
    for n, rows, pairs in SHAPES:
        result[f"upper-{n}"] = measure(n, rows, pairs, log)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
