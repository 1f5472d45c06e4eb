#!/usr/bin/env python3
"""Timing of the vector models' kernels (csrc/vector_models.hip) on the GPU box: `euclidean`, `poincare` and `prod-hysph` at dims
20 and 272 on the table size of configs[3] (45 500 rows, 262 144 pairs per batch), in one process.

  forward   Model.forward under no_grad (sympa_vector_model_forward): gather, distance, scale -- one launch;
  backward  Model.fused_loss_backward: per-pair gradient rows with the loss fused (sympa_vector_backward_rows), then the
            scatter-add into the dense gradient (sympa_scatter_add_flat_rows) -- two launches;
  rsgd      RiemannianSGD.step over the whole table (sympa_vector_rsgd_step) -- one launch;
  torch_*   the same formulas written in torch ops on the same tensors (sympa_amd/manifolds/vector.py: torch_dist with two
            index gathers, AverageDistortionLoss + autograd, torch_rsgd_row), the formulation a user without the kernels has.

The forward is also set against a bytes roof: a pair reads two rows and two indices and writes one value, 2 dims 8 + 24 bytes, at
the measured HBM rate of 6.29 TB/s.  The 7.3 MB table of dims 20 stays resident in the L2s / Infinity Cache and the 99 MB table of
dims 272 in the Infinity Cache (256 MB), so gathered rows need not come from HBM and the kernel may beat that roof; the output says
where it does.  Kernel and torch results are compared before anything is timed.  Times are host clocks around work that ends in a
device synchronise, warm, median of 5, the forms alternating.  Recorded numbers only: nothing here is a threshold.

`--radam` measures the RiemannianAdam step instead (sympa_vector_radam_step, one launch, against torch_radam_row of
sympa_amd/manifolds/vector.py on the same tensors) with its bytes roof of 7 dims 8 bytes per row (read x, g, m, s; write x, m, s),
and writes profiles/vector_radam_time.json; the table says where the kernel loses to torch.

    python tools/vector_time.py [--out profiles/vector_time.json]
    python tools/vector_time.py --radam [--out profiles/vector_radam_time.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODELS = ("euclidean", "poincare", "prod-hysph")
DIMS = (20, 272)
ROWS, PAIRS = 45500, 262144
HBM_BYTES_PER_S = 6.29e12


def once_ms(run):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 4)


def spread_table(model, dims, dev):
    """A table as training leaves it: distances O(1) (the initial table has every point within 1e-3 of the origin)."""
    import torch
    from sympa_amd.manifolds import vector as mv
    g = torch.Generator().manual_seed(dims)
    x = torch.randn(ROWS, dims, generator=g, dtype=torch.float64)
    x = 0.7 * x / x.norm(dim=-1, keepdim=True) * torch.rand(ROWS, 1, generator=g, dtype=torch.float64)
    return mv.torch_projx(x, model)[0].to(dev).contiguous()


def measure(model, dims, log):
    import torch
    from sympa_amd import ops
    from sympa_amd.losses import AverageDistortionLoss
    from sympa_amd.manifolds import vector as mv
    from sympa_amd.model import Model
    from sympa_amd.optim import RiemannianSGD
    dev = torch.device("cuda:0")

    class A:
        manifold, metric, num_points = model, "riem", ROWS
        scale_coef, scale_init, train_scale = 1.0, 1.0, False
    A.dims = dims
    m = Model(A).to(dev)
    with torch.no_grad():
        m.embeddings.embeds.data = spread_table(model, dims, dev)
    emb = m.embeddings.embeds
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, ROWS, (PAIRS, 2), generator=g).to(dev)
    gd = torch.randint(1, 9, (PAIRS,), generator=g).to(torch.float64).to(dev)
    loss_fn = AverageDistortionLoss()
    opt = RiemannianSGD(m.parameters(), lr=1e-3)
    keep = ids[:, 0] != ids[:, 1]                      # torch's sqrt has no gradient at distance 0

    def forward():
        with torch.no_grad():
            return m(ids)

    def torch_forward():
        with torch.no_grad():
            t = emb.data
            return mv.torch_dist(t[ids[:, 0]], t[ids[:, 1]], model) * m.get_scale()

    def backward():
        emb.grad.zero_()
        return m.fused_loss_backward(ids, gd)

    def torch_backward():
        t = emb.data.clone().requires_grad_(True)
        i = ids[keep]
        d = mv.torch_dist(t[i[:, 0]], t[i[:, 1]], model)
        loss = loss_fn.calculate_loss(gd[keep], d)
        (gt,) = torch.autograd.grad(loss, t)
        return loss, gt

    # results first (the warm-up of every shape too)
    a, b = forward(), torch_forward()
    err_fwd = float(((a - b).abs() / b.abs().clamp_min(1e-300))[keep].max())
    emb.grad = torch.zeros_like(emb.data)
    la = backward()
    ga = emb.grad.clone()
    lb, gb = torch_backward()
    same = float((~keep).sum())                        # a pair with src == dst adds |0 - 1| = 1 to the loss and no gradient
    err_loss = abs(float(la) - float(lb) - same) / abs(float(lb))
    err_bwd = float((ga - gb).abs().max() / gb.abs().max())
    start = emb.data.clone()
    grad = ga * 1e-3
    emb.grad = grad.clone()
    opt.step()
    stepped = emb.data.clone()
    want = mv.torch_rsgd_row(start, grad, model, 1e-3)
    err_step = float((stepped - want).abs().max() / want.abs().max())
    assert ops.check_status(dev) == (0, 0)
    assert err_fwd < 1e-10 and err_loss < 1e-10 and err_bwd < 1e-9 and err_step < 1e-12, (err_fwd, err_loss, err_bwd, err_step)
    with torch.no_grad():
        emb.data.copy_(start)

    def rsgd():
        opt.step()                                     # (the table drifts by lr = 1e-3 steps of a 1e-3-scaled gradient: harmless)

    def torch_rsgd():
        with torch.no_grad():
            emb.data.copy_(mv.torch_rsgd_row(emb.data, emb.grad, model, 1e-3))

    passes = {"forward": forward, "torch_forward": torch_forward, "backward": backward, "torch_backward": torch_backward,
              "rsgd": rsgd, "torch_rsgd": torch_rsgd}
    for run in passes.values():
        run()
    times = {k: [] for k in passes}
    for _ in range(5):
        for k, run in passes.items():
            times[k].append(once_ms(run))
    out = {"rows": ROWS, "pairs": PAIRS, "dims": dims, "lanes_per_pair": min(64, 1 << max(0, (dims - 1).bit_length() - 2)),
           "table_megabytes": round(ROWS * dims * 8 / 1e6, 1),
           "max_relative_difference_kernel_torch": {"forward": err_fwd, "loss": err_loss, "gradient": err_bwd, "rsgd": err_step}}
    ms = {k: {"median_ms": sorted(v)[len(v) // 2], "all_ms": v} for k, v in times.items()}
    out["passes"] = ms
    out["torch_over_kernel"] = {k: round(ms["torch_" + k]["median_ms"] / ms[k]["median_ms"], 2) for k in ("forward", "backward", "rsgd")}
    roof_ms = PAIRS * (2 * dims * 8 + 24) / HBM_BYTES_PER_S * 1e3
    out["forward_bytes_roof_ms"] = round(roof_ms, 4)
    out["forward_over_roof"] = round(ms["forward"]["median_ms"] / roof_ms, 2)
    out["forward_beats_the_hbm_roof"] = ms["forward"]["median_ms"] < roof_ms       # possible: the rows come out of cache
    log(f"{model} dims {dims}: {json.dumps(out)}")
    return out


def measure_radam(model, dims, log):
    """The RiemannianAdam step over the same table (sympa_vector_radam_step, one launch) against torch_radam_row on the same
    tensors.  Bytes roof: a row reads x, g, m, s and writes x, m, s: 7 dims 8 bytes."""
    import torch
    from sympa_amd import ops
    from sympa_amd.manifolds import vector as mv
    from sympa_amd.manifolds.base import ManifoldParameter
    from sympa_amd.optim import RiemannianAdam
    dev = torch.device("cuda:0")
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-7
    table = spread_table(model, dims, dev)
    p = ManifoldParameter(table.clone(), manifold=mv.get_vector_manifold(model, dims))
    g = torch.Generator().manual_seed(2)
    grad = (torch.randn(ROWS, dims, generator=g, dtype=torch.float64) / dims ** 0.5).to(dev)
    p.grad = grad
    opt = RiemannianAdam([p], lr=lr, betas=betas, eps=eps)
    # results first: three steps of the optimiser against three torch rows (the warm-up too)
    x, m, s = table.clone(), torch.zeros_like(table), torch.zeros_like(table)
    for t in (1, 2, 3):
        opt.step()
        x, m, s = mv.torch_radam_row(x, grad, m, s, (betas[0] ** t, betas[1] ** t), model, lr, betas, eps)
    st = opt.state[p]
    errs = {"x": float((p.data - x).abs().max() / x.abs().max()), "exp_avg": float((st["exp_avg"] - m).abs().max() / m.abs().max()),
            "exp_avg_sq": float((st["exp_avg_sq"] - s).abs().max() / s.abs().max())}
    assert ops.check_status(dev) == (0, 0)
    assert max(errs.values()) < 1e-10, errs
    pows = torch.tensor([betas[0] ** 4, betas[1] ** 4], dtype=torch.float64, device=dev)
    state = [x, m, s]

    def radam():
        opt.step()                                     # (the table drifts by lr = 1e-3 steps: harmless)

    def torch_radam():
        with torch.no_grad():
            state[0], state[1], state[2] = mv.torch_radam_row(state[0], grad, state[1], state[2], pows, model, lr, betas, eps)

    passes = {"radam": radam, "torch_radam": torch_radam}
    for run in passes.values():
        run()
    times = {k: [] for k in passes}
    for _ in range(5):
        for k, run in passes.items():
            times[k].append(once_ms(run))
    ms = {k: {"median_ms": sorted(v)[len(v) // 2], "all_ms": v} for k, v in times.items()}
    roof_ms = ROWS * 7 * dims * 8 / HBM_BYTES_PER_S * 1e3
    out = {"rows": ROWS, "dims": dims, "lanes_per_row": min(64, 1 << max(0, (dims - 1).bit_length() - 2)),
           "table_megabytes": round(ROWS * dims * 8 / 1e6, 1), "max_relative_difference_kernel_torch_after_3_steps": errs,
           "passes": ms, "torch_over_kernel": round(ms["torch_radam"]["median_ms"] / ms["radam"]["median_ms"], 2),
           "kernel_loses_to_torch": ms["radam"]["median_ms"] > ms["torch_radam"]["median_ms"],
           "bytes_roof_ms": round(roof_ms, 4), "radam_over_roof": round(ms["radam"]["median_ms"] / roof_ms, 2)}
    log(f"{model} dims {dims} radam: {json.dumps(out)}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radam", action="store_true",
                    help="measure the RiemannianAdam step alone (default --out: profiles/vector_radam_time.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "vector_radam_time.json" if args.radam else "vector_time.json")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vector_time.py measures on a GPU and found none")

    def log(line):
        print(line, flush=True)
    result = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S,
              "timing": "host clock around a pass that ends in a device synchronise, warm, median of 5, forms alternating"}
    for model in MODELS:
        for dims in DIMS:
            result[f"{model}-{dims}"] = measure_radam(model, dims, log) if args.radam else measure(model, dims, log)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
