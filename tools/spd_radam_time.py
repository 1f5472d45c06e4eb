"""Timing record of the spd model's RiemannianAdam step (sympa_spd_radam_step): the 100 000-row table of
configs[4] at n = 16 and the same row count at n = 4.  In one run, alternating: the kernel step (RiemannianAdam.step, one launch),
(a) manifolds.spd.torch_radam_row on the same tensors, (b) the existing ops.spd_rsgd_step_ on the same table.  Results are compared
first (kernel against torch_radam_row after one step from a non-zero state), then timed: host clock around a pass that ends in
a device synchronise, warm, median of 5.  Bytes roof: (4 n^2 + 1) doubles read and (2 n^2 + 1) written per row at 6.29 TB/s.

    python tools/spd_radam_time.py [--out profiles/spd_radam_time.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = 100_000
DIMS = (16, 4)
HBM_BYTES_PER_S = 6.29e12


def once_ms(run):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(n, log):
    import torch
    from sympa_amd import data, ops
    from sympa_amd.manifolds.base import ManifoldParameter
    from sympa_amd.manifolds.spd import SymmetricPositiveDefinite, torch_radam_row
    from sympa_amd.optim import RiemannianAdam
    dev = torch.device("cuda:0")
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-7
    man = SymmetricPositiveDefinite()
    table = data.spd_table(ROWS, n, scale=0.3, seed=7).to(dev)
    gen = torch.Generator().manual_seed(2)
    grad = torch.randn(ROWS, n, n, generator=gen, dtype=torch.float64)
    grad = (0.5 * (grad + grad.transpose(1, 2)) / n).to(dev)
    # results first: one step from a non-zero state (t = 4) through the kernel and through torch_radam_row
    m0 = table @ grad.roll(1, 0) @ table
    m0 = 0.5 * (m0 + m0.transpose(1, 2))
    s0 = man.inner(table, m0) * 0.01
    pows = torch.tensor([betas[0] ** 4, betas[1] ** 4], dtype=torch.float64, device=dev)
    xk, mk, sk = table.clone(), m0.clone(), s0.clone()
    ops.spd_radam_step_(xk, grad, mk, sk, pows, lr, betas, eps, 0.0)
    xt, mt, st = torch_radam_row(man, table, grad, m0, s0, pows, lr, betas, eps)
    errs = {"x": float((xk - xt).abs().max() / xt.abs().max()), "exp_avg": float((mk - mt).abs().max() / mt.abs().max()),
            "exp_avg_sq": float(((sk - st).abs() / st).max())}
    assert ops.check_status(dev) == (0, 0)
    assert max(errs.values()) < 1e-10, errs
    p = ManifoldParameter(table.clone(), manifold=man)
    p.grad = grad
    opt = RiemannianAdam([p], lr=lr, betas=betas, eps=eps)
    state = [table.clone(), m0.clone(), s0.clone()]
    rsgd_table = table.clone()

    def radam():
        opt.step()                                     # (the table drifts by lr = 1e-3 steps: harmless)

    def torch_radam():
        with torch.no_grad():
            state[0], state[1], state[2] = torch_radam_row(man, state[0], grad, state[1], state[2], pows, lr, betas, eps)

    def rsgd():
        ops.spd_rsgd_step_(rsgd_table, grad, lr)

    passes = {"radam": radam, "torch_radam": torch_radam, "rsgd": rsgd}
    for run in passes.values():
        run()
    times = {k: [] for k in passes}
    for _ in range(5):
        for k, run in passes.items():
            times[k].append(once_ms(run))
    ms = {k: {"median_ms": sorted(v)[len(v) // 2], "all_ms": v} for k, v in times.items()}
    roof_ms = ROWS * (6 * n * n + 2) * 8 / HBM_BYTES_PER_S * 1e3
    out = {"rows": ROWS, "n": n, "kernel": "sixteen lanes per row" if n >= 3 else "one row per lane",
           "table_megabytes": round(ROWS * n * n * 8 / 1e6, 1), "max_relative_difference_kernel_torch_after_1_step": errs,
           "passes": ms, "torch_over_kernel": round(ms["torch_radam"]["median_ms"] / ms["radam"]["median_ms"], 2),
           "kernel_over_rsgd_step": round(ms["radam"]["median_ms"] / ms["rsgd"]["median_ms"], 2),
           "bytes_roof_ms": round(roof_ms, 4), "kernel_over_bytes_roof": round(ms["radam"]["median_ms"] / roof_ms, 2)}
    log(f"spd n = {n} radam: {json.dumps(out)}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spd_radam_time.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spd_radam_time.py measures on a GPU and found none")
    result = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S,
              "timing": "host clock around a pass that ends in a device synchronise, warm, median of 5, forms alternating"}
    for n in DIMS:
        result[f"spd-{n}"] = measure(n, lambda line: print(line, flush=True))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
