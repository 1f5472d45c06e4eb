#!/usr/bin/env python3
"""Device time of the geodesic RiemannianAdam step (sympa_radam_step_exp), same process, interleaved:

    python tools/radam_exp_time.py [--rounds 40] [--limit 20] [--out profiles/radam_exp_time.json]

Tables: those of tools/transp_time.py -- bench.py's headline table (5 041 rows, n = 4) and 45 500 rows at n = 8
(data.trained_like_table), both models.  Rows per table, each a hipGraph of 8 launches replayed `rounds` times, the rows
alternating inside every round, device events around each replay (the median is the figure, the minimum is printed next to it):
  radam_step_exp   sympa_radam_step_exp: the whole step in one launch
  composed         the same step from the entries that existed before it, as tests/test_radam_exp_gpu.py composes it: egrad2rgrad,
                   sym and the moments in torch, the invariant norm, transp_exp with the point, projx, three copies back.  The norm
                   is taken by sympa_tangent_sqnorm (bounded: at conj g) instead of
                   SiegelManifold.invariant_inner, whose torch.linalg.inv does not go into a captured graph
  radam_step       the linear sympa_radam_step, where it exists (n <= 6)
Every row steps its own copy of the table and of the moments in place, from one fixed random symmetric gradient, lr = 1e-3 and
the powers of t = 5 held fixed: over the 8 x (rounds + 4) steps of a row the table drifts by an invariant length of about 0.4
and stays inside the domain.
Every launch and every replay runs under its own time limit (--limit seconds): the host polls the event behind it and, when the
limit passes, leaves the process at once with exit status 124 and starts nothing more on the device.
No ratio is promised; the numbers are recorded."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import transp_time as tt  # noqa: E402
from sympa_amd import data, ops  # noqa: E402

LR, BETAS, EPS_ADAM, T = 1e-3, (0.9, 0.999), 1e-7, 5


def rows_for(model, n, nodes, dev, rounds):
    table = data.trained_like_table(nodes, n, model=model).to(dev).contiguous()
    gen = torch.Generator(device=dev).manual_seed(3)
    grad = torch.randn(table.shape, dtype=torch.float64, device=dev, generator=gen)
    grad = (grad + grad.transpose(-1, -2)).contiguous()     # symmetric, as the gradient of a loss of a symmetric table is: the linear
    #                                                         step takes its norm as a trace, which is a norm on symmetric tangents only
    pows = torch.tensor([BETAS[0] ** T, BETAS[1] ** T], dtype=torch.float64, device=dev)
    bc1, bc2 = 1.0 - BETAS[0] ** T, 1.0 - BETAS[1] ** T
    sym = lambda a: 0.5 * (a + a.transpose(-1, -2))
    conj = torch.tensor([1.0, -1.0], dtype=torch.float64, device=dev).view(1, 2, 1, 1)

    def state():
        return table.clone(), torch.zeros_like(table), torch.zeros(nodes, dtype=torch.float64, device=dev)

    def fused(x, m, s):
        return lambda: ops.radam_step_exp_(x, grad, m, s, pows, model, LR, BETAS, EPS_ADAM, 0.0)

    def linear(x, m, s):
        return lambda: ops.radam_step_(x, grad, m, s, pows, model, LR, BETAS, EPS_ADAM, 0.0)

    def composed(x, m, s):
        def step():
            g = sym(ops.egrad2rgrad(x, grad, model))
            m1 = BETAS[0] * sym(m) + (1.0 - BETAS[0]) * g
            s1 = BETAS[1] * s + (1.0 - BETAS[1]) * ops.tangent_sqnorm(x, g * conj if model == "bounded" else g, model)
            alpha = LR / (bc1 * ((s1 / bc2).sqrt() + EPS_ADAM))
            y, mt = ops.transp_exp(x, -alpha.view(-1, 1, 1, 1) * m1, m1, model, return_point=True)
            x.copy_(ops.projx(y, model))
            m.copy_(mt)
            s.copy_(s1)
        return step

    work = {"radam_step_exp": fused(*state()), "composed": composed(*state())}
    if n <= ops.RADAM_FUSED_MAX_DIMS:
        work["radam_step"] = linear(*state())
    tag = f"{model} n={n} rows={nodes}"
    t = tt.time_interleaved({k: tt.graph_of(f, f"{tag} {k}") for k, f in work.items()}, rounds)
    rec = {k: {"median_us": x[len(x) // 2], "min_us": x[0]} for k, x in t.items()}
    torch.cuda.synchronize()
    ops.check_status(dev)
    print(f"{tag}: " + ", ".join(f"{k} {rec[k]['median_us']:.1f} us (min {rec[k]['min_us']:.1f})" for k in work), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--limit", type=float, default=tt.LIMIT, help="seconds a single launch or replay may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tt.LIMIT = args.limit
    assert torch.cuda.is_available(), "radam_exp_time.py measures device time: it needs the GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "launches_per_replay": tt.LAUNCHES, "rounds": args.rounds}
    for model in ops.EXPMAP_MODELS:
        res[f"{model}_n4_5041"] = rows_for(model, 4, 5041, dev, args.rounds)
        res[f"{model}_n8_45500"] = rows_for(model, 8, 45500, dev, args.rounds)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
