"""GPU: the spd exponential map, logarithm, geodesic and geodesic RSGD step -- C-ABI sympa_spd_expmap /
sympa_spd_logmap / sympa_spd_geodesic / sympa_spd_rsgd_step_exp through ops, both kernel forms (the default dispatch: sixteen lanes
per row for n >= 3; SYMPA_FLAG_GENERIC: one row per lane), against the 100-digit fixtures and against the g++ build of the same
arithmetic; SymmetricPositiveDefinite.expmap / logmap / geodesic, RiemannianSGD(retraction="exp") and tools/train_siegel.py
--manifold spd --retraction exp.  Bounds: tests/spd_expmap_helpers.py (the same constants as the CPU build's)."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import spd_expmap_helpers as h

sys.path.insert(0, os.path.join(h.ROOT, "tools"))
pytestmark = pytest.mark.gpu
ROWS_ALL = (1, 5, 65)                       # every n
ROWS_EDGES = (3, 4, 63, 64, 130)            # n in EDGE_DIMS: the group-of-four and wave edges, a ragged tail over three blocks
EDGE_DIMS = (2, 5, 6, 11, 16)
SHAPES = [(n, b) for n in h.DIMS for b in ROWS_ALL] + [(n, b) for n in EDGE_DIMS for b in ROWS_EDGES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(group, x, p2, flags):
    from sympa_amd import ops
    if group["entry"] == "step":
        lr, wd = group["param"]
        return ops.spd_rsgd_step_exp_(x.clone(), p2, lr, wd, flags=flags)
    if group["entry"] == "exp":
        return ops.spd_expmap(x, p2, flags=flags)
    if group["entry"] == "log":
        return ops.spd_logmap(x, p2, flags=flags)
    return ops.spd_geodesic(x, p2, group["param"], flags=flags)


@pytest.mark.parametrize("n,b", SHAPES)
def test_kernels_against_fixtures_and_host_build(dev, n, b):
    """the fixture rows tiled to b rows, through the default dispatch and SYMPA_FLAG_GENERIC"""
    from sympa_amd import _lib, ops, selfcheck
    tally = h.Tally()
    try:
        for g in h.groups(n):
            idx = np.arange(max(b, 1)) % g["x"].shape[0]
            xs, p2 = np.ascontiguousarray(g["x"][idx]), np.ascontiguousarray(g["p2"][idx])
            host, st, _ = (h.hostsim_step(xs, p2, *g["param"]) if g["entry"] == "step" else h.hostsim_map(g["entry"], xs, p2, g["param"] or 0.0))
            assert st == 0
            x, second = _d(xs, dev), _d(p2, dev)
            for flags, form in ((0, "default"), (ops.FLAG_GENERIC, "generic")):
                got = _run(g, x, second, flags).cpu().numpy()
                ops.check_status(dev)
                assert np.array_equal(got, np.swapaxes(got, -1, -2)), f"{g['labels'][0]} {form}: outputs are symmetric bit for bit"
                tally.check(g, got, f"{form} b={b}")
                tally.check(g, got, f"{form} b={b} against g++", reference=host)
            assert torch.equal(x, _d(xs, dev)) and torch.equal(second, _d(p2, dev)), "inputs are left alone"
    finally:
        tally.report(f"MI355X n = {n} b = {b}")
    if n >= 3:
        assert not _lib.load().sympa_get_instance_fallback(selfcheck.SPD_TABLE, 0, n), "the self-check demoted the sixteen-lanes kernels"


@pytest.mark.parametrize("n", (2, 3, 8, 16))
def test_exact_properties_and_status(dev, n):
    from sympa_amd import ops
    g = next(g for g in h.groups(n) if g["entry"] == "log")
    x, y = _d(g["x"], dev), _d(g["p2"], dev)
    # tangents and gradients of moderate invariant length at every point: 0.3 x sym(v) x / (|x| |v| |x|)
    v = h.sym(np.random.default_rng(n).standard_normal(g["x"].shape))
    scale = 0.3 / (np.linalg.norm(g["x"], axis=(1, 2)) ** 2 * np.linalg.norm(v, axis=(1, 2)))
    u = _d(h.sym(g["x"] @ v @ g["x"]) * scale[:, None, None], dev)
    grad = _d(v * scale[:, None, None], dev)
    for flags in (0, ops.FLAG_GENERIC):
        assert torch.equal(ops.spd_expmap(x, torch.zeros_like(x), flags=flags), x)
        assert torch.equal(ops.spd_geodesic(x, y, 0.0, flags=flags), x)
        assert torch.equal(ops.spd_rsgd_step_exp_(x.clone(), grad, 0.0, 0.1, flags=flags), x)
        assert bool((ops.spd_logmap(x, x, flags=flags) == 0.0).all())
        ops.check_status(dev)
        # an indefinite row among good ones: flagged, counted once, NaN; its neighbours untouched by it
        bad = x.clone()
        bad[1] = -bad[1]
        for call in (lambda: ops.spd_expmap(bad, u, flags=flags), lambda: ops.spd_logmap(bad, y, flags=flags),
                     lambda: ops.spd_geodesic(bad, y, 0.3, flags=flags), lambda: ops.spd_rsgd_step_exp_(bad.clone(), grad, 0.01, flags=flags)):
            out = call()
            st = ops._status_buf(dev).cpu()
            ops._status_buf(dev).zero_()
            assert int(st[0]) == h.ST_NOT_PD and int(st[1]) == 1, st
            assert bool(torch.isnan(out[1]).all()) and bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[2:]).all())
    # b == 0 is a no-op; the folded clip equals a prescaled gradient to rounding
    empty = torch.empty(0, n, n, dtype=torch.float64, device=dev)
    assert ops.spd_expmap(empty, empty).shape == (0, n, n)
    sq = (grad * grad).sum().reshape(1)
    coef = min(1.0, 0.5 / (float(sq.sqrt()) + 1e-6))
    a = ops.spd_rsgd_step_exp_(x.clone(), grad, 0.05, 0.0, clip_sqnorm=sq, max_norm=0.5)
    b = ops.spd_rsgd_step_exp_(x.clone(), grad * coef, 0.05, 0.0)
    assert float((a - b).abs().max()) <= 64 * h.EPS64 * float(b.abs().max())


@pytest.mark.parametrize("n", (3, 8, 16))
def test_step_against_the_composition_of_the_separate_entries(dev, n):
    """sympa_spd_rsgd_step_exp against spd_expmap(x, -lr spd_egrad2rgrad(x, g + wd x)): within the expmap bound of that tangent, to
    which the rounding of the tangent itself (2 n eps lr |x| |S| |x|, carried through the map by kappa_row's dw) is added.  Bit for
    bit is not promised (a fused evaluation rounds differently)."""
    from sympa_amd import ops
    worst = 0.0
    for g in (g for g in h.groups(n) if g["entry"] == "step"):
        lr, wd = g["param"]
        x, grad = _d(g["x"], dev), _d(g["p2"], dev)
        stepped = ops.spd_rsgd_step_exp_(x.clone(), grad, lr, wd).cpu().numpy()
        u = -lr * ops.spd_egrad2rgrad(x, grad + wd * x)
        composed = ops.spd_expmap(x, u).cpu().numpy()
        ops.check_status(dev)
        for i in range(len(stepped)):
            xi, S = g["x"][i], g["p2"][i] + wd * g["x"][i]
            dw = 2.0 * lr * np.abs(xi) @ np.abs(S) @ np.abs(xi)
            kap = h.kappa_row("exp", xi, -lr * xi @ S @ xi, g["want"][i], dw=dw)
            unit = n * h.EPS64 * kap * np.abs(g["want"][i]).max()
            ratio = float(np.abs(stepped[i] - composed[i]).max() / unit)
            worst = max(worst, ratio)
            assert ratio <= h.C["exp"], (g["labels"][i], ratio)
    print(f"[spd expmap] step against composition, n = {n}: worst error / (n eps kappa max|want|) = {worst:.3g}")


def _spd_model(dims, nodes, dev, seed=1):
    from sympa_amd import data
    from sympa_amd.model import Model

    class A:
        pass
    A.manifold, A.metric, A.dims, A.num_points = "spd", "riem", dims, nodes
    A.scale_coef, A.scale_init, A.train_scale = 1.0, 1.0, False
    m = Model(A)
    with torch.no_grad():
        m.embeddings.embeds.data = data.spd_table(nodes, dims, scale=0.3, seed=seed)
    return m.to(dev)


def test_manifold_surface_and_optimizer(dev):
    """SymmetricPositiveDefinite.expmap / logmap / geodesic, and RiemannianSGD(retraction="exp") on a 16-node spd model, n = 3:
    30 steps of the classic loop, the loss falls and every row stays SPD"""
    import networkx as nx
    from sympa_amd import data, ops
    from sympa_amd.optim import RiemannianAdam, RiemannianSGD
    model = _spd_model(3, 16, dev)
    man, table = model.manifold, model.embeddings.embeds
    x, y = table.detach()[:8].contiguous(), table.detach()[8:].contiguous()
    lg = man.logmap(x, y)
    assert not lg.requires_grad and torch.equal(lg, ops.spd_logmap(x, y))
    assert torch.equal(man.expmap(x, lg), ops.spd_expmap(x, lg))
    mid = man.geodesic(0.5, x, y)
    assert torch.equal(mid, ops.spd_geodesic(x, y, 0.5))
    d, a, b = man.dist(x, y), man.dist(x, mid), man.dist(mid, y)
    assert float(((a - 0.5 * d).abs() / d).max()) < 1e-12 and float(((b - 0.5 * d).abs() / d).max()) < 1e-12
    assert float((man.expmap(x, lg) - y).abs().max()) < 1e-12 * float(y.abs().max())
    # retr stays geoopt's second-order retraction, and the Adam optimiser keeps refusing the table
    u = 0.1 * lg
    r, e = man.retr(x, u), man.expmap(x, u)
    assert not torch.equal(r, e) and float((r - e).abs().max()) < 1e-2 * float(e.abs().max())
    with pytest.raises(NotImplementedError, match="retraction='linear'"):
        RiemannianAdam(model.parameters(), lr=1e-2, retraction="exp")
    # one optimiser step equals the kernel on a copy, and differs from the linear step
    trip, _ = data.graph_triplets(nx.cycle_graph(16))
    ids, gd = trip[:, :2].to(torch.int64).contiguous().to(dev), trip[:, 2].to(torch.float64).to(dev)
    opt = RiemannianSGD(model.parameters(), lr=0.05, retraction="exp")
    opt.zero_grad(set_to_none=False)
    first = float(model.fused_loss_backward(ids, gd))
    want = ops.spd_rsgd_step_exp_(table.detach().clone(), table.grad, 0.05, 0.0)
    lin = ops.spd_rsgd_step_(table.detach().clone(), table.grad, 0.05, 0.0)
    opt.step()
    assert torch.equal(table.detach(), want) and not torch.equal(table.detach(), lin)
    losses = [first]
    for _ in range(29):
        opt.zero_grad(set_to_none=False)
        losses.append(float(model.fused_loss_backward(ids, gd)))
        torch.nn.utils.clip_grad_norm_(model.parameters(), 50.0)
        opt.step()
    ops.check_status(dev)
    print(f"[spd expmap] 16 nodes, n = 3, RiemannianSGD(retraction='exp'): loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < losses[0], losses
    t = table.detach()
    assert torch.equal(t, t.transpose(-1, -2)) and bool((torch.linalg.eigvalsh(t) > 0).all())


def test_train_siegel_spd_with_the_exponential_retraction():
    """tools/train_siegel.py --graph grid3d-125 --manifold spd --retraction exp (rsgd, the classic loop), dims 3, lr 0.3, 6 epochs,
    next to the linear run of the same seed: the distortion falls from ~1 to below 0.5, stays within 1.5 x the linear run's (three
    seeds at 10 epochs: linear 0.160 / 0.178 / 0.179, exp 0.202 / 0.172 / 0.189), and every point stays SPD;
    with --optim radam the tool exits with the optimiser's refusal"""
    import train_siegel
    argv = ["--graph", "grid3d-125", "--manifold", "spd", "--metric", "riem", "--dims", "3", "--epochs", "6", "--batch_size", "512",
            "--val_every", "3", "--learning_rate", "0.3", "--burnin", "0", "--seed", "42", "--no_graph_step", "--retraction"]
    model, hist = train_siegel.train(train_siegel.parser().parse_args(argv + ["exp"]), log=lambda *_: None)
    _, lin = train_siegel.train(train_siegel.parser().parse_args(argv + ["linear"]), log=lambda *_: None)
    print("[spd expmap] train_siegel spd exp: " + ", ".join(f"({e[0]}, {e[2]:.4f})" for e in hist) + "; linear: " +
          ", ".join(f"({e[0]}, {e[2]:.4f})" for e in lin))
    assert np.isfinite(hist[-1][1]) and hist[-1][2] < hist[0][2] and hist[-1][2] < 0.5, hist
    assert hist[-1][2] <= 1.5 * lin[-1][2], (hist, lin)
    t = model.embeddings.embeds.detach()
    assert bool((torch.linalg.eigvalsh(t) > 0).all())
    with pytest.raises(SystemExit, match="retraction='linear'"):
        train_siegel.train(train_siegel.parser().parse_args(argv + ["exp", "--optim", "radam"]), log=lambda *_: None)
