"""RiemannianAdam on the spd model on the GPU: sympa_spd_radam_step through the optimiser and through
ops.spd_radam_step_, both kernels (one row per lane; sixteen lanes per row) against the 50-digit fixtures within the bounds of
tests/spd_radam_helpers.py, partial waves inside guarded buffers, the folded clip, graph capture and training."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from tests import spd_radam_helpers as rh  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GENERIC_DIMS = (3, 7, 16)


def _param(x):
    from sympa_amd.manifolds.base import ManifoldParameter
    from sympa_amd.manifolds.spd import SymmetricPositiveDefinite
    return ManifoldParameter(torch.as_tensor(x, dtype=torch.float64).to(DEV).contiguous(), manifold=SymmetricPositiveDefinite())


def _settings(n):
    """the fixture cells of dims n grouped per (state, lr, wd): one optimiser step serves the ten rows of the five cases"""
    groups = {}
    for cell in rh.cells(n):
        groups.setdefault((cell["state"], cell["lr"], cell["wd"]), []).append(cell)
    return groups


def optimiser_step(cells, lr, wd):
    """the rows of `cells` (same state and setting) as one table through RiemannianAdam.step(); -> y, exp_avg, exp_avg_sq (numpy)"""
    from sympa_amd.optim import RiemannianAdam
    p = _param(np.concatenate([c["x"] for c in cells]))
    opt = RiemannianAdam([p], lr=lr, betas=rh.BETAS, eps=rh.EPS_ADAM, weight_decay=wd)
    opt.init_state()
    st = opt.state[p]
    st["exp_avg"].copy_(torch.from_numpy(np.concatenate([c["m"] for c in cells])))
    st["exp_avg_sq"].copy_(torch.from_numpy(np.concatenate([c["s"] for c in cells])))
    st["bias_pows"].copy_(torch.from_numpy(cells[0]["pows_prev"]))
    opt.param_groups[0]["step"] = cells[0]["t"] - 1
    p.grad = torch.from_numpy(np.concatenate([c["g"] for c in cells])).to(DEV)
    opt.step()
    return p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()


def check_dims(n, tally):
    from sympa_amd import ops
    for (state, lr, wd), cells in _settings(n).items():
        y, m, s = optimiser_step(cells, lr, wd)
        assert (y == np.swapaxes(y, 1, 2)).all() and (m == np.swapaxes(m, 1, 2)).all(), (n, state, lr, wd)      # bit for bit
        for k, cell in enumerate(cells):
            tally.check(cell, y[2 * k:2 * k + 2], m[2 * k:2 * k + 2], s[2 * k:2 * k + 2], "RiemannianAdam.step")
            if cell["case"] == "diag":
                off = ~np.eye(n, dtype=bool)
                assert not y[2 * k:2 * k + 2][:, off].any() and not m[2 * k:2 * k + 2][:, off].any(), cell["label"]
    assert ops.check_status(torch.device(DEV))[0] == 0


def _not_demoted(n):
    from sympa_amd import _lib, selfcheck
    assert not selfcheck.FAILURES, selfcheck.FAILURES
    assert not _lib.load().sympa_get_instance_fallback(selfcheck.SPD_TABLE, 0, n), \
        f"the self-check demoted the spd table instantiation n={n}: the step ran the one-lane kernel"


@pytest.mark.parametrize("n", rh.DIMS)
def test_every_fixture_through_the_optimiser(n):
    """n <= 2: the one-row-per-lane kernel; n >= 3: sixteen lanes per row (and the self-check must not have demoted it)"""
    tally = rh.Tally(rh.C_ONE_LANE if n <= 2 else rh.C_SIXTEEN_LANES)
    check_dims(n, tally)
    if n >= 3:
        _not_demoted(n)
    tally.report(f"MI355X n={n}, " + ("one row per lane" if n <= 2 else "sixteen lanes per row"))


def child_main():
    """runs in a fresh process started with SYMPA_SPD_TABLE_GENERIC=1: the dispatcher reads the variable once per process"""
    assert os.environ.get("SYMPA_SPD_TABLE_GENERIC") == "1"
    tally = rh.Tally(rh.C_ONE_LANE)
    for n in GENERIC_DIMS:
        check_dims(n, tally)
    tally.report("MI355X one row per lane (SYMPA_SPD_TABLE_GENERIC=1), n in %s" % (GENERIC_DIMS,))
    print("generic-ok")


def test_every_fixture_through_the_one_lane_kernel_in_a_child_process():
    env = dict(os.environ, SYMPA_SPD_TABLE_GENERIC="1")
    res = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) +
                         ["-c", "import tests.test_spd_radam_gpu as t; t.child_main()"], cwd=rh.ROOT, env=env, capture_output=True,
                         text=True, timeout=300)
    print(res.stdout[-2000:])
    assert res.returncode == 0 and "generic-ok" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


SENTINEL = -7.25e77
PAD = 64


def _guarded(values):
    """a copy of `values` inside a buffer with PAD sentinels on both sides; -> (buffer, view)"""
    flat = torch.as_tensor(values, dtype=torch.float64).reshape(-1)
    buf = torch.full((flat.numel() + 2 * PAD,), SENTINEL, dtype=torch.float64, device=DEV)
    view = buf[PAD:PAD + flat.numel()].view(tuple(np.shape(values)))
    view.copy_(flat.view(view.shape))
    return buf, view


def _intact(buf):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())


@pytest.mark.parametrize("n", (3, 11, 16))
def test_partial_waves_inside_guarded_buffers(n):
    """1, 3, 4, 5, 130 rows and 4 101 rows (two rounds per wave, the last wave with one live row in its second round): the
    fixture rows of the `later`, lr = 1 setting tiled; every row within its bound, nothing written outside the three tensors"""
    from sympa_amd import ops
    cells = _settings(n)[("later", 1.0, 0.0)]
    x, g, m = (np.concatenate([c[k] for c in cells]) for k in ("x", "g", "m"))
    s = np.concatenate([c["s"] for c in cells])
    wy, wm = (np.concatenate([c["want"][k] for c in cells]) for k in ("y", "m"))
    ws = np.concatenate([c["want"]["s1"] for c in cells])
    by, bm, bs = (np.concatenate(b) for b in zip(*(rh.bounds(c, rh.C_SIXTEEN_LANES) for c in cells)))
    pows = torch.from_numpy(cells[0]["pows"]).to(DEV)
    for rows in (1, 3, 4, 5, 130, 4101):
        idx = np.arange(rows) % x.shape[0]
        (bx, tx), (bm_, tm), (bs_, ts) = _guarded(x[idx]), _guarded(m[idx]), _guarded(s[idx])
        ops.spd_radam_step_(tx, torch.from_numpy(g[idx]).to(DEV), tm, ts, pows, 1.0, rh.BETAS, rh.EPS_ADAM, 0.0)
        torch.cuda.synchronize()
        assert _intact(bx) and _intact(bm_) and _intact(bs_), (n, rows)
        assert (np.abs(tx.cpu().numpy() - wy[idx]).max((1, 2)) <= by[idx]).all(), (n, rows)
        assert (np.abs(tm.cpu().numpy() - wm[idx]).max((1, 2)) <= bm[idx]).all(), (n, rows)
        assert (np.abs(ts.cpu().numpy() - ws[idx]) <= bs[idx]).all(), (n, rows)
        assert torch.equal(tx, tx.transpose(1, 2)) and torch.equal(tm, tm.transpose(1, 2)), (n, rows)
    assert ops.check_status(torch.device(DEV))[0] == 0
    _not_demoted(n)


@pytest.mark.parametrize("n", (2, 9))
def test_two_optimiser_steps_equal_two_hand_driven_launches(n):
    from sympa_amd import ops
    from sympa_amd.optim import RiemannianAdam
    cells = _settings(n)[("first", 0.01, 0.1)]
    x = np.concatenate([c["x"] for c in cells])
    g1 = np.concatenate([c["g"] for c in cells])
    g2 = g1[::-1].copy()
    p = _param(x)
    opt = RiemannianAdam([p], lr=0.01, betas=rh.BETAS, eps=rh.EPS_ADAM, weight_decay=0.1)
    t, m, s = _param(x).data, torch.zeros(x.shape, dtype=torch.float64, device=DEV), torch.zeros(x.shape[0], dtype=torch.float64, device=DEV)
    pows, betas = torch.ones(2, dtype=torch.float64, device=DEV), torch.tensor(rh.BETAS, dtype=torch.float64, device=DEV)
    for g in (g1, g2):
        p.grad = torch.from_numpy(g).to(DEV)
        opt.step()
        pows.mul_(betas)
        ops.spd_radam_step_(t, torch.from_numpy(g).to(DEV), m, s, pows, 0.01, rh.BETAS, rh.EPS_ADAM, 0.1)
    st = opt.state[p]
    assert torch.equal(p.data, t) and torch.equal(st["exp_avg"], m) and torch.equal(st["exp_avg_sq"], s)
    assert torch.equal(st["bias_pows"], pows) and st["exp_avg_sq"].shape == (x.shape[0],)


@pytest.mark.parametrize("n", (2, 8))
def test_folded_clip_equals_a_prescaled_gradient(n):
    from sympa_amd import ops
    cells = _settings(n)[("later", 1.0, 0.0)]
    x, g, m = (np.concatenate([c[k] for c in cells]) for k in ("x", "g", "m"))
    s = np.concatenate([c["s"] for c in cells])
    pows = torch.from_numpy(cells[0]["pows"]).to(DEV)
    total = float((g * g).sum()) * 4.0          # as if other parameters added to the norm
    max_norm = 0.25 * np.sqrt(total)
    coef = min(1.0, max_norm / (np.sqrt(total) + 1e-6))
    assert coef < 0.26
    outs = []
    for grad, kw in ((g, dict(clip_sqnorm=torch.tensor([total], dtype=torch.float64, device=DEV), max_norm=max_norm)), (coef * g, {})):
        t, tm, ts = _param(x).data, torch.from_numpy(m).to(DEV), torch.from_numpy(s).to(DEV)
        ops.spd_radam_step_(t, torch.from_numpy(grad).to(DEV), tm, ts, pows, 1.0, rh.BETAS, rh.EPS_ADAM, 0.0, **kw)
        outs.append([a.cpu().numpy() for a in (t, tm, ts)])
    C = rh.C_ONE_LANE if n <= 2 else rh.C_SIXTEEN_LANES
    for i in range(x.shape[0]):
        want = {"y": outs[1][0][i], "m": outs[1][1][i]}
        ky, km, ks = rh._kappa_row(x[i], coef * g[i], m[i], s[i], cells[0]["pows"], 1.0, 0.0, want)
        unit = 2.0 * C * n * rh.EPS64            # both runs carry their own rounding
        assert np.abs(outs[0][0][i] - want["y"]).max() <= unit * ky * np.abs(want["y"]).max(), i
        assert np.abs(outs[0][1][i] - want["m"]).max() <= unit * km * np.abs(want["m"]).max(), i
        assert abs(outs[0][2][i] - outs[1][2][i]) <= unit * ks * outs[1][2][i], i


def test_manifold_transp_is_a_second_route_to_exp_avg():
    """64 random rows at n = 5: exp_avg of the kernel (the cubic polynomial) against SymmetricPositiveDefinite.transp (E m1 E^T
    through eigh) of the same m1 to the kernel's y, at the eigh route's tolerance (tests/test_spd_radam_cpu.py: 20 n eps cond x)"""
    from sympa_amd import data, ops
    from sympa_amd.manifolds.spd import SymmetricPositiveDefinite
    man, n, rows = SymmetricPositiveDefinite(), 5, 64
    gen = torch.Generator().manual_seed(11)
    x = data.spd_table(rows, n, scale=0.5, seed=3).to(DEV)
    g = torch.randn(rows, n, n, generator=gen, dtype=torch.float64)
    g = (0.5 * (g + g.transpose(1, 2))).to(DEV)
    m0 = torch.randn(rows, n, n, generator=gen, dtype=torch.float64)
    m0 = x @ (0.5 * (m0 + m0.transpose(1, 2))).to(DEV) @ x
    m0 = 0.5 * (m0 + m0.transpose(1, 2))
    s0 = man.inner(x, x @ g @ x) * 0.002
    pows = torch.tensor([0.9 ** 7, 0.999 ** 7], dtype=torch.float64, device=DEV)
    y, m, s = x.clone(), m0.clone(), s0.clone()
    ops.spd_radam_step_(y, g, m, s, pows, 1.0, rh.BETAS, rh.EPS_ADAM, 0.0)
    m1 = 0.9 * m0 + (1.0 - 0.9) * (x @ g @ x)
    want = man.transp(x, y, m1)
    tol = 20.0 * n * rh.EPS64 * torch.linalg.cond(x) * want.abs().amax((1, 2))
    assert ((m - want).abs().amax((1, 2)) <= tol).all()
    assert float((m - m1).abs().max()) > 1e-3 * float(m1.abs().max())          # the transport did move exp_avg


@pytest.mark.parametrize("n", (2, 6, 16))
def test_fifty_steps_at_lr_one_stay_on_the_manifold(n):
    from sympa_amd import data, ops
    from sympa_amd.optim import RiemannianAdam
    p = _param(data.spd_table(64, n, scale=0.3, seed=5))
    opt = RiemannianAdam([p], lr=1.0, eps=rh.EPS_ADAM)
    gen = torch.Generator().manual_seed(n)
    for _ in range(50):
        g = torch.randn(64, n, n, generator=gen, dtype=torch.float64)
        p.grad = (0.5 * (g + g.transpose(1, 2))).to(DEV)
        opt.step()
    assert ops.check_status(torch.device(DEV))[0] == 0
    assert torch.isfinite(p).all() and p.manifold.check_point_on_manifold(p.detach())
    assert bool((torch.linalg.eigvalsh(p.detach()) > 0).all())


def _spd_model(dims, nodes, seed=1):
    from sympa_amd import data
    from sympa_amd.model import Model

    class A:
        pass
    A.manifold, A.metric, A.dims, A.num_points = "spd", "riem", dims, nodes
    A.scale_coef, A.scale_init, A.train_scale = 2.0, 1.5, True
    m = Model(A)
    with torch.no_grad():
        m.embeddings.embeds.data = data.spd_table(nodes, dims, scale=0.3, seed=seed)
    return m.to(DEV)


def _eager_steps(model, opt, batches, out=None):
    for ids, gd in batches:
        opt.zero_grad(set_to_none=False)
        model.fused_loss_backward(ids, gd)
        torch.nn.utils.clip_grad_norm_(model.parameters(), 50.0)
        opt.step()


def test_riemannian_adam_on_spd_captured_in_a_graph():
    """`--manifold spd --optim radam` under GraphedTrainStep (classic mode): five replays equal five eager steps at the tolerances
    of test_riemannian_adam_step_captured_in_a_graph, 1e-11 relative on the table and 1e-12 on exp_avg.  Those are used as they
    stand: measured on the MI355X, two identical eager runs differ by 1.5e-16 (table) and 3.3e-16 (exp_avg) through the backward's
    atomic scatter, the graph and the eager run by 3.0e-16 and 2.7e-16; the test prints both."""
    from sympa_amd import data
    from sympa_amd.optim import RiemannianAdam
    from sympa_amd.train_step import GraphedTrainStep
    dev = torch.device(DEV)
    nodes, b = 300, 2048
    gen = torch.Generator().manual_seed(9)
    batches = []
    for it in range(5):
        ids = data.sample_pairs(nodes, b, it, 1).to(dev)
        batches.append((ids[:, :2].contiguous(), (torch.rand(b, generator=gen, dtype=torch.float64) * 5 + 1).to(dev)))
    models = [_spd_model(3, nodes) for _ in range(3)]
    opts = [RiemannianAdam(m.parameters(), lr=0.02, eps=1e-7, stabilize=None) for m in models]
    stepper = GraphedTrainStep(models[0], opts[0], b, 50.0, dev, two_kernels=False)
    assert stepper.mode == "classic"
    for ids, gd in batches:
        stepper(ids, gd)
    _eager_steps(models[1], opts[1], batches)
    _eager_steps(models[2], opts[2], batches)
    ta, tb, tc = (m.embeddings.embeds.detach() for m in models)
    sa, sb, sc = (o.state[m.embeddings.embeds] for o, m in zip(opts, models))
    print(f"[spd radam] eager against eager: table {float((tb - tc).abs().max()) / float(tb.abs().max()):.3g}, exp_avg "
          f"{float((sb['exp_avg'] - sc['exp_avg']).abs().max()) / float(sb['exp_avg'].abs().max()):.3g};  graph against eager: table "
          f"{float((ta - tb).abs().max()) / float(tb.abs().max()):.3g}, exp_avg "
          f"{float((sa['exp_avg'] - sb['exp_avg']).abs().max()) / float(sb['exp_avg'].abs().max()):.3g}")
    assert float((ta - tb).abs().max()) < 1e-11 * float(tb.abs().max())
    assert abs(float(models[0].scale.detach()) - float(models[1].scale.detach())) < 1e-12
    assert abs(float(sa["bias_pows"][0]) - 0.9 ** 5) < 1e-14 and abs(float(sb["bias_pows"][0]) - 0.9 ** 5) < 1e-14
    assert float((sa["exp_avg"] - sb["exp_avg"]).abs().max()) < 1e-12 * float(sb["exp_avg"].abs().max())
    assert sa["exp_avg_sq"].shape == (nodes,)


@pytest.mark.parametrize("dims,epochs", [(3, 30), (16, 10)])
def test_train_siegel_spd_radam(dims, epochs):
    """tools/train_siegel.py --graph grid3d-125 --manifold spd --optim radam: the distortion falls and every point stays SPD.
    Measured histories (epoch, distortion), no ratio promised: dims 3: (5, 0.7482), (10, 0.6735), (15, 0.6261), (20, 0.6001),
    (25, 0.5815), (30, 0.5666);  dims 16: (5, 0.7378), (10, 0.6791)"""
    import train_siegel
    args = train_siegel.parser().parse_args(["--graph", "grid3d-125", "--manifold", "spd", "--metric", "riem", "--dims", str(dims),
                                             "--epochs", str(epochs), "--batch_size", "512", "--optim", "radam", "--val_every", "5",
                                             "--learning_rate", "0.01", "--burnin", "0"])
    model, hist = train_siegel.train(args, log=lambda *_: None)
    print(f"[spd radam] train_siegel dims={dims}: " + ", ".join(f"({h[0]}, {h[2]:.4f})" for h in hist))
    assert hist[-1][2] < hist[0][2], hist
    ok, point, reason = model.check_all_points()
    assert ok, reason
    assert bool((torch.linalg.eigvalsh(model.embeddings.embeds.detach()) > 0).all())
