"""RiemannianAdam for the vector models on the MI355X (vec_radam_kernel of csrc/vector_models.hip): every fixture of
tools/make_golden_vector_radam_exact.py through RiemannianAdam.step within the bounds of tests/vector_radam_helpers.py; tables
that do not fill their last wave inside guarded buffers; the step against hand-driven kernel calls; the folded clip; the status
word; the manifold's transp as a second route to exp_avg; training."""
import numpy as np
import pytest
import torch

from tests import vector_helpers as vh
from tests import vector_radam_helpers as rh
from tests.test_vector_gpu import _d, make_model, tree_csr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _param(model, dims, x, dev):
    from sympa_amd.embeddings import ManifoldFactory
    from sympa_amd.manifolds.base import ManifoldParameter
    man = ManifoldFactory.get_manifold(model, "riem", dims)
    return ManifoldParameter(_d(x, dev).clone(), manifold=man), man


def _optimiser(p, fx, lr, wd, dev):
    """RiemannianAdam([p]) in the fixture's state: exp_avg, exp_avg_sq, bias_pows = betas^(t-1), step = t - 1"""
    from sympa_amd.optim import RiemannianAdam
    opt = RiemannianAdam([p], lr=lr, betas=rh.BETAS, eps=rh.EPS_ADAM, weight_decay=wd)
    opt.init_state()
    st = opt.state[p]
    st["exp_avg"].copy_(_d(fx["m"], dev))
    st["exp_avg_sq"].copy_(_d(fx["s"], dev))
    st["bias_pows"].copy_(_d(fx["pows_prev"], dev))
    opt.param_groups[0]["step"] = fx["t"] - 1
    return opt, st


@pytest.mark.parametrize("model", vh.MODELS)
def test_every_fixture_through_the_optimiser_step(model, dev):
    from sympa_amd import ops
    tally = vh.Tally()
    for dims in rh.dims_of(model):
        for state in rh.STATES:
            fx = rh.radam_fixture(model, dims, state)
            for lr, wd in rh.SETTINGS:
                want = fx[rh.setting_key(lr, wd)]
                p, man = _param(model, dims, fx["x"], dev)
                p.grad = _d(fx["g"], dev)
                opt, st = _optimiser(p, fx, lr, wd, dev)
                opt.step()
                label = f"{model} dims {dims} {state} lr {lr} wd {wd}"
                rh.check_radam(tally, model, dims, want, p.data.cpu().numpy(), st["exp_avg"].cpu().numpy(),
                               st["exp_avg_sq"].cpu().numpy(), label)
                assert man.projected_points == int(want["moved"].sum()), label
                assert opt.param_groups[0]["step"] == fx["t"]
                if lr == 1.0 and state == "later":
                    # the second route to exp_avg: the manifold's transp of m1 along x -> the kernel's new row
                    from sympa_amd.manifolds.vector import torch_egrad2rgrad
                    X, G = _d(fx["x"], dev), _d(fx["g"], dev)
                    m1 = rh.BETAS[0] * _d(fx["m"], dev) + (1 - rh.BETAS[0]) * torch_egrad2rgrad(X, G, model)
                    two = man.transp(X, p.data, m1).cpu().numpy()
                    tol = 2 * rh.radam_bound(model, dims, want["m"], want["km"])
                    assert (np.abs(two - st["exp_avg"].cpu().numpy()).max(1) <= tol).all(), label
    assert ops.check_status(dev) == (0, 0)
    tally.report(f"GPU radam {model}")


def _hand_step(model, x, g, m, s, pows, lr, wd, dev, sentinel=None, counter=None, **kw):
    """One ops.vector_radam_step_ on fresh copies; with `sentinel`, the three tensors are slices [pad, pad + rows) of buffers
    filled with it.  -> (x, m, s, the three whole buffers or None)"""
    from sympa_amd import ops
    n, dims = x.shape
    bufs = None
    if sentinel is None:
        X, M, S = (_d(a, dev).clone() for a in (x, m, s))
    else:
        pad = 3
        bufs = [torch.full((n + 2 * pad, dims), sentinel, dtype=torch.float64, device=dev) for _ in range(3)]
        X, M, S = (b[pad:pad + n] for b in bufs)
        for t, a in ((X, x), (M, m), (S, s)):
            t.copy_(_d(a, dev))
    ops.vector_radam_step_(X, _d(g, dev), M, S, _d(np.asarray(pows, dtype=np.float64), dev), model, lr, rh.BETAS, rh.EPS_ADAM, wd,
                           counter=counter, **kw)
    return X, M, S, bufs


@pytest.mark.parametrize("model,dims,n", [("poincare", 4, 70), ("lorentz", 4, 70), ("sphere", 272, 5), ("prod-hyhy", 272, 5),
                                          ("poincare", 5, 9), ("lorentz", 5, 9), ("prod-hysph", 6, 3), ("prod-hyeu", 6, 3)])
def test_partial_waves_inside_guarded_buffers(model, dims, n, dev):
    """N rows as a slice of larger buffers filled with a sentinel: rows [0, N) are the rows of a 64-row table bit for bit (the
    fixture rows, repeated), and nothing in front of or behind the three tensors is touched."""
    from sympa_amd import ops
    fx = rh.radam_fixture(model, dims, "later")
    rep = [np.tile(fx[k], (5, 1))[:max(n, 64)] for k in ("x", "g", "m", "s")]
    pows = fx["pows_prev"] * np.array(rh.BETAS)
    full = _hand_step(model, *[a[:64] for a in rep], pows, 1.0, 0.0, dev)
    sentinel = -7.25
    X, M, S, bufs = _hand_step(model, *[a[:n] for a in rep], pows, 1.0, 0.0, dev, sentinel=sentinel)
    k = min(n, 64)
    for got, want in zip((X, M, S), full[:3]):
        assert torch.equal(got[:k], want[:k]), (model, dims, n)
    if n > 64:                                   # rows 64.. repeat rows 0..: the same bits again
        for got in (X, M, S):
            assert torch.equal(got[64:n], got[64 - 64:n - 64])
    for b in bufs:
        assert bool((b[:3] == sentinel).all()) and bool((b[3 + n:] == sentinel).all()), (model, dims, n)
    assert ops.check_status(dev) == (0, 0)


@pytest.mark.parametrize("model,dims", [("poincare", 8), ("prod-hysph", 10), ("lorentz", 17), ("euclidean", 5)])
def test_two_optimiser_steps_are_two_kernel_calls(model, dims, dev):
    from sympa_amd.optim import RiemannianAdam
    fx = rh.radam_fixture(model, dims, "first")
    g2 = np.roll(fx["g"], 1, axis=0)
    p, man = _param(model, dims, fx["x"], dev)
    opt = RiemannianAdam([p], lr=0.05, betas=rh.BETAS, eps=rh.EPS_ADAM, weight_decay=0.1)
    for g in (fx["g"], g2):
        p.grad = _d(g, dev)
        opt.step()
    b = np.array(rh.BETAS)
    z = np.zeros_like(fx["x"])
    X, M, S, _ = _hand_step(model, fx["x"], fx["g"], z, z, b, 0.05, 0.1, dev)
    from sympa_amd import ops
    ops.vector_radam_step_(X, _d(g2, dev), M, S, _d(b, dev) * _d(b, dev), model, 0.05, rh.BETAS, rh.EPS_ADAM, 0.1)
    st = opt.state[p]
    assert torch.equal(p.data, X) and torch.equal(st["exp_avg"], M) and torch.equal(st["exp_avg_sq"], S)
    assert opt.param_groups[0]["step"] == 2
    # snapshot / restore and a changed group["betas"], as for the Siegel tables
    snap = opt.snapshot_state()
    before = p.data.clone()
    p.grad = _d(fx["g"], dev)
    opt.step()
    opt.restore_state(snap)
    assert opt.param_groups[0]["step"] == 2 and torch.equal(st["exp_avg"], M) and torch.equal(st["exp_avg_sq"], S)
    assert torch.equal(st["bias_pows"], _d(b * b, dev))
    opt.param_groups[0]["betas"] = (0.8, 0.99)
    p.data.copy_(before)
    opt.step()
    assert np.allclose(st["bias_pows"].cpu().numpy(), np.array([0.8, 0.99]) ** 3, rtol=1e-14, atol=0)


@pytest.mark.parametrize("model,dims", [("poincare", 9), ("prod-hyeu", 16), ("sphere", 33), ("lorentz", 4)])
def test_folded_clip_is_a_step_on_the_scaled_gradient(model, dims, dev):
    fx = rh.radam_fixture(model, dims, "later")
    pows = fx["pows_prev"] * np.array(rh.BETAS)
    G = _d(fx["g"], dev)
    sq = (G * G).sum().reshape(1)
    coef = min(1.0, 0.5 / (float(sq.sqrt()) + 1e-6))
    assert coef < 1.0
    a = _hand_step(model, fx["x"], fx["g"], fx["m"], fx["s"], pows, 0.01, 0.1, dev, clip_sqnorm=sq, max_norm=0.5)
    b = _hand_step(model, fx["x"], fx["g"] * coef, fx["m"], fx["s"], pows, 0.01, 0.1, dev)
    for u, v in zip(a[:3], b[:3]):
        assert float((u - v).abs().max()) <= 8 * vh.EPS64 * float(v.abs().max())


def test_nan_gradient_sets_the_status_bit_and_spares_the_other_rows(dev):
    from sympa_amd import ops
    model, dims = "prod-hysph", 8
    fx = rh.radam_fixture(model, dims, "later")
    pows = fx["pows_prev"] * np.array(rh.BETAS)
    clean = _hand_step(model, fx["x"], fx["g"], fx["m"], fx["s"], pows, 0.01, 0.0, dev)
    assert ops.check_status(dev) == (0, 0)
    g = fx["g"].copy()
    g[5, 6] = np.nan
    dirty = _hand_step(model, fx["x"], g, fx["m"], fx["s"], pows, 0.01, 0.0, dev)
    keep = [r for r in range(16) if r != 5]
    for u, v in zip(dirty[:3], clean[:3]):
        assert torch.equal(u[keep], v[keep])
    st = ops._status_buf(dev).cpu()
    assert int(st[0]) & 2 and int(st[1]) == 1                      # SYMPA_ST_NONFINITE, one row
    with pytest.raises(AssertionError):
        ops.check_status(dev)
    assert ops.check_status(dev) == (0, 0)


@pytest.mark.parametrize("model", vh.MODELS)
def test_fifty_adam_steps_at_lr_1_stay_on_the_manifold(model, dev):
    """Rows 0..15 take 50 RiemannianAdam steps at lr = 1 on sum_i d(x_i, c_i) towards the anchors c_i = rows 16..31 (whose
    gradient is zeroed).  The Riemannian gradient of a distance has length 1, so Adam's normalised step has Riemannian length
    at most about lr = 1 -- in the ball a Euclidean length of (1 - xx) / 2, which cannot carry a row out from a generic point.
    For the models with a Poincare factor the anchors are therefore the `boundary` points of the pair fixtures (at the projx
    norm 1 - 1e-5) and the rows start at their partners: a row reaches its anchor after a dozen steps, overshoots it outwards,
    and projx has to bring it back.  The other models take the `generic` pairs of the RiemannianSGD test."""
    from sympa_amd import ops
    from sympa_amd.manifolds.vector import _factor_slices, _lorentz_sign
    from sympa_amd.optim import RiemannianAdam
    dims = 8
    if "P" in vh.FACTORS[model]:
        fx = vh.pair_fixture(model, dims, "boundary")
        start, anchors = fx["y"], fx["x"]
    else:
        fx = vh.pair_fixture(model, dims, "generic")
        start, anchors = fx["x"], fx["y"]
    m = make_model(model, dims, 32, dev)
    with torch.no_grad():
        m.embeddings.embeds.data = torch.cat((_d(start, dev), _d(anchors, dev))).contiguous()
    opt = RiemannianAdam(m.parameters(), lr=1.0, eps=rh.EPS_ADAM)
    ar = torch.arange(16, device=dev)
    trip = torch.stack((ar, ar + 16), 1).contiguous()
    m.manifold.projected_points = 0
    for _ in range(50):
        opt.zero_grad(set_to_none=False)
        m(trip).sum().backward()
        m.embeddings.embeds.grad[16:].zero_()
        opt.step()
    ok, point, reason = m.check_all_points()
    assert ok, (model, reason, point)
    assert ops.check_status(dev) == (0, 0)
    if model == "poincare":
        assert m.manifold.projected_points > 0
    x, mom = m.embeddings.embeds.data, opt.state[m.embeddings.embeds]["exp_avg"]
    assert bool(torch.isfinite(mom).all())
    for g, s in _factor_slices(model, dims):
        xs, ms = x[:, s], mom[:, s]
        if g in "SL":
            j = _lorentz_sign(xs) if g == "L" else 1.0
            assert float((j * xs * ms).sum(-1).abs().max()) <= 1e-12 * float(ms.abs().max()), (model, g)


@pytest.mark.parametrize("model", vh.MODELS)
def test_training_a_tree_with_adam(model, dev):
    from sympa_amd import ops
    from sympa_amd.graph import GraphDistances
    from sympa_amd.losses import AverageDistortionLoss
    from sympa_amd.optim import RiemannianAdam
    torch.manual_seed(3)
    n = 31
    hops = GraphDistances(*tree_csr(n), device=dev)
    trip = hops.triplets()
    ids, gd = trip[:, :2].contiguous(), trip[:, 2].to(torch.float64)
    m = make_model(model, 4, n, dev)
    opt = RiemannianAdam(m.parameters(), lr=0.05, eps=rh.EPS_ADAM)
    loss_fn = AverageDistortionLoss()
    with torch.no_grad():
        start = float(loss_fn.calculate_loss(gd, m(ids)))
    g = torch.Generator().manual_seed(1)
    for step in range(100):
        sel = torch.randint(0, ids.shape[0], (64,), generator=g).to(dev)
        opt.zero_grad(set_to_none=False)
        m.fused_loss_backward(ids[sel].contiguous(), gd[sel])
        opt.step()
    with torch.no_grad():
        end = float(loss_fn.calculate_loss(gd, m(ids)))
    print(f"[vector] {model} dims 4, 31-node tree, 100 Adam steps: loss {start:.4g} -> {end:.4g}", flush=True)
    assert np.isfinite(end) and end < start, (model, start, end)
    assert m.check_all_points()[0] and ops.check_status(dev) == (0, 0)


def test_the_trainer_runs_a_vector_model_with_radam(dev):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import train_siegel
    args = train_siegel.parser().parse_args(["--graph", "grid3d-125", "--manifold", "poincare", "--optim", "radam", "--dims", "4",
                                             "--epochs", "3", "--batch_size", "2048", "--val_every", "1"])
    model, history = train_siegel.train(args, log=lambda *a: None)
    assert len(history) == 3 and all(np.isfinite(h[1]) and np.isfinite(h[2]) for h in history)
    assert model.check_all_points()[0]
