"""GPU: the differentiable vector-valued distance -- C-ABI sympa_model_vvd_forward / sympa_siegel_vvd_bwd / sympa_model_vvd_backward,
the autograd functions, SiegelManifold.vvd and Model.forward_vvd -- against the 50-digit directional derivatives of the sorted v
(bounds and method: tests/vvd_helpers.py) and against the library's own routes."""
import numpy as np
import pytest
import torch

from oracle import siegel_oracle as so
from tests import dual_helpers as dh
from tests import vvd_helpers as vh
from tests.helpers import METRICS, points

pytestmark = pytest.mark.gpu
EPS64 = vh.EPS64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _points(model, b, n, seed, s=0.3):
    if model == "dual":
        return dh.sym_points(b, n, s, seed)
    return points(model, b, n, s, torch.Generator().manual_seed(seed))


def _model(model, metric, n, table, dev, train_scale=False, scale_init=1.0):
    from sympa_amd.model import Model

    class A:
        pass
    A.manifold, A.metric, A.dims, A.num_points = model, metric, n, table.shape[0]
    A.scale_coef, A.scale_init, A.train_scale = 1.0, scale_init, train_scale
    m = Model(A)
    with torch.no_grad():
        m.embeddings.embeds.data = table.clone()
    return m.to(dev)


# ------------------------------------------------------------------------------------------------ the 50-digit fixtures
@pytest.mark.parametrize("n", vh.DIMS)
@pytest.mark.parametrize("model", vh.MODELS)
def test_pregathered_backward_exact(dev, model, n):
    """sympa_siegel_vvd_bwd: every case, both cotangent sets; the v it returns against the exact v."""
    from sympa_amd import ops

    def route(z1, z2, gv):
        g1, g2, v = ops.siegel_vvd_backward(_d(z1, dev), _d(z2, dev), _d(gv, dev), model, return_vvd=True)
        return g1.cpu().numpy(), g2.cpu().numpy(), v.cpu().numpy()
    vh.check_route(model, n, route, "sympa_siegel_vvd_bwd")
    ops.check_status(dev)


@pytest.mark.parametrize("n", vh.DIMS)
@pytest.mark.parametrize("model", vh.MODELS)
def test_table_route_exact(dev, model, n):
    """Model.forward_vvd + autograd: the table rows are the fixture's z1 then z2, triplets (i, b + i), loss (gv * v).sum(); every row is
    touched once, so the atomics do not enter the bound."""
    from sympa_amd import ops

    def route(z1, z2, gv):
        b = len(z1)
        m = _model(model, "riem", n, torch.from_numpy(np.concatenate((z1, z2))), dev)
        trip = torch.stack((torch.arange(b), torch.arange(b) + b), 1).to(dev)
        v = m.forward_vvd(trip)
        (_d(gv, dev) * v).sum().backward()
        g = m.embeddings.embeds.grad.cpu().numpy()
        return g[:b], g[b:], v.detach().cpu().numpy()
    vh.check_route(model, n, route, "Model.forward_vvd")
    ops.check_status(dev)


# ------------------------------------------------------------------------------------------------ against the library's own routes
@pytest.mark.parametrize("n", (1, 4, 6, 8, 9, 16))
@pytest.mark.parametrize("model", vh.MODELS)
def test_gathered_forward_equals_the_pregathered_forward_bit_for_bit(dev, model, n):
    from sympa_amd import ops
    rows, b = 37, 200
    table = _points(model, rows, n, 3).to(dev)
    g = torch.Generator().manual_seed(n)
    trip = torch.stack((torch.randint(0, rows, (b,), generator=g), torch.randint(0, rows, (b,), generator=g),
                        torch.randint(1, 9, (b,), generator=g)), 1).to(dev)
    got = ops.model_vvd_forward(table, trip, model)
    _, want = ops.siegel_dist_forward(table[trip[:, 0]], table[trip[:, 1]], model, "riem", return_vvd=True)
    ops.check_status(dev)
    assert got.shape == (b, n) and torch.equal(got, want)
    # a [b, 2] list, and SiegelManifold.vvd: the same values, bit for bit, with and without a graph
    assert torch.equal(ops.model_vvd_forward(table, trip[:, :2].contiguous(), model), want)
    man = _model(model, "riem", n, table.cpu(), dev).manifold
    z1 = table[trip[:, 0]].clone().requires_grad_(True)
    assert torch.equal(man.vvd(table[trip[:, 0]], table[trip[:, 1]]), want)
    v = man.vvd(z1, table[trip[:, 1]])
    assert v.requires_grad and torch.equal(v.detach(), want)


@pytest.mark.parametrize("n", (2, 6, 7, 16))
@pytest.mark.parametrize("model", vh.MODELS)
def test_scatter_against_dense(dev, model, n):
    """7 rows, 200 pairs with repeated ids and some src == dst: sympa_model_vvd_backward against an fp64 index_add of the dense rows of
    sympa_siegel_vvd_bwd, within the summation-order bound 200 eps64 sum |terms| per element."""
    from sympa_amd import ops
    rows, b = 7, 200
    table = _points(model, rows, n, 5).to(dev)
    g = torch.Generator().manual_seed(n)
    src, dst = torch.randint(0, rows, (b,), generator=g), torch.randint(0, rows, (b,), generator=g)
    dst[::17] = src[::17]
    trip = torch.stack((src, dst), 1).to(dev)
    gv = _d(vh.cotangent("mixed", b, n, 9), dev)
    gt, v = ops.model_vvd_backward(table, trip, gv, model, return_vvd=True)
    g1, g2, v2 = ops.siegel_vvd_backward(table[trip[:, 0]], table[trip[:, 1]], gv, model, return_vvd=True)
    ops.check_status(dev)
    assert torch.equal(v, v2)
    idx = torch.cat((trip[:, 0], trip[:, 1]))
    terms = torch.cat((g1, g2))
    want = torch.zeros_like(table).index_add_(0, idx, terms)
    bound = 200 * EPS64 * torch.zeros_like(table).index_add_(0, idx, terms.abs())
    assert ((gt - want).abs() <= bound).all(), float(((gt - want).abs() - bound).max())
    assert (want.abs().amax((1, 2, 3)) > 0).all()
    # an accumulating call adds on top
    gt2 = ops.model_vvd_backward(table, trip, gv, model, grad_table=gt.clone())
    assert ((gt2 - 2 * want).abs() <= 2 * bound).all()


@pytest.mark.parametrize("n", (1, 3, 4, 6, 7, 12))
@pytest.mark.parametrize("model", vh.MODELS)
def test_equal_points_and_zero_cotangent_give_exact_zeros(dev, model, n):
    from sympa_amd import ops
    b = 70
    z1, z2 = _points(model, b, n, 7).to(dev), _points(model, b, n, 8).to(dev)
    gv = _d(vh.cotangent("mixed", b, n, 1), dev)
    g1, g2, v = ops.siegel_vvd_backward(z1, z1.clone(), gv, model, return_vvd=True)
    assert not g1.any() and not g2.any() and not v.any()
    g1, g2 = ops.siegel_vvd_backward(z1, z2, torch.zeros_like(gv), model)
    assert not g1.any() and not g2.any()
    table = torch.cat((z1, z2))
    trip = torch.stack((torch.arange(b), torch.arange(b)), 1).to(dev)        # src == dst through the table
    gt, v = ops.model_vvd_backward(table, trip, gv, model, return_vvd=True)
    assert not gt.any() and not v.any()
    assert not ops.model_vvd_forward(table, trip, model).any()
    ops.check_status(dev)


@pytest.mark.parametrize("n", (2, 5, 7, 10))
@pytest.mark.parametrize("model", vh.MODELS)
def test_one_bad_index(dev, model, n):
    """the status bit, a NaN row, nothing added for that pair, every other pair unchanged bit for bit"""
    from sympa_amd import ops
    rows, b, bad = 9, 130, 77
    table = _points(model, rows, n, 2).to(dev)
    trip = torch.stack((torch.arange(b) % rows, (torch.arange(b) * 5 + 1) % rows), 1).to(dev)
    gv = _d(vh.cotangent("positive", b, n, 4), dev)
    rest = torch.arange(b, device=dev) != bad
    # a table of 2 b rows, each touched once: no accumulation order, the same call with good indices is the reference for "bit for bit"
    big = torch.cat((table[trip[:, 0]], table[trip[:, 1]]))
    tt_good = torch.stack((torch.arange(b), torch.arange(b) + b), 1).to(dev)
    good, v_good = ops.model_vvd_backward(big, tt_good, gv, model, return_vvd=True)
    g1, g2 = good[:b], good[b:]
    fwd_good = ops.model_vvd_forward(table, trip, model)
    ops.check_status(dev)
    for value in (rows, -1):
        t = trip.clone()
        t[bad, 1] = value
        fwd = ops.model_vvd_forward(table, t, model)
        with pytest.raises(IndexError):
            ops.check_status(dev)
        assert fwd[bad].isnan().all() and torch.equal(fwd[rest], fwd_good[rest])
        tt = tt_good.clone()
        tt[bad, 1] = 2 * b if value > 0 else -1
        gt, v = ops.model_vvd_backward(big, tt, gv, model, return_vvd=True)
        bits, count = ops._status_buf(dev).tolist()
        assert bits & ops.ST_BAD_INDEX and count == 1
        with pytest.raises(IndexError):
            ops.check_status(dev)
        assert v[bad].isnan().all() and torch.equal(v[rest], v_good[rest])
        assert not gt[bad].any() and not gt[b + bad].any()
        assert torch.equal(gt[:b][rest], g1[rest]) and torch.equal(gt[b:][rest], g2[rest])


def test_a_point_outside_the_manifold_raises_not_pd(dev):
    from sympa_amd import ops
    for n in (3, 7):
        z1, z2 = _points("upper", 5, n, 1).to(dev), _points("upper", 5, n, 2).to(dev)
        z2[3, 1] = -z2[3, 1]                     # Im Z negative definite
        gv = torch.ones(5, n, dtype=torch.float64, device=dev)
        ops.siegel_vvd_backward(z1, z2, gv, "upper")
        bits, _ = ops._status_buf(dev).tolist()
        assert bits & ops.ST_NOT_PD
        with pytest.raises(AssertionError):
            ops.check_status(dev)


@pytest.mark.parametrize("b", (1, 63, 64, 65))
def test_wave_edges(dev, b):
    """dense and scatter forms of an unrolled (n = 3) and a rolled (n = 7) kernel: b pairs of a longer batch are its first b rows."""
    from sympa_amd import ops
    for model, n in (("upper", 3), ("bounded", 7), ("dual", 4)):
        z1, z2 = _points(model, 65, n, 3).to(dev), _points(model, 65, n, 4).to(dev)
        gv = _d(vh.cotangent("mixed", 65, n, 2), dev)
        G1, G2, V = ops.siegel_vvd_backward(z1, z2, gv, model, return_vvd=True)
        g1, g2, v = ops.siegel_vvd_backward(z1[:b], z2[:b], gv[:b], model, return_vvd=True)
        assert torch.equal(g1, G1[:b]) and torch.equal(g2, G2[:b]) and torch.equal(v, V[:b])
        table = torch.cat((z1, z2))
        trip = torch.stack((torch.arange(65), torch.arange(65) + 65), 1).to(dev)
        GT = ops.model_vvd_backward(table, trip, gv, model)
        gt = ops.model_vvd_backward(table, trip[:b], gv[:b], model)
        assert torch.equal(gt[:b], GT[:b]) and torch.equal(gt[65:65 + b], GT[65:65 + b])
        assert not gt[b:65].any() and not gt[65 + b:].any()
        assert torch.equal(ops.model_vvd_forward(table, trip[:b], model),
                           ops.siegel_dist_forward(z1[:b], z2[:b], model, "riem", return_vvd=True)[1])
    ops.check_status(dev)


@pytest.mark.parametrize("n", (2, 4, 6, 9))
@pytest.mark.parametrize("model", vh.MODELS)
def test_builtin_metrics_are_functions_of_forward_vvd(dev, model, n):
    """compute_metric(model.forward_vvd(t)) = model.forward(t) to 4 n eps64 sum_i |w_i v_i| (w = d metric / d v: the n-term sum and
    riem's square root); the rank metrics only where the relevant relative gap is >= GAP_ZERO."""
    from sympa_amd import ops
    rows, b = 41, 300
    table = _points(model, rows, n, 6)
    g = torch.Generator().manual_seed(10 + n)
    trip = torch.stack((torch.randint(0, rows, (b,), generator=g), torch.randint(0, rows, (b,), generator=g)), 1).to(dev)
    for metric in METRICS:
        m = _model(model, metric, n, table, dev, scale_init=2.0)        # (a power of two: the scale adds no rounding of its own)
        w = None
        if metric == "wsum":
            with torch.no_grad():
                m.manifold.metric.weights.data = torch.linspace(0.2, 1.5, n, dtype=torch.float64, device=dev).reshape(
                    m.manifold.metric.weights.shape)
            w = m.manifold.metric.weights.detach().cpu().reshape(-1)
        with torch.no_grad():
            want = m(trip).cpu()
            v = m.forward_vvd(trip).cpu()
        ops.check_status(dev)
        vv = v.clone().requires_grad_(True)
        got = so.compute_metric(vv, metric, w)
        (gw,) = torch.autograd.grad(got.sum(), vv)
        bound = 4 * n * EPS64 * (gw * v).abs().sum(1)
        ok = torch.ones(b, dtype=torch.bool)
        if n > 1 and metric in ("finf", "fmin", "wsum"):
            rg = (v[:, 1:] - v[:, :-1]) / v[:, 1:].clamp_min(1e-300)
            gap = rg[:, -1] if metric == "finf" else rg.min(1).values
            ok = gap >= vh.GAP_ZERO
        err = (got.detach() - want).abs()
        worst = float((err / bound.clamp_min(1e-300))[ok].max()) if ok.any() else 0.0
        print(f"[vvd] {model} n={n} {metric}: worst {worst:.3g} of the bound, {int((~ok).sum())} pairs skipped", flush=True)
        assert (err <= bound)[ok].all(), (model, n, metric, worst)


def test_forward_vvd_scale_gradient_comes_from_autograd(dev):
    from sympa_amd import ops
    n, rows, b = 3, 11, 50
    m = _model("upper", "riem", n, _points("upper", rows, n, 1), dev, train_scale=True, scale_init=2.0)
    trip = torch.stack((torch.arange(b) % rows, (torch.arange(b) * 3 + 1) % rows), 1).to(dev)
    v = m.forward_vvd(trip)
    v.sum().backward()
    raw = ops.model_vvd_forward(m.embeddings.embeds.data, trip, "upper")
    assert torch.allclose(m.scale.grad.reshape(()), raw.sum(), rtol=1e-13)
    assert torch.equal(v.detach(), raw * 2.0) and m.embeddings.embeds.grad is not None


@pytest.mark.parametrize("model,n", (("upper", 2), ("bounded", 3)))
def test_training_on_an_l3_norm_of_v_lowers_the_distortion(dev, model, n):
    """a 16-node tree, the classic loop (zero_grad, loss, backward, step) of RiemannianSGD, distance = l3 norm of forward_vvd"""
    import networkx as nx
    from sympa_amd import data, ops
    from sympa_amd.optim import RiemannianSGD
    tree = nx.balanced_tree(2, 3)
    tree.add_edge(14, 15)
    trip, _ = data.graph_triplets(tree)
    assert int(trip[:, :2].max()) + 1 == 16
    torch.manual_seed(0)
    m = _model(model, "riem", n, _points(model, 16, n, 12, s=0.1), dev)
    opt = RiemannianSGD(m.parameters(), lr=0.02)
    t, gd = trip.to(dev), trip[:, 2].to(torch.float64).to(dev)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        d = m.forward_vvd(t).pow(3).sum(-1).pow(1.0 / 3.0)
        loss = ((d / gd) ** 2 - 1).abs().mean()              # AverageDistortionLoss (losses.py:10-19)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    ops.check_status(dev)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
