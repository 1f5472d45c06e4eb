"""GPU: the spd model's differentiable vector-valued distance (C-ABI sympa_spd_vvd_fwd / sympa_spd_model_vvd_forward /
sympa_spd_vvd_bwd / sympa_spd_model_vvd_backward) -- every route against the 70-digit fixtures at every n,
against the library's own distance routes, at the batch and instantiation boundaries, and the Finsler distances built on it.
Every test is one launch (per route) over at most a few hundred pairs.  Bounds and their reasoning: tests/spd_vvd_helpers.py."""
import numpy as np
import pytest
import torch

from tests import spd_vvd_helpers as h
from tests.test_spd_exact import EPS64, check, fwd_errors, fwd_tol, pool, skip_same

pytestmark = pytest.mark.gpu
EDGE_DIMS = (1, 2, 3, 5, 6, 9, 11, 12, 16)       # the instantiation boundaries: one lane / sixteen lanes, the translation units


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def _np(*ts):
    return tuple(t.detach().cpu().numpy() for t in ts)


def _model(table, dev, spd_metric=None):
    from sympa_amd.model import Model

    class A:
        manifold, metric, dims, num_points = "spd", "riem", int(table.shape[1]), int(table.shape[0])
        scale_coef, scale_init, train_scale = 1.0, 1.0, False
    A.spd_metric = spd_metric
    m = Model(A)
    with torch.no_grad():
        m.embeddings.embeds.data = table.detach().cpu().clone()
    return m.to(dev)


def _random_pairs(b, n, seed, dev, spread=0.4):
    g = torch.Generator().manual_seed(seed)
    def pts():
        a = spread * torch.randn(b, n, n, generator=g, dtype=torch.float64)
        p = torch.matrix_exp(0.5 * (a + a.transpose(-1, -2)))
        return (0.5 * (p + p.transpose(-1, -2))).to(dev)
    return pts(), pts()


def _status(dev):
    from sympa_amd import ops
    bits, count = ops._status_buf(dev).tolist()
    ops._status_buf(dev).zero_()
    return bits, count


# ------------------------------------------------------------------------------------------------ against the 70-digit fixtures
@pytest.mark.parametrize("n", h.DIMS)
def test_vvd_bwd_exact(dev, n):
    """sympa_spd_vvd_bwd, flags 0 (n >= 3: spd_vvd_coop_bwd_kernel<n>; n <= 2: the one-lane kernel) and SYMPA_FLAG_GENERIC (the
    one-lane kernel at every n): gradients and vvd_out on every case, both cotangent sets."""
    from sympa_amd import ops
    for flags, coop, name in ((0, n >= 3, "flags0"), (ops.FLAG_GENERIC, False, "generic")):
        def route(x, y, gv):
            return _np(*ops.spd_vvd_backward(_d(x, dev), _d(y, dev), _d(gv, dev), return_vvd=True, flags=flags))
        h.check_route(n, route, f"sympa_spd_vvd_bwd {name} n={n}", coop)
        ops.check_status(dev)


@pytest.mark.parametrize("n", h.DIMS)
def test_model_forward_vvd_autograd_exact(dev, n):
    """Model.forward_vvd + autograd: table rows = x then y, triplets (i, b + i), loss (gv * v).sum() -- sympa_spd_model_vvd_forward
    and the in-kernel scatter of sympa_spd_model_vvd_backward; the forward's v against the fixture as well."""
    from sympa_amd import ops

    def route(x, y, gv):
        b = len(x)
        m = _model(torch.from_numpy(np.concatenate((x, y))), dev)
        trip = torch.stack((torch.arange(b), torch.arange(b) + b), 1).to(dev)
        v = m.forward_vvd(trip)
        (_d(gv, dev) * v).sum().backward()
        g = m.embeddings.embeds.grad.cpu().numpy()
        return g[:b], g[b:], v.detach().cpu().numpy()
    h.check_route(n, route, f"Model.forward_vvd n={n}", n >= 3, v_coop=n >= 6)       # (v comes from the forward kernel here)
    ops.check_status(dev)


@pytest.mark.parametrize("n", h.DIMS)
def test_forward_routes_exact(dev, n):
    """sympa_spd_vvd_fwd with flags 0 (n >= 6: spd_vvd_coop_fwd_kernel<n>, n <= 5 the one-lane kernel) and SYMPA_FLAG_GENERIC, and the
    gathered forward, against the fixture's v; spd_metric(v, "riem") against the exact distance within fwd_tol."""
    from sympa_amd import ops
    from sympa_amd.manifolds.spd import spd_metric
    p = h.vpool(n)
    X, Y = _d(p["x"], dev), _d(p["y"], dev)
    b = len(p["x"])
    trip = torch.stack((torch.arange(b), torch.arange(b) + b), 1).to(dev)
    routes = {"flags0": (ops.spd_vvd_forward(X, Y), n >= 6), "generic": (ops.spd_vvd_forward(X, Y, flags=ops.FLAG_GENERIC), False),
              "model": (ops.spd_model_vvd_forward(torch.cat((X, Y)).contiguous(), trip), n >= 6)}
    ops.check_status(dev)
    assert torch.equal(routes["model"][0], routes["flags0"][0])
    for name, (v, coop) in routes.items():
        h.check_v(p, v.cpu().numpy(), coop, f"sympa_spd_vvd_fwd {name} n={n}")
        check(fwd_errors(pool(n), spd_metric(v, "riem").cpu().numpy()), fwd_tol(pool(n), coop=coop), skip_same(pool(n)),
              f"spd_metric(v, riem) {name} n={n}")


# ------------------------------------------------------------------------------------------------ against the library's own routes
@pytest.mark.parametrize("n", h.DIMS)
def test_consistent_with_the_distance_routes(dev, n):
    """gv = v / ||v||: sympa_spd_vvd_bwd agrees with sympa_spd_backward_rows(grad_out = 1) of the same flags within the sum of the two
    routes' bounds; spd_metric(vvd, "riem") agrees with sympa_spd_dist_fwd within fwd_tol."""
    from sympa_amd import ops
    from sympa_amd.manifolds.spd import spd_metric
    p = h.vpool(n)
    b = len(p["x"])
    X, Y, GV = _d(p["x"], dev), _d(p["y"], dev), _d(h.unit_cotangent(p), dev)
    one = torch.ones(b, dtype=torch.float64, device=dev)
    for flags, coop, built_in in ((0, n >= 3, ops.FLAG_COOP), (ops.FLAG_GENERIC, False, ops.FLAG_GENERIC)):
        rows, _ = ops.spd_backward_rows(X, Y, grad_out=one, want_out=True, flags=built_in)
        gx, gy = ops.spd_vvd_backward(X, Y, GV, flags=flags)
        h.check_against_distance_backward(n, *_np(gx, gy, rows[:b], rows[b:]), coop, f"flags={flags} n={n}")
        fcoop = n >= 6 and flags == 0
        d, v = ops.spd_dist_forward(X, Y, flags=flags), ops.spd_vvd_forward(X, Y, flags=flags)
        err = ((spd_metric(v, "riem") - d).abs() / d.clamp_min(1e-300)).cpu().numpy()
        check(err, fwd_tol(pool(n), coop=fcoop), skip_same(pool(n)), f"riem of vvd against spd_dist_fwd flags={flags} n={n}")
    ops.check_status(dev)


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("n", EDGE_DIMS)
def test_batch_boundaries_and_the_gather(dev, n):
    """b = 1, 3, 4, 5, 63, 64, 65 (four pairs per round, 64 per wave): every prefix of a batch gives the rows of the whole batch bit
    for bit, forward and backward, the scatter writes nothing behind its end, and the gathered forward equals the pre-gathered one
    bit for bit."""
    from sympa_amd import ops
    x, y = _random_pairs(65, n, 40 + n, dev)
    gv = _d(h.cotangent("mixed", 65, n, 11), dev)
    table = torch.cat((x, y)).contiguous()
    trip = torch.stack((torch.arange(65), torch.arange(65) + 65), 1).to(dev)
    v_all = ops.spd_vvd_forward(x, y)
    gx_all, gy_all, vb_all = ops.spd_vvd_backward(x, y, gv, return_vvd=True)
    for b in (1, 3, 4, 5, 63, 64, 65):
        # (a lane of the forward's QL is frozen once its pair has converged: a row depends on its own pair, not on its wave)
        assert torch.equal(ops.spd_vvd_forward(x[:b], y[:b]), v_all[:b])
        assert torch.equal(ops.spd_model_vvd_forward(table, trip[:b]), v_all[:b])
        gx, gy, vb = ops.spd_vvd_backward(x[:b], y[:b], gv[:b], return_vvd=True)
        assert torch.equal(gx, gx_all[:b]) and torch.equal(gy, gy_all[:b]) and torch.equal(vb, vb_all[:b])
        gt, vt = ops.spd_model_vvd_backward(table, trip[:b], gv[:b], return_vvd=True)
        assert torch.equal(vt, vb_all[:b]) and not gt[b:65].any() and not gt[65 + b:].any()
        # every row is used once: the scatter adds each gradient row to zero
        assert torch.equal(gt[:b], gx_all[:b]) and torch.equal(gt[65:65 + b], gy_all[:b])
    # a strided [b, 3] triplet list reads the same pairs
    t3 = torch.cat((trip, torch.ones(65, 1, dtype=torch.int64, device=dev)), 1)
    assert torch.equal(ops.spd_model_vvd_forward(table, t3), v_all)
    ops.check_status(dev)


@pytest.mark.parametrize("n", EDGE_DIMS)
def test_scatter_against_index_add(dev, n):
    """200 pairs over 7 rows: the accumulated table gradient against an fp64 index_add of the dense rows, within
    200 eps64 sum |terms| per element (the order of the atomic adds is free)."""
    from sympa_amd import ops
    tab, _ = _random_pairs(7, n, 60 + n, dev)
    g = torch.Generator().manual_seed(n)
    trip = torch.stack((torch.randint(0, 7, (200,), generator=g), torch.randint(0, 7, (200,), generator=g)), 1).to(dev)
    gv = _d(h.cotangent("mixed", 200, n, 13), dev)
    gt, v = ops.spd_model_vvd_backward(tab, trip, gv, return_vvd=True)
    gx, gy, v2 = ops.spd_vvd_backward(tab[trip[:, 0]], tab[trip[:, 1]], gv, return_vvd=True)
    ops.check_status(dev)
    assert torch.equal(v, v2)
    idx = torch.cat((trip[:, 0], trip[:, 1]))
    terms = torch.cat((gx, gy))
    want = torch.zeros_like(tab).index_add_(0, idx, terms)
    mag = torch.zeros_like(tab).index_add_(0, idx, terms.abs())
    assert bool(((gt - want).abs() <= 200 * EPS64 * mag).all())
    # accumulation into a given gradient
    gt2 = ops.spd_model_vvd_backward(tab, trip, gv, grad_table=gt.clone())
    assert bool(((gt2 - 2 * want).abs() <= 400 * EPS64 * mag).all())


@pytest.mark.parametrize("n", EDGE_DIMS)
def test_exact_zeros_bad_index_not_pd_and_ties(dev, n):
    from sympa_amd import ops
    b = 9
    x, y = _random_pairs(b, n, 80 + n, dev)
    gv = _d(h.cotangent("mixed", b, n, 17), dev)
    table = torch.cat((x, y)).contiguous()
    trip = torch.stack((torch.arange(b), torch.arange(b) + b), 1).to(dev)
    # x == y: v = 0 and exact zero gradients whatever the cotangent; a zero cotangent: exact zero gradients
    for flags in (0, ops.FLAG_GENERIC):
        gx, gy, v = ops.spd_vvd_backward(x, x, gv, return_vvd=True, flags=flags)
        assert not gx.any() and not gy.any() and not v.any()
        assert not ops.spd_vvd_forward(x, x, flags=flags).any()
        gx, gy = ops.spd_vvd_backward(x, y, torch.zeros_like(gv), flags=flags)
        assert not gx.any() and not gy.any()
    assert not ops.spd_model_vvd_backward(table, torch.stack((trip[:, 0], trip[:, 0]), 1).contiguous(), gv).any()
    # an exact tie with a constant cotangent is finite and equals c d log det
    for flags in (0, ops.FLAG_GENERIC):
        c = torch.full((b, n), 0.75, dtype=torch.float64, device=dev)
        gx, gy, v = ops.spd_vvd_backward(x, 2.0 * x, c, return_vvd=True, flags=flags)
        assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gy).all())
        torch.testing.assert_close(v, torch.full_like(v, float(np.log(2.0))), rtol=1e-13, atol=0)
        xi = torch.linalg.inv(x)
        torch.testing.assert_close(gx, -0.75 * xi, rtol=1e-9, atol=1e-12)
        torch.testing.assert_close(gy, 0.375 * xi, rtol=1e-9, atol=1e-12)
    ops.check_status(dev)
    # one bad index: SYMPA_ST_BAD_INDEX, a NaN row, no contribution; every other pair bit for bit
    good, v_good = ops.spd_model_vvd_backward(table, trip, gv, return_vvd=True)
    f_good = ops.spd_model_vvd_forward(table, trip)
    ops.check_status(dev)
    bad, rest = 4, torch.arange(b, device=dev) != 4
    for value in (2 * b, -1):
        t = trip.clone()
        t[bad, 1] = value
        for flags in (0, ops.FLAG_GENERIC):
            f = ops.spd_model_vvd_forward(table, t, flags=flags)
            bits, count = _status(dev)
            assert bits & ops.ST_BAD_INDEX and count == 1
            assert f[bad].isnan().all() and (flags or torch.equal(f[rest], f_good[rest]))
            gt, v = ops.spd_model_vvd_backward(table, t, gv, return_vvd=True, flags=flags)
            bits, count = _status(dev)
            assert bits & ops.ST_BAD_INDEX and count == 1
            assert v[bad].isnan().all() and not gt[bad].any() and not gt[b + bad].any() and bool(torch.isfinite(gt).all())
            if not flags:
                assert torch.equal(v[rest], v_good[rest]) and torch.equal(gt[:b][rest], good[:b][rest]) \
                    and torch.equal(gt[b:][rest], good[b:][rest])
    # a point that is not positive definite
    xb = x.clone()
    xb[2] = -xb[2]
    for flags in (0, ops.FLAG_GENERIC):
        ops.spd_vvd_forward(xb, y, flags=flags)
        assert _status(dev)[0] & ops.ST_NOT_PD
        ops.spd_vvd_backward(xb, y, gv, flags=flags)
        assert _status(dev)[0] & ops.ST_NOT_PD


# ------------------------------------------------------------------------------------------------ Finsler
@pytest.mark.parametrize("n", (2, 5, 8, 16))
def test_finsler_distances(dev, n):
    """SymmetricPositiveDefinite(finsler=...).dist against sum |log lam| and max |log lam| of the fixture (the v bound, summed / at the
    largest component); Model.forward with spd_metric = "fone" follows it; riem / None stay on the distance kernel."""
    from sympa_amd import ops
    from sympa_amd.manifolds import SymmetricPositiveDefinite
    p = h.vpool(n)
    X, Y = _d(p["x"], dev), _d(p["y"], dev)
    coop = n >= 6
    tol = h.v_tol(p, coop)
    want = {"fone": np.abs(p["v"]).sum(1), "finf": np.abs(p["v"]).max(1)}
    bound = {"fone": tol.sum(1), "finf": tol.max(1)}
    for kind in ("fone", "finf"):
        got = SymmetricPositiveDefinite(finsler=kind).dist(X, Y).cpu().numpy()
        assert (np.abs(got - want[kind]) <= bound[kind]).all(), kind
        assert got[p["same"]] == 0.0
    assert torch.equal(SymmetricPositiveDefinite(finsler="riem").dist(X, Y), SymmetricPositiveDefinite().dist(X, Y))
    assert torch.equal(SymmetricPositiveDefinite().dist(X, Y), ops.spd_dist_forward(X, Y))
    b = len(p["x"])
    trip = torch.stack((torch.arange(b), torch.arange(b) + b), 1).to(dev)
    m = _model(torch.cat((X, Y)), dev, "fone")
    with torch.no_grad():
        out = m(trip).cpu().numpy()
    assert (np.abs(out - want["fone"]) <= bound["fone"]).all()
    ops.check_status(dev)


def test_finsler_model_differentiates_and_the_graphed_step_refuses(dev):
    from sympa_amd import ops
    from sympa_amd.optim import RiemannianSGD
    from sympa_amd.train_step import GraphedTrainStep
    x, _ = _random_pairs(12, 3, 5, dev)
    m = _model(x, dev, "finf")
    trip = torch.stack((torch.arange(6), torch.arange(6) + 6), 1).to(dev)
    d = m(trip)
    d.sum().backward()
    g = m.embeddings.embeds.grad
    assert bool(torch.isfinite(g).all()) and bool(g.abs().sum() > 0)
    # finf weights one component per pair: the gradient is that of sympa_spd_vvd_bwd under the one-hot cotangent autograd built
    v = ops.spd_vvd_forward(x[:6], x[6:])
    hot = torch.zeros_like(v)
    k = v.abs().argmax(1)
    hot[torch.arange(6), k] = torch.sign(v[torch.arange(6), k])
    gx, gy = ops.spd_vvd_backward(x[:6], x[6:], hot)
    assert torch.equal(g[:6], gx) and torch.equal(g[6:], gy)
    opt = RiemannianSGD(m.parameters(), lr=1e-2, weight_decay=0.0, stabilize=None)
    with pytest.raises(NotImplementedError, match="GraphedTrainStep"):
        GraphedTrainStep(m, opt, 6, 50.0, dev)
    with pytest.raises(NotImplementedError, match="finf"):
        m.forward_batches([trip])
    ops.check_status(dev)


def test_fone_training_lowers_the_distortion_loss(dev):
    """30 classic-loop RiemannianSGD steps on a 16-node tree with the fone distance at n = 3."""
    import networkx as nx
    from sympa_amd import data, ops
    from sympa_amd.losses import AverageDistortionLoss
    from sympa_amd.model import Model
    from sympa_amd.optim import RiemannianSGD
    torch.manual_seed(3)
    trip, id2node = data.graph_triplets(nx.full_rary_tree(2, 16))
    assert len(id2node) == 16

    class A:
        manifold, metric, dims, num_points, spd_metric = "spd", "riem", 3, 16, "fone"
        scale_coef, scale_init, train_scale = 1.0, 1.0, False
    m = Model(A).to(dev)
    opt = RiemannianSGD(m.parameters(), lr=2e-2, weight_decay=0.0, stabilize=None)
    ids = trip[:, :2].to(torch.int64).contiguous().to(dev)
    gd = trip[:, 2].to(torch.float64).to(dev)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=False)
        loss = AverageDistortionLoss().calculate_loss(gd, m(ids))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 50.0)
        opt.step()
        losses.append(float(loss.detach()))
    ops.check_status(dev)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
