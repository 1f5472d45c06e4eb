"""The vector models on the MI355X (csrc/vector_models.hip): every fixture of tools/make_golden_vector_exact.py through the three
forward entries (bit-equal to each other) and the backward, within the bounds of tests/vector_helpers.py; batches that do not
fill their last wave, prefixes, index strides; the distance matrix; autograd, the fused loss and the deterministic route; the
row operations and RiemannianSGD; training end to end; the status word."""
import numpy as np
import pytest
import torch

from tests import vector_helpers as vh

pytestmark = pytest.mark.gpu
N = 37


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def make_model(model, dims, n, dev, train_scale=False, scale_init=1.0):
    from sympa_amd.model import Model

    class A:
        manifold, metric, num_points = model, "riem", n
        scale_coef = 1.0
    A.dims, A.train_scale, A.scale_init = dims, train_scale, scale_init
    return Model(A).to(dev)


def generic_table(model, dims, n, seed):
    """n points on the manifold, distances O(1): the generator's `generic` recipe restated with numpy."""
    rng = np.random.default_rng(seed)
    f = vh.FACTORS[model]
    m = dims // len(f)
    t = np.zeros((n, dims))
    for k, g in enumerate(f):
        v = rng.standard_normal((n, m))
        u = v / np.linalg.norm(v, axis=1, keepdims=True)
        if g == "E":
            u = v / np.sqrt(m)
        elif g == "P":
            u = u * rng.uniform(0.1, 0.9, (n, 1)) if m > 1 else np.sign(v) * rng.uniform(0.1, 0.9, (n, 1))
        elif g == "L":
            u[:, 1:] = v[:, 1:] / np.linalg.norm(v[:, 1:], axis=1, keepdims=True) * rng.uniform(0.3, 1.5, (n, 1))
            u[:, 0] = np.sqrt(1.0 + (u[:, 1:] ** 2).sum(1))
        t[:, k * m:(k + 1) * m] = u
    return t


def pair_sums(model, x, y):
    """[pairs, factors, (xx, yy, dd, sum |terms|)] in numpy, for the kappa of pairs that are not fixtures"""
    f = vh.FACTORS[model]
    m = x.shape[1] // len(f)
    out = np.zeros((x.shape[0], len(f), 4))
    for k, g in enumerate(f):
        xs, ys = x[:, k * m:(k + 1) * m], y[:, k * m:(k + 1) * m]
        t = (xs - ys) ** 2
        j = np.ones(m)
        if g == "L":
            j[0] = -1.0
        out[:, k] = np.stack(((xs * xs).sum(1), (ys * ys).sum(1), (j * t).sum(1), t.sum(1)), 1)
    return out


def host_dist(model, x, y):
    from sympa_amd.manifolds import vector as mv
    return mv.torch_dist(torch.from_numpy(x), torch.from_numpy(y), model).numpy()


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("model", vh.MODELS)
def test_every_fixture_through_the_three_forward_routes(model, dev):
    from sympa_amd import ops
    tally = vh.Tally()
    for dims in vh.dims_of(model):
        for case in vh.CASES:
            fx = vh.pair_fixture(model, dims, case)
            b = fx["x"].shape[0]
            X, Y = _d(fx["x"], dev), _d(fx["y"], dev)
            single = ops.vector_dist_forward(X, Y, model)
            table = torch.cat((X, Y)).contiguous()
            ar = torch.arange(b, device=dev)
            trip = torch.stack((ar, ar + b), 1).contiguous()
            listed = ops.vector_model_forward(table, trip, model)
            mat = ops.vector_all_pairs_dist(table, model)
            label = f"{model} dims {dims} {case}"
            assert torch.equal(single, listed), label
            assert torch.equal(single, mat[ar, ar + b]), label
            assert torch.equal(mat, mat.T) and bool((mat.diagonal() == 0).all()), label
            vh.check_forward(tally, model, dims, case, fx, single.cpu().numpy(), label)
    assert ops.check_status(dev) == (0, 0)
    tally.report(f"GPU forward {model}")


@pytest.mark.parametrize("model,dims", [("euclidean", 1), ("poincare", 1), ("poincare", 5), ("lorentz", 5), ("sphere", 17),
                                        ("euclidean", 17), ("poincare", 65), ("lorentz", 65), ("sphere", 272), ("poincare", 272),
                                        ("prod-hysph", 272), ("prod-hyeu", 16)])
def test_batches_that_do_not_fill_a_wave_and_their_prefixes(model, dims, dev):
    """b in {1, 63, 64, 65, 257}: every batch is the prefix of the longest one, and equals the host formulas."""
    from sympa_amd import ops
    table = generic_table(model, dims, N, 100 + dims)
    rng = np.random.default_rng(dims)
    trip = rng.integers(0, N, (257, 2))
    T, TR = _d(table, dev), _d(trip, dev)
    full = ops.vector_model_forward(T, TR, model)
    want = host_dist(model, table[trip[:, 0]], table[trip[:, 1]])
    tol, _ = vh.fwd_bound(model, dims, {"sums": pair_sums(model, table[trip[:, 0]], table[trip[:, 1]]), "dist": want})
    got = full.cpu().numpy()
    same = trip[:, 0] == trip[:, 1]
    assert (got[same] == 0).all()
    assert (np.abs(got - want) <= 2 * tol + 4 * vh.EPS64 * want).all()         # (the host formulas carry a bound of their own)
    for b in (1, 63, 64, 65, 257):
        out = ops.vector_model_forward(T, TR[:b].contiguous(), model)
        assert torch.equal(out, full[:b]), (model, dims, b)
        # the same pairs as rows, and backward rows of the prefix
        xs, ys = T[TR[:b, 0]].contiguous(), T[TR[:b, 1]].contiguous()
        assert torch.equal(ops.vector_dist_forward(xs, ys, model), full[:b])
        go = torch.ones(b, dtype=torch.float64, device=dev)
        rows_full, out_b = ops.vector_backward_rows(T, T, model, TR[:b].contiguous(), grad_out=go, want_out=True)
        assert torch.equal(out_b, full[:b])
        if b > 1:
            rows_pref, _ = ops.vector_backward_rows(T, T, model, TR[:b - 1].contiguous(), grad_out=go[:b - 1])
            assert torch.equal(rows_pref[:b - 1], rows_full[:b - 1]) and torch.equal(rows_pref[b - 1:], rows_full[b:2 * b - 1])
        assert bool(torch.isfinite(rows_full).all())
    assert ops.check_status(dev) == (0, 0)


@pytest.mark.parametrize("model,dims", [("poincare", 5), ("lorentz", 17), ("prod-sphsph", 16)])
def test_non_contiguous_index_stride(model, dims, dev):
    from sympa_amd import ops
    T = _d(generic_table(model, dims, N, 7), dev)
    trip3 = torch.randint(0, N, (130, 3), device=dev)
    a = ops.vector_model_forward(T, trip3, model)                           # [b, 3] triplets: stride 3
    b = ops.vector_model_forward(T, trip3[:, :2].contiguous(), model)
    c = ops.vector_model_forward(T, trip3[::2], model)                      # stride 6
    assert torch.equal(a, b) and torch.equal(c, a[::2])
    go = torch.full((130,), 0.5, dtype=torch.float64, device=dev)
    r3, _ = ops.vector_backward_rows(T, T, model, trip3, grad_out=go)
    r2, _ = ops.vector_backward_rows(T, T, model, trip3[:, :2].contiguous(), grad_out=go)
    assert torch.equal(r3, r2)


@pytest.mark.parametrize("model,dims", [("euclidean", 1), ("poincare", 5), ("lorentz", 17), ("sphere", 65), ("prod-hysph", 272)])
def test_distance_matrix_in_row_blocks(model, dims, dev):
    m = make_model(model, dims, N, dev, scale_init=1.7)
    with torch.no_grad():
        m.embeddings.embeds.data = _d(generic_table(model, dims, N, 11), dev)
        whole = m.distance_matrix()
        blocks = torch.cat([m.distance_matrix(b, min(5, N - b)) for b in range(0, N, 5)])
    assert whole.shape == (N, N) and torch.equal(whole, blocks)
    assert bool((whole.diagonal() == 0).all()) and torch.equal(whole, whole.T)
    table = m.embeddings.embeds.data.cpu().numpy()
    i, j = np.divmod(np.arange(N * N), N)
    want = 1.7 * host_dist(model, table[i], table[j]).reshape(N, N)
    assert np.allclose(whole.cpu().numpy(), want, rtol=1e-11, atol=1e-14)


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("model", vh.MODELS)
def test_backward_rows_match_the_fixtures(model, dev):
    from sympa_amd import ops
    tally = vh.Tally()
    for dims in vh.dims_of(model):
        for case in vh.CASES:
            fx = vh.pair_fixture(model, dims, case)
            b = fx["x"].shape[0]
            go = vh.go_of(b, 3 * dims + 2)
            rows, out = ops.vector_backward_rows(_d(fx["x"], dev), _d(fx["y"], dev), model, grad_out=_d(go, dev), want_out=True)
            label = f"{model} dims {dims} {case}"
            vh.check_forward(tally, model, dims, case, fx, out.cpu().numpy(), label)
            rows = rows.cpu().numpy()
            vh.check_backward(tally, model, dims, case, fx, go, rows[:b], rows[b:], label)
    assert ops.check_status(dev) == (0, 0)
    tally.report(f"GPU backward {model}")


def accumulation_bound(model, dims, table, trip, exact_rows, kappa):
    """per table row: (m + C_BWD_EXTRA + 2b) eps kappa^2 sum of the ||.||_inf of the rows added into it (2b: their order is free)"""
    b = trip.shape[0]
    idx = np.concatenate((trip[:, 0], trip[:, 1]))
    acc = np.zeros(table.shape[0])
    np.add.at(acc, idx, np.abs(exact_rows).max(1))
    m = dims // len(vh.FACTORS[model])
    return (m + vh.C_BWD_EXTRA + 2 * b) * vh.EPS64 * kappa * kappa * acc


@pytest.mark.parametrize("model,dims", [("euclidean", 5), ("poincare", 17), ("lorentz", 8), ("sphere", 65), ("prod-hysph", 16),
                                        ("prod-hyhy", 272), ("prod-hyeu", 4), ("prod-sphsph", 8)])
def test_autograd_fused_loss_and_the_deterministic_route(model, dims, dev):
    from sympa_amd import ops
    from sympa_amd.losses import AverageDistortionLoss
    from sympa_amd.manifolds import vector as mv
    b = 65
    m = make_model(model, dims, N, dev, train_scale=True, scale_init=1.3)
    table = generic_table(model, dims, N, 23)
    rng = np.random.default_rng(5)
    trip = rng.integers(0, N, (b, 2))
    trip[3] = (4, 4)                                       # src == dst: a zero gradient, never NaN
    gd = rng.integers(1, 6, b).astype(np.float64)
    TR, GD = _d(trip, dev), _d(gd, dev)
    with torch.no_grad():
        m.embeddings.embeds.data = _d(table, dev)
    emb = m.embeddings.embeds
    # autograd through Model.forward == rows + scatter, bit for bit up to the order of the atomics
    out = m(TR)
    out.sum().backward()
    g_auto, gs_auto = emb.grad.clone(), m.scale.grad.clone()
    rows, _ = ops.vector_backward_rows(emb.data, emb.data, model, TR, grad_out=torch.ones(b, dtype=torch.float64, device=dev),
                                       scale=m.scale.data, scale_coef=1.0)
    # the exact rows of the host formulas (autograd in torch ops) give the size of the bound
    xt = torch.from_numpy(table).requires_grad_(True)
    keep = trip[:, 0] != trip[:, 1]          # (torch's sqrt has no gradient at 0; the kernel's is defined as 0)
    d_host = 1.3 * mv.torch_dist(xt[trip[keep, 0]], xt[trip[keep, 1]], model)
    (g_host,) = torch.autograd.grad(d_host.sum(), xt)
    kappa = float(np.max([vh.factor_kappa(g, pair_sums(model, table[trip[:, 0]], table[trip[:, 1]])[:, k])
                          for k, g in enumerate(vh.FACTORS[model])]))
    tol = accumulation_bound(model, dims, table, trip, rows.cpu().numpy(), kappa)
    assert bool(torch.isfinite(g_auto).all())
    assert (np.abs(g_auto.cpu().numpy() - g_host.numpy()).max(1) <= tol + 1e-300).all()
    gt = torch.zeros_like(emb.data)
    ops.scatter_add_flat_rows_(gt, rows, torch.cat((TR[:, 0], TR[:, 1])).contiguous())
    assert (np.abs((gt - g_auto).cpu().numpy()).max(1) <= tol).all()
    assert abs(float(gs_auto) - float(out.detach().sum()) / 1.3) <= 1e-12 * abs(float(gs_auto))
    # fused loss + backward against AverageDistortionLoss + autograd
    emb.grad = None; m.scale.grad = None
    loss = AverageDistortionLoss().calculate_loss(GD, m(TR))
    loss.backward()
    g_ref, gs_ref = emb.grad.clone(), m.scale.grad.clone()
    emb.grad = None; m.scale.grad = None
    fused = m.fused_loss_backward(TR, GD)
    assert abs(float(fused) - float(loss)) <= 1e-12 * abs(float(loss))
    rows_l = torch.empty(2 * b, dims, dtype=torch.float64, device=dev)
    m.scale.grad.zero_()
    loss_r = m.fused_loss_backward_rows(TR, GD, rows_l)
    assert abs(float(loss_r) - float(loss)) <= 1e-12 * abs(float(loss))
    tol_l = accumulation_bound(model, dims, table, trip, rows_l.cpu().numpy(), kappa)
    assert (np.abs((emb.grad - g_ref).cpu().numpy()).max(1) <= tol_l).all()
    assert abs(float(m.scale.grad) - float(gs_ref)) <= 1e-11 * abs(float(gs_ref))
    # the segment-sum route: the same bits in two runs, and the scatter's values
    order, rowptr = ops.sorted_slots(torch.cat((TR[:, 0], TR[:, 1])), N)
    runs = []
    for _ in range(2):
        r = torch.empty(2 * b, dims, dtype=torch.float64, device=dev)
        m.fused_loss_backward_rows(TR, GD, r)
        gdet = torch.zeros_like(emb.data)
        ops.segment_sum_rows_(gdet, r, order[0], rowptr[0])
        runs.append(gdet)
    assert torch.equal(runs[0], runs[1])
    assert (np.abs((runs[0] - g_ref).cpu().numpy()).max(1) <= tol_l).all()
    assert ops.check_status(dev) == (0, 0)


# ------------------------------------------------------------------------------------------------ rows and the optimiser
@pytest.mark.parametrize("model", vh.MODELS)
def test_row_operations_and_rsgd_match_the_fixtures(model, dev):
    from sympa_amd import ops
    from sympa_amd.embeddings import ManifoldFactory
    from sympa_amd.manifolds.base import ManifoldParameter
    from sympa_amd.optim import RiemannianSGD
    tally = vh.Tally()
    for dims in vh.dims_of(model):
        rows = vh.row_fixture(model, dims)
        man = ManifoldFactory.get_manifold(model, "riem", dims)
        X, G = _d(rows["x"], dev), _d(rows["g"], dev)
        vh.check_rows(tally, model, dims, man.egrad2rgrad(X, G).cpu().numpy(), rows["egrad2rgrad"], rows["egrad2rgrad_kappa"],
                      f"{model} dims {dims} egrad2rgrad")
        vh.check_rows(tally, model, dims, man.projx(_d(rows["projx_in"], dev)).cpu().numpy(), rows["projx_out"], 1.0,
                      f"{model} dims {dims} projx")
        assert man.projected_points == int(rows["projx_moved"].sum())
        man.projected_points = 0
        for name in vh.STEPS:
            lr, wd = vh.STEP_ARGS[name]
            p = ManifoldParameter(X.clone(), manifold=man)
            p.grad = G.clone()
            RiemannianSGD([p], lr=lr, weight_decay=wd).step()
            vh.check_rows(tally, model, dims, p.data.cpu().numpy(), rows["rsgd_" + name], rows["rsgd_" + name + "_kappa"],
                          f"{model} dims {dims} rsgd {name}")
            assert man.projected_points == int(rows["rsgd_" + name + "_moved"].sum()), (model, dims, name)
            man.projected_points = 0
        # the clip of runner.py:115 folded into the step: the same row as a step on the scaled gradient
        sq = (G * G).sum().reshape(1)
        a, b2 = X.clone(), X.clone()
        ops.vector_rsgd_step_(a, G, model, 0.01, 0.1, clip_sqnorm=sq, max_norm=0.5)
        coef = min(1.0, 0.5 / (float(sq.sqrt()) + 1e-6))
        ops.vector_rsgd_step_(b2, G * coef, model, 0.01, 0.1)
        assert float((a - b2).abs().max()) <= 8 * vh.EPS64 * float(b2.abs().max())
    assert ops.check_status(dev) == (0, 0)
    tally.report(f"GPU rows {model}")


@pytest.mark.parametrize("model", vh.MODELS)
def test_fifty_steps_at_lr_10_stay_on_the_manifold(model, dev):
    """Rows 0..15 take 50 RiemannianSGD steps at lr = 10 on sum_i d(x_i, c_i) towards the anchors c_i = rows 16..31 (whose
    gradient is zeroed).  The Riemannian gradient of a distance has length 1, so every step moves a row by 10: far past its
    anchor, and a Poincare row out of the ball, where projx has to bring it back."""
    from sympa_amd import ops
    from sympa_amd.optim import RiemannianSGD
    dims = 8
    fx = vh.pair_fixture(model, dims, "generic")
    m = make_model(model, dims, 32, dev)
    with torch.no_grad():
        m.embeddings.embeds.data = torch.cat((_d(fx["x"], dev), _d(fx["y"], dev))).contiguous()
    opt = RiemannianSGD(m.parameters(), lr=10.0)
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
    assert torch.equal(m.embeddings.embeds.data[16:].cpu(), torch.from_numpy(fx["y"])) or model in ("lorentz", "sphere", "prod-hysph",
                                                                                                    "prod-sphsph")
    if model == "poincare":
        assert m.manifold.projected_points > 0


# ------------------------------------------------------------------------------------------------ end to end
def tree_csr(n):
    nbrs = [[] for _ in range(n)]
    for i in range(1, n):
        nbrs[i].append((i - 1) // 2)
        nbrs[(i - 1) // 2].append(i)
    rowptr = np.cumsum([0] + [len(a) for a in nbrs]).astype(np.int64)
    cols = np.concatenate([sorted(a) for a in nbrs]).astype(np.int32)
    return rowptr, cols


@pytest.mark.parametrize("model", vh.MODELS)
def test_training_a_tree_end_to_end(model, dev):
    from sympa_amd import ops
    from sympa_amd.graph import GraphDistances
    from sympa_amd.losses import AverageDistortionLoss
    from sympa_amd.metrics import MeanAveragePrecisionMetric
    from sympa_amd.optim import RiemannianSGD
    torch.manual_seed(3)
    n = 31
    hops = GraphDistances(*tree_csr(n), device=dev)
    trip = hops.triplets()
    ids, gd = trip[:, :2].contiguous(), trip[:, 2].to(torch.float64)
    m = make_model(model, 4, n, dev)
    opt = RiemannianSGD(m.parameters(), lr=0.05)
    loss_fn = AverageDistortionLoss()
    with torch.no_grad():
        start = float(loss_fn.calculate_loss(gd, m(ids)))
    g = torch.Generator().manual_seed(1)
    for step in range(100):
        sel = torch.randint(0, ids.shape[0], (64,), generator=g).to(dev)
        opt.zero_grad(set_to_none=False)
        if step % 2:
            m.fused_loss_backward(ids[sel].contiguous(), gd[sel])
        else:                                            # the classic loop: forward, loss, backward
            loss_fn.calculate_loss(gd[sel], m(ids[sel].contiguous())).backward()
        opt.step()
    with torch.no_grad():
        end = float(loss_fn.calculate_loss(gd, m(ids)))
        mat = m.distance_matrix()
    print(f"[vector] {model} dims 4, 31-node tree, 100 steps: loss {start:.4g} -> {end:.4g}", flush=True)
    assert np.isfinite(end) and end < start, (model, start, end)
    assert m.check_all_points()[0] and ops.check_status(dev) == (0, 0)
    # the evaluations against their torch formulations on the gathered matrix
    dist = mat[ids[:, 0], ids[:, 1]]
    want = float(((dist - gd).abs() / gd).mean())
    got = m.evaluate(ids, gd, batch_size=100)
    assert np.isfinite(got) and abs(got - want) <= 1e-12 * abs(want)
    got_all = m.evaluate_all_pairs(hops)
    assert np.isfinite(got_all) and abs(got_all - want) <= 1e-12 * abs(want)          # i < j, every pair reachable: the same set
    metric = MeanAveragePrecisionMetric((ids.cpu(), gd.cpu()))
    got_map = m.mean_average_precision(metric, dtype=torch.float64, max_block_bytes=8 * n * 7)
    want_map = metric.calculate_metric(mat.cpu().numpy())
    assert np.isfinite(got_map) and 0.0 < got_map <= 1.0 and abs(got_map - want_map) <= 1e-12


def test_off_manifold_poincare_point_is_nan_and_flagged(dev):
    from sympa_amd import ops
    x = torch.zeros(70, 4, dtype=torch.float64, device=dev)
    x[:, 1] = 0.5
    x[66, :] = 0.0
    x[66, 0] = 1.0                                          # |x| = 1, in the last, partly filled wave
    y = torch.full((70, 4), 0.1, dtype=torch.float64, device=dev)
    assert ops.check_status(dev) == (0, 0)
    out = ops.vector_dist_forward(x, y, "poincare")
    assert bool(torch.isnan(out[66])) and bool(torch.isfinite(torch.cat((out[:66], out[67:]))).all())
    with pytest.raises(AssertionError):
        ops.check_status(dev)
    x[66, 0] = 0.5                                          # the next clean call is unaffected
    out = ops.vector_dist_forward(x, y, "poincare")
    assert bool(torch.isfinite(out).all()) and ops.check_status(dev) == (0, 0)
    # an index outside the table: NaN, IndexError from the status word, nothing read out of bounds
    t = torch.tensor([[0, 1], [2, 70], [-1, 3]], device=dev)
    out = ops.vector_model_forward(x, t, "poincare")
    assert bool(torch.isfinite(out[0])) and bool(torch.isnan(out[1:]).all())
    with pytest.raises(IndexError):
        ops.check_status(dev)


def test_graphed_step_refuses_the_vector_models(dev):
    from sympa_amd.optim import RiemannianSGD
    from sympa_amd.train_step import GraphedTrainStep
    m = make_model("poincare", 4, 9, dev)
    with pytest.raises(NotImplementedError, match="classic loop"):
        GraphedTrainStep(m, RiemannianSGD(m.parameters(), lr=0.1), 8, 50.0, dev)
