"""GPU: the geodesic RiemannianAdam step -- C-ABI sympa_radam_step_exp through ops.radam_step_exp_, RiemannianAdam(retraction="exp")
and tools/train_siegel.py --optim radam --retraction exp -- against the 100-digit fixtures, the g++ build of the same arithmetic
and the step composed from the entries that existed before it.  Bounds: tests/radam_exp_helpers.py (the same constants as the CPU
build's)."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import radam_exp_helpers as rh

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
pytestmark = pytest.mark.gpu
ROWS = (1, 63, 64, 65, 130)      # the wave edges and a ragged tail over three one-wave blocks
BETAS = (0.9, 0.999)
EPS_ADAM = 1e-7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(dev)


def _manifold(model, n):
    from sympa_amd.manifolds import BoundedDomainManifold, UpperHalfManifold
    return (UpperHalfManifold if model == "upper" else BoundedDomainManifold)(dims=n)


def _kappa(model, x):
    """The condition of every point of x [b,2,n,n] (numpy): of Im x (upper), of I - x conj x (bounded)."""
    xc = x[:, 0] + 1j * x[:, 1]
    a = x[:, 1] if model == "upper" else np.eye(x.shape[-1]) - xc @ xc.conj().transpose(0, 2, 1)
    ev = np.linalg.eigvalsh(a)
    return ev[:, -1] / ev[:, 0]


def _step(dev, model, x, grad, m, s, lr, wd, pow1, pow2, counter=None, **kw):
    """One launch on copies -> (x', m', s1) as numpy."""
    from sympa_amd import ops
    t, mm, ss = _d(x, dev), _d(m, dev), _d(s, dev)
    pows = torch.tensor([pow1, pow2], dtype=torch.float64, device=dev)
    ops.radam_step_exp_(t, _d(grad, dev), mm, ss, pows, model, lr, BETAS, EPS_ADAM, wd, counter=counter, **kw)
    return t.cpu().numpy(), mm.cpu().numpy(), ss.cpu().numpy()


@pytest.mark.parametrize("b", ROWS)
@pytest.mark.parametrize("n", rh.DIMS)
@pytest.mark.parametrize("model", rh.MODELS)
def test_kernel_against_fixtures_and_host_build(dev, model, n, b):
    from sympa_amd import ops
    f = rh.fixture(model, n)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    for c in rh.cases(f):
        x, grad, m, s, wy, wm, ws, kappa = (rh.tile_rows(c[k], b) for k in ("x", "grad", "m", "s", "y", "m_out", "s1", "kappa"))
        got = _step(dev, model, x, grad, m, s, c["lr"], c["wd"], c["pow1"], c["pow2"], counter=cnt)
        ops.check_status(dev)
        host = rh.hostsim_radam_exp(x, grad, m, s, model, c["lr"], c["betas"], c["eps_adam"], c["wd"], c["pow1"], c["pow2"])
        assert host[4] == 0
        exact, against_host = rh.errors(*got, wy, wm, ws), rh.errors(*got, *host[:3])
        for o in rh.OUTPUTS:
            bound = rh.bound(model, o, c["k"], kappa)
            print(f"{model} n={n} b={b} state {c['st']} lr {c['lr']:g}: {o} kernel / exact {(exact[o] / (rh.EPS64 * kappa)).max():.3g}, "
                  f"kernel / g++ {(against_host[o] / (rh.EPS64 * kappa)).max():.3g} eps kappa")
            assert (exact[o] <= bound).all(), (o, c["st"], c["k"], float((exact[o] / (rh.EPS64 * kappa)).max()))
            assert (against_host[o] <= bound).all(), (o, c["st"], c["k"], float((against_host[o] / (rh.EPS64 * kappa)).max()))
    assert int(cnt.item()) == 0


def _composed(man, model, x, grad, m, s, lr, wd, pow1, pow2, counter=None):
    """The step from the entries that existed before it: egrad2rgrad, sym and moments in torch, the invariant norm from
    SiegelManifold.invariant_inner, transp_exp with the point, projx."""
    from sympa_amd import ops
    sym = lambda a: 0.5 * (a + a.transpose(-1, -2))
    g = sym(ops.egrad2rgrad(x, grad + wd * x, model))
    m1 = BETAS[0] * sym(m) + (1.0 - BETAS[0]) * g
    s1 = BETAS[1] * s + (1.0 - BETAS[1]) * man.invariant_inner(x, g)[:, 0, 0, 0]
    alpha = lr / ((1.0 - pow1) * ((s1 / (1.0 - pow2)).sqrt() + EPS_ADAM))
    y, mt = ops.transp_exp(x, -alpha.view(-1, 1, 1, 1) * m1, m1, model, return_point=True)
    return ops.projx(y, model, counter=counter), mt, s1, y


@pytest.mark.parametrize("n", (3, 6))
@pytest.mark.parametrize("model", rh.MODELS)
def test_the_optimiser_against_the_step_composed_from_the_separate_entries(dev, model, n):
    from sympa_amd import ops
    from sympa_amd.manifolds.base import ManifoldParameter
    from sympa_amd.optim import RiemannianAdam
    man = _manifold(model, n)
    table = ManifoldParameter(_d(rh.tile_rows(rh.fixture(model, n)["x"], 130), dev), manifold=man)
    lr, k = 0.1, 1                                                   # the lr class of the bound: steps of invariant length <= 0.1
    opt = RiemannianAdam([table], lr=lr, betas=BETAS, eps=EPS_ADAM, retraction="exp")
    gen = torch.Generator(device=dev).manual_seed(100 + n)
    for t in (1, 2, 3):
        table.grad = torch.randn(table.shape, dtype=torch.float64, device=dev, generator=gen)
        x0 = table.data.clone()
        if t == 1:
            m0, s0 = torch.zeros_like(x0), torch.zeros(130, dtype=torch.float64, device=dev)
        else:
            m0, s0 = opt.state[table]["exp_avg"].clone(), opt.state[table]["exp_avg_sq"].clone()
        want_x, want_m, want_s, _ = _composed(man, model, x0, table.grad, m0, s0, lr, 0.0, BETAS[0] ** t, BETAS[1] ** t)
        opt.step()
        ops.check_status(dev)
        st = opt.state[table]
        assert st["exp_avg_sq"].shape == (130,) and st["exp_avg"].shape == table.shape
        err = rh.errors(table.data.cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(),
                        want_x.cpu().numpy(), want_m.cpu().numpy(), want_s.cpu().numpy())
        kappa = _kappa(model, x0.cpu().numpy())
        for o in rh.OUTPUTS:
            print(f"{model} n={n} step {t}: {o} optimiser / composition {(err[o] / (rh.EPS64 * kappa)).max():.3g} eps kappa")
            assert (err[o] <= rh.bound(model, o, k, kappa)).all(), (o, t, float((err[o] / (rh.EPS64 * kappa)).max()))
    want = torch.tensor([BETAS[0] ** 3, BETAS[1] ** 3], dtype=torch.float64)
    assert torch.allclose(opt.state[table]["bias_pows"].cpu(), want, rtol=4 * rh.EPS64, atol=0)
    # snapshot / restore work on this state as on the linear step's
    snap = opt.snapshot_state()
    kept = table.data.clone()
    opt.step()
    opt.restore_state(snap)
    assert torch.equal(opt.state[table]["bias_pows"].cpu(), snap[1][table]["bias_pows"].cpu()) and not torch.equal(table.data, kept)


@pytest.mark.parametrize("model", rh.MODELS)
def test_a_first_step_has_adams_unit_length(dev, model):
    """dist(x, x') / dist_scale = lr |g|_x / (|g|_x + eps_adam) through manifold.dist on the device, lr = 0.1 and 1: the bound of the
    new point at that lr class carried into the distance (compose_unit), plus 64 eps for the distance itself."""
    from sympa_amd import ops
    from sympa_amd.manifolds.base import ManifoldParameter
    from sympa_amd.optim import RiemannianAdam
    for n in (2, 5, 8):
        man = _manifold(model, n)
        f = rh.fixture(model, n)
        for lr, k in ((0.1, 1), (1.0, 2)):
            x0 = _d(f["x"], dev)
            table = ManifoldParameter(x0.clone(), manifold=man)
            table.grad = _d(f["grad"], dev)
            RiemannianAdam([table], lr=lr, betas=BETAS, eps=EPS_ADAM, retraction="exp").step()
            ops.check_status(dev)
            g = ops.egrad2rgrad(x0, table.grad, model)
            gx = man.invariant_inner(x0, 0.5 * (g + g.transpose(-1, -2)))[:, 0, 0, 0].sqrt().cpu().numpy()
            exact = lr * gx / (gx + EPS_ADAM)
            got = (man.dist(x0, table.data) / man.dist_scale).cpu().numpy().reshape(-1)
            ops.check_status(dev)
            fac = f["kappa"] * np.exp(2.0 * exact)
            tol = rh.C_RADAM[model]["y"][k] * rh.compose_unit(fac, table.data.cpu().numpy(), exact[:, None]) + 64 * rh.EPS64
            off = np.abs(got - exact) / exact
            print(f"{model} n={n} lr={lr}: unit step off by {off.max():.2e}, tolerance {tol.min():.2e}")
            assert (off <= tol).all(), (model, n, lr, float((off / tol).max()))


def _near_the_boundary(model, x, margin):
    """The rows of x moved to `margin` times eps from the eps-boundary: Im x scaled so that its smallest eigenvalue is margin * eps
    (upper), x scaled to the spectral norm 1 - margin * eps (bounded)."""
    x = np.array(x)
    for i in range(len(x)):
        if model == "upper":
            x[i, 1] *= margin * rh.EPS_INTERIOR / np.linalg.eigvalsh(x[i, 1]).min()
        else:
            x[i] *= (1.0 - margin * rh.EPS_INTERIOR) / np.linalg.norm(x[i, 0] + 1j * x[i, 1], 2)
    return x


@pytest.mark.parametrize("model", rh.MODELS)
def test_the_clamp_counts_and_moves_the_rows_projx_moves(dev, model):
    """Rows just inside the eps-interior, lr = 1 on a first step (an invariant length of 1) with the gradient pointing outward on the
    even rows and no gradient on the odd rows, which stay where they are.  upper: Im x at 1.2 eps, grad = i (Im x)^-1, so that
    g = i Im x and every eigenvalue of Im x shrinks by exp(-1 / sqrt n) < 1 / 1.2; bounded: spectral norm 1 - 2 eps, grad = -x.
    projected_count is the number of rows ops.projx moves on the composed result, and those rows equal it within the bound of
    the lr = 1 class; exp_avg stays as transported to y.  The bounded rows are 2 eps from the boundary, where
    I - x conj(x) is a difference of nearly equal numbers: formed with an absolute error eps it has the relative error
    eps / lambda_min(I - x conj x), which takes the place of kappa (<= it) in the bound of these rows."""
    from sympa_amd import ops
    for n in (2, 5):
        man = _manifold(model, n)
        f = rh.fixture(model, n)
        x = _near_the_boundary(model, rh.tile_rows(f["x"][1:], 70), 1.2 if model == "upper" else 2.0)
        grad = np.zeros_like(x)
        out = np.arange(70) % 2 == 0
        if model == "upper":
            grad[out, 1] = np.linalg.inv(x[out, 1])
            cond = _kappa(model, x)
        else:
            grad[out] = -x[out]
            xc = x[:, 0] + 1j * x[:, 1]
            cond = 1.0 / np.linalg.eigvalsh(np.eye(n) - xc @ xc.conj().transpose(0, 2, 1))[:, 0]
        zero_m, zero_s = torch.zeros(x.shape, dtype=torch.float64, device=dev), torch.zeros(70, dtype=torch.float64, device=dev)
        c_want = torch.zeros(1, dtype=torch.int32, device=dev)
        want_x, want_m, want_s, y = _composed(man, model, _d(x, dev), _d(grad, dev), zero_m, zero_s, 1.0, 0.0, BETAS[0], BETAS[1],
                                              counter=c_want)
        c_got = torch.zeros(1, dtype=torch.int32, device=dev)
        got = _step(dev, model, x, grad, zero_m.cpu().numpy(), zero_s.cpu().numpy(), 1.0, 0.0, BETAS[0], BETAS[1], counter=c_got)
        ops.check_status(dev)
        moved = (want_x != y).flatten(1).any(1).cpu().numpy()
        print(f"{model} n={n}: the clamp moved {int(c_got.item())} of 70 rows (composition: {int(c_want.item())})")
        assert 0 < int(c_want.item()) <= 35 and int(moved.sum()) == int(c_want.item()) and not moved[~out].any()
        assert int(c_got.item()) == int(c_want.item())
        ws = want_s.cpu().numpy()
        err = rh.errors(got[0], got[1], np.where(out, got[2], 1.0), want_x.cpu().numpy(), want_m.cpu().numpy(), np.where(out, ws, 1.0))
        for o in rh.OUTPUTS:
            print(f"{model} n={n}: {o} step / composition at the clamp {(err[o] / (rh.EPS64 * cond)).max():.3g} eps cond")
            assert (err[o] <= rh.bound(model, o, 2, cond)).all(), (model, n, o, float((err[o] / (rh.EPS64 * cond)).max()))
        assert (got[2][~out] == 0.0).all() and (ws[~out] == 0.0).all()


@pytest.mark.parametrize("model", rh.MODELS)
def test_the_folded_clip_equals_the_scaled_gradient(dev, model):
    for n in (3, 7):
        f = rh.fixture(model, n)
        c = next(c for c in rh.cases(f) if c["st"] == 1 and c["k"] == 1)
        x, grad, m, s, kappa = (rh.tile_rows(c[k], 65) for k in ("x", "grad", "m", "s", "kappa"))
        total, max_norm = 7.3, 0.9
        coef = min(1.0, max_norm / (np.sqrt(total) + 1e-6))
        assert coef < 1.0
        sq = torch.tensor([total], dtype=torch.float64, device=dev)
        a = _step(dev, model, x, grad, m, s, c["lr"], c["wd"], c["pow1"], c["pow2"], clip_sqnorm=sq, max_norm=max_norm)
        b = _step(dev, model, x, coef * grad, m, s, c["lr"], c["wd"], c["pow1"], c["pow2"])
        err = rh.errors(*a, *b)
        for o in rh.OUTPUTS:
            assert (err[o] <= rh.bound(model, o, c["k"], kappa)).all(), (model, n, o)
        # a norm below max_norm leaves the gradient alone: the bits of the entry without a clip
        sq.fill_(0.25)
        a = _step(dev, model, x, grad, m, s, c["lr"], c["wd"], c["pow1"], c["pow2"], clip_sqnorm=sq, max_norm=max_norm)
        b = _step(dev, model, x, grad, m, s, c["lr"], c["wd"], c["pow1"], c["pow2"])
        assert all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("model", rh.MODELS)
def test_a_row_outside_the_domain_sets_the_status_words_and_nothing_else(dev, model):
    from sympa_amd import ops
    n = 4
    f = rh.fixture(model, n)
    c = next(c for c in rh.cases(f) if c["st"] == 1 and c["k"] == 1)
    x, grad, m, s = (np.array(rh.tile_rows(c[k], 65)) for k in ("x", "grad", "m", "s"))
    clean = _step(dev, model, x, grad, m, s, c["lr"], c["wd"], c["pow1"], c["pow2"])
    ops.check_status(dev)
    bad = x.copy()
    if model == "upper":
        bad[17, 1] = -bad[17, 1]                      # Im x negative definite
    else:
        bad[17] = 0.0
        bad[17, 0] = 1.5 * np.eye(n)                  # singular values above 1
    got = _step(dev, model, bad, grad, m, s, c["lr"], c["wd"], c["pow1"], c["pow2"])
    buf = ops._status_buf(dev)
    bits, count = (int(v) for v in buf.tolist())
    buf.zero_()
    assert bits & ops.ST_NOT_PD and count == 1, (bits, count)
    keep = np.arange(65) != 17
    assert all(np.array_equal(p[keep], q[keep]) for p, q in zip(got, clean))


def test_the_entry_refuses_the_dual_model_and_dims_9_and_touches_nothing(dev):
    from sympa_amd import _lib, ops
    lib = _lib.load()
    for n, model, code in ((4, _lib.DEFINES["SYMPA_MODEL_DUAL"], "SYMPA_ERR_BAD_ARG"), (9, 0, "SYMPA_ERR_UNSUPPORTED_DIMS")):
        gen = torch.Generator(device=dev).manual_seed(n)
        t, g, m = (torch.randn(5, 2, n, n, dtype=torch.float64, device=dev, generator=gen) for _ in range(3))
        s = torch.rand(5, dtype=torch.float64, device=dev, generator=gen)
        pows = torch.tensor(BETAS, dtype=torch.float64, device=dev)
        before = [a.clone() for a in (t, m, s)]
        rc = lib.sympa_radam_step_exp(t.data_ptr(), g.data_ptr(), m.data_ptr(), s.data_ptr(), 5, n, model, 1e-2, BETAS[0], BETAS[1],
                                      EPS_ADAM, 0.0, pows.data_ptr(), 1e-5, None, 0.0, None, ops._status_buf(dev).data_ptr(),
                                      ops._stream())
        torch.cuda.synchronize(dev)
        assert rc == _lib.DEFINES[code], (n, model, rc)
        assert all(torch.equal(a, b) for a, b in zip((t, m, s), before))
    ops.check_status(dev)


def test_the_graphed_step_refuses_the_optimiser(dev):
    from sympa_amd.manifolds.base import ManifoldParameter
    from sympa_amd.optim import RiemannianAdam
    from sympa_amd.train_step import GraphedTrainStep
    table = ManifoldParameter(_d(rh.fixture("upper", 2)["x"], dev), manifold=_manifold("upper", 2))
    opt = RiemannianAdam([table], lr=1e-2, retraction="exp")
    with pytest.raises(NotImplementedError, match="linear retraction"):
        GraphedTrainStep(None, opt, 8, 50.0, dev)


@pytest.mark.parametrize("manifold", rh.MODELS)
def test_a_forty_step_training_run(manifold, tmp_path, dev):
    """The classic loop of tools/train_siegel.py with --optim radam --retraction exp on the 4 x 4 grid (120 pairs, 10 steps an epoch,
    4 epochs) at n = 2: the status words stay clean, every row is on the manifold, loss and distortion are finite.  No claim on the
    loss value."""
    import networkx as nx
    import train_siegel
    from sympa_amd import ops
    path = tmp_path / "grid4x4.edges"
    nodes = {v: i for i, v in enumerate(nx.grid_2d_graph(4, 4).nodes())}
    path.write_text("".join(f"{nodes[a]} {nodes[b]}\n" for a, b in nx.grid_2d_graph(4, 4).edges()))
    argv = ["--edges", str(path), "--manifold", manifold, "--metric", "riem", "--dims", "2", "--epochs", "4", "--batch_size", "12",
            "--val_every", "4", "--learning_rate", "0.01", "--burnin", "0", "--seed", "42", "--optim", "radam", "--retraction", "exp"]
    model, hist = train_siegel.train(train_siegel.parser().parse_args(argv), log=lambda *_: None)
    ops.check_status(dev)
    assert np.isfinite(hist[-1][1]) and np.isfinite(hist[-1][2])
    table = model.embeddings.embeds
    assert table.shape[0] == 16
    for row in table.data:
        ok, reason = model.manifold._check_point_on_manifold(row)
        assert ok, reason
