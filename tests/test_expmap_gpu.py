"""GPU: the exponential / logarithm maps and the RiemannianSGD step along the geodesic -- C-ABI sympa_expmap / sympa_logmap /
sympa_rsgd_step_exp through ops, SiegelManifold.expmap / logmap / geodesic, RiemannianSGD(retraction="exp") and
tools/train_siegel.py --retraction exp -- against the 100-digit fixtures, the g++ build of the same arithmetic and the composition
of the separate entries.  Bounds: tests/expmap_helpers.py (the same constants as the CPU build's)."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import expmap_helpers as eh

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
pytestmark = pytest.mark.gpu
MODELS = ("upper", "bounded")
ROWS = (1, 63, 64, 65, 130)      # the wave edges and a ragged tail over three one-wave blocks


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _length(model, z, u):
    """The invariant length of the symmetric tangent u at z: 2 |L^-1 u L^-T / 2|_F (upper) resp. |C^-1 u C^-T|_F (bounded), in numpy."""
    out = np.zeros(len(z))
    for i, (p, t) in enumerate(zip(z, u)):
        if model == "upper":
            lo = np.linalg.cholesky(p[1])
        else:
            w = p[0] + 1j * p[1]
            lo = np.linalg.cholesky(np.eye(len(w)) - w @ w.conj().T)
        out[i] = np.linalg.norm(np.linalg.solve(lo, np.linalg.solve(lo, (t[0] + 1j * t[1])).T).T)
    return out


@pytest.mark.parametrize("b", ROWS)
@pytest.mark.parametrize("n", eh.DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_kernels_against_fixtures_host_build_and_composition(dev, model, n, b):
    from sympa_amd import ops
    f = eh.fixture(model, n)
    # 1. expmap: fixture rows tiled to b, against the exact values and against the g++ build, per norm of the tangent
    z, u, want, kappa, k = (eh.tile_rows(a, b) for a in eh.exp_inputs(f))
    got = ops.expmap(_d(z, dev), _d(u, dev), model).cpu().numpy()
    ops.check_status(dev)
    host, st = eh.hostsim_expmap(z, u, model)
    assert st == 0
    r, rh = eh.row_err(got, want) / (eh.EPS64 * kappa), eh.row_err(got, host) / (eh.EPS64 * kappa)
    per = lambda x: [float(f"{x[k == j].max():.3g}") if (k == j).any() else 0.0 for j in range(4)]
    print(f"{model} n={n} b={b}: expmap kernel / exact per norm {per(r)}, kernel / g++ per norm {per(rh)}")
    bound = eh.exp_bound(model, kappa, k)
    assert (eh.row_err(got, want) <= bound).all() and (eh.row_err(got, host) <= bound).all(), (per(r), per(rh))
    # 2. logmap
    z1, z2, lg, lf = (eh.tile_rows(a, b) for a in (f["z1"], f["z2"], f["log"], eh.log_factor(f)))
    got = ops.logmap(_d(z1, dev), _d(z2, dev), model).cpu().numpy()
    ops.check_status(dev)
    host, st = eh.hostsim_logmap(z1, z2, model)
    assert st == 0
    r = eh.row_err(got, lg) / (eh.EPS64 * lf)
    rh = eh.row_err(got, host) / (eh.EPS64 * lf)
    print(f"{model} n={n} b={b}: logmap kernel / exact {r.max():.3g}, kernel / g++ {rh.max():.3g}")
    assert (r <= eh.C_LOG[model]).all() and (rh <= eh.C_LOG[model]).all(), (float(r.max()), float(rh.max()))
    # 3. the step = projx(expmap(x, -lr egrad2rgrad(x, g))) composed from the separate entries (wd = 0: the step forms g + wd x in one
    #    fused multiply-add).  Not promised bit for bit: inside the one kernel the compiler may contract -lr * r into the sum that
    #    symmetrises it, one rounding instead of two on u, which the map then carries like any rounding of its input: every row steps
    #    an invariant length of 1, and the two results agree to the bound of expmap at that length, C_EXP[model][2] eps kappa.
    #    The rows the clamp moves are the same rows.
    table = eh.tile_rows(f["z1"], b)
    rng = np.random.RandomState(100 * n + b)
    g = rng.randn(*table.shape)
    g = g + g.transpose(0, 1, 3, 2)
    lr = 1e-2
    t_dev = _d(table, dev)
    r0 = -lr * ops.egrad2rgrad(t_dev, _d(g, dev), model).cpu().numpy()          # (egrad2rgrad is linear in g)
    g *= (1.0 / _length(model, table, 0.5 * (r0 + r0.transpose(0, 1, 3, 2))))[:, None, None, None]
    g_dev = _d(g, dev)
    rg = ops.egrad2rgrad(t_dev, g_dev, model)
    ex = ops.expmap(t_dev, -lr * rg, model)
    c_want = torch.zeros(1, dtype=torch.int32, device=dev)
    want = ops.projx(ex, model, counter=c_want).cpu().numpy()
    c_got = torch.zeros(1, dtype=torch.int32, device=dev)
    stepped = t_dev.clone()
    ops.rsgd_step_exp_(stepped, g_dev, model, lr, 0.0, counter=c_got)
    ops.check_status(dev)
    stepped = stepped.cpu().numpy()
    r = eh.row_err(stepped, want) / (eh.EPS64 * eh.tile_rows(f["kappa"], b))
    print(f"{model} n={n} b={b}: step / composition {r.max():.3g} of eps kappa, bit for bit: {np.array_equal(stepped, want)}, "
          f"moved {int(c_got.item())}")
    assert (r <= eh.C_EXP[model][2]).all(), float(r.max())
    assert int(c_got.item()) == int(c_want.item())
    hs, moved, st = eh.hostsim_rsgd_exp(table, g, model, lr, 0.0)
    assert st == 0 and int(moved.sum()) == int(c_got.item())


@pytest.mark.parametrize("model", MODELS)
def test_projected_count_counts_only_the_rows_the_clamp_moved(dev, model):
    """A table of interior rows with every fifth row put outside the eps-interior (upper: Im x scaled to 1e-7; bounded: spectral norm
    1 - 1e-7): the zero-gradient step is expmap(x, 0) = x, then the clamp moves exactly those rows."""
    from sympa_amd import ops
    for n in (2, 5, 8):
        f = eh.fixture(model, n)
        table = np.array(eh.tile_rows(f["z1"][f["case"] == "generic"], 70))
        out = np.arange(70) % 5 == 0
        for i in np.nonzero(out)[0]:
            if model == "upper":
                table[i, 1] *= 1e-7 / np.linalg.eigvalsh(table[i, 1]).max()
            else:
                table[i] *= (1.0 - 1e-7) / np.linalg.norm(table[i, 0] + 1j * table[i, 1], 2)
        t = _d(table, dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.rsgd_step_exp_(t, torch.zeros_like(t), model, 1e-2, 0.0, counter=cnt)
        ops.check_status(dev)
        assert int(cnt.item()) == int(out.sum()), (model, n)
        assert np.array_equal(t.cpu().numpy()[~out], table[~out]), (model, n)


@pytest.mark.parametrize("model", MODELS)
def test_manifold_surface_and_optimizer(dev, model):
    from sympa_amd import ops
    from sympa_amd.manifolds import BoundedDomainManifold, UpperHalfManifold
    from sympa_amd.manifolds.base import ManifoldParameter
    from sympa_amd.optim import RiemannianSGD
    n = 4
    man = (UpperHalfManifold if model == "upper" else BoundedDomainManifold)(dims=n)
    f = eh.fixture(model, n)
    keep = f["case"] != "far"
    x, y = _d(f["z1"][keep], dev), _d(f["z2"][keep], dev)
    lg = man.logmap(x, y)
    assert not lg.requires_grad and torch.equal(lg, ops.logmap(x, y, model))
    assert torch.equal(man.expmap(x, lg), ops.expmap(x, lg, model))
    mid = man.geodesic(0.5, x, y)
    assert torch.equal(mid, ops.expmap(x, 0.5 * lg, model))
    d, a, b = man.dist(x, y), man.dist(x, mid), man.dist(mid, y)
    ops.check_status(dev)
    # the unit of a composition of the two maps with the midpoint's constant, plus 64 eps for the three distances themselves
    tol = _d(eh.C_MID[model] * eh.compose_unit(eh.pair_condition(f)[keep], f["z2"][keep], f["log"][keep]), dev) + 64 * eh.EPS64
    assert ((a - 0.5 * d).abs() <= tol * d).all() and ((b - 0.5 * d).abs() <= tol * d).all()
    # the optimiser takes the new kernel: one step equals ops.rsgd_step_exp_ on a copy, and differs from the linear step
    table = ManifoldParameter(x.clone(), manifold=man)
    table.grad = torch.randn(x.shape, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    want = ops.rsgd_step_exp_(x.clone(), table.grad, model, 0.05, 0.0)
    lin = ops.rsgd_step_(x.clone(), table.grad, model, 0.05, 0.0)
    RiemannianSGD([table], lr=0.05, retraction="exp").step()
    assert torch.equal(table.data, want) and not torch.equal(table.data, lin)


def _train(manifold, dims, retraction, seed, lr, epochs=3):
    import train_siegel
    argv = ["--graph", "grid3d-125", "--manifold", manifold, "--metric", "riem", "--dims", str(dims), "--epochs", str(epochs),
            "--batch_size", "512", "--val_every", str(epochs), "--learning_rate", str(lr), "--burnin", "0", "--seed", str(seed),
            "--no_graph_step", "--retraction", retraction]
    model, hist = train_siegel.train(train_siegel.parser().parse_args(argv), log=lambda *_: None)
    return hist[-1][1], hist[-1][2], model.manifold.projected_points


@pytest.mark.parametrize("dims", (2, 5))
@pytest.mark.parametrize("manifold", MODELS)
def test_a_short_training_run_with_the_exponential_retraction(manifold, dims):
    """The classic loop of tools/train_siegel.py on the 125-node grid, 3 epochs of 16 steps: a finite loss, and a final distortion
    no worse than the linear run's by more than the spread of the linear run over three seeds.  Figures: DESIGN.md."""
    lin = [_train(manifold, dims, "linear", seed, 0.02) for seed in (42, 43, 44)]
    loss, dist, projected = _train(manifold, dims, "exp", 42, 0.02)
    spread = max(d for _, d, _ in lin) - min(d for _, d, _ in lin)
    print(f"{manifold} n={dims}: distortion linear {[round(d, 5) for _, d, _ in lin]} (spread {spread:.5f}), exp {dist:.5f}; "
          f"projected linear {[p for _, _, p in lin]}, exp {projected}")
    assert np.isfinite(loss) and np.isfinite(dist)
    assert dist <= lin[0][1] + spread, (dist, lin)


def test_the_exponential_step_needs_no_projection_where_the_linear_one_does():
    """upper, n = 2, a step size at which the linear retraction leaves the eps-interior on some rows (projected_points > 0): the
    geodesic stays inside, nothing is projected.  Measured over 2 epochs (32 steps): lr 0.1: 0 / 0 rows, 0.3: 1 / 0, 1.0: 2 / 0
    (loss per triplet 1.48 linear, 0.94 exp), 3.0: 7 / 1 (a step of that length reaches the eps-boundary itself)."""
    lr = 1.0
    _, _, p_lin = _train("upper", 2, "linear", 42, lr, epochs=2)
    loss, _, p_exp = _train("upper", 2, "exp", 42, lr, epochs=2)
    print(f"upper n=2 lr={lr}: projected points linear {p_lin}, exp {p_exp}")
    assert p_lin > 0, "no row left the interior at this step size: the comparison shows nothing"
    assert np.isfinite(loss) and p_exp == 0
