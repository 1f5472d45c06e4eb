"""CPU (`-m "not gpu"`): the exponential / logarithm maps and the geodesic RiemannianSGD row (g++ build of
sympa_amd/csrc/siegel_expmap_math.hpp, tests/hostsim/hostsim_expmap.cpp) against the 100-digit fixtures, the identities they
satisfy, the argument validation of the three C-ABI entries and the refusals of the Python surface.  Bounds: tests/expmap_helpers.py.

The metric of the maps is the invariant one, of which the riem distance measures c times the length.  For the upper model that is
`inner`.  For the bounded model it is inner(x, conj u, conj u): the reference's bounded inner (bounded_domain.py:86-116, restated by
oracle.bounded_inner and sympa_tangent_sqnorm) has its two inverses the other way round and differs from the invariant norm by up to
48 % on the fixture points at n >= 2 (equal at n = 1 and at real points).  The identity dist = c sqrt(inner) is therefore checked
with conj(u) for the bounded model; test_bounded_inner_is_the_invariant_norm_at_conj_u pins the relation down."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import siegel_oracle as so
from sympa_amd import _lib
from tests import expmap_helpers as eh

MODELS = ("upper", "bounded")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy())


def _conj(a):
    c = np.array(a, copy=True)
    c[:, 1] = -c[:, 1]
    return c


def _inner(model, z, u):
    """The squared invariant norm through the oracle's restatement of the manifold's inner."""
    if model == "upper":
        return so.upper_inner(_t(z), _t(u)).numpy()
    return so.bounded_inner(_t(z), _t(_conj(u))).numpy()


def _dist(model, z1, z2):
    return so.manifold_dist(model, _t(z1), _t(z2), "riem", check=False).numpy()


@pytest.mark.parametrize("n", eh.DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_hostsim_expmap_against_the_exact_values(model, n):
    z, u, want, kappa, k = eh.exp_inputs(eh.fixture(model, n))
    got, st = eh.hostsim_expmap(z, u, model)
    assert st == 0
    err = eh.row_err(got, want)
    ratio = err / (eh.EPS64 * kappa)
    print(f"{model} n={n}: expmap worst err / (eps kappa) per norm {[float(f'{ratio[k == j].max():.3g}') for j in range(4)]}, "
          f"worst err {err.max():.3e}")
    assert (err <= eh.exp_bound(model, kappa, k)).all(), (model, n, [float(ratio[k == j].max()) for j in range(4)])


@pytest.mark.parametrize("n", eh.DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_hostsim_logmap_against_the_exact_values(model, n):
    f = eh.fixture(model, n)
    got, st = eh.hostsim_logmap(f["z1"], f["z2"], model)
    assert st == 0
    err = eh.row_err(got, f["log"])
    ratio = err / (eh.EPS64 * eh.log_factor(f))
    print(f"{model} n={n}: logmap worst err / (eps factor) {ratio.max():.3g}, worst err {err.max():.3e}")
    assert (ratio <= eh.C_LOG[model]).all(), (model, n, float(ratio.max()))


@pytest.mark.parametrize("n", eh.DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_distance_identity_through_the_oracle(model, n):
    """oracle dist(x, expmap(x, u)) = c sqrt(inner).  Tolerance: 4 x the oracle's own worst error on the same identity at the exact
    100-digit points of the fixture (per norm of u), nothing taken from the code under test.  The norm 1e-8 is left to the exact
    comparison above: the oracle's distance has an absolute error ~1e-15 there."""
    f = eh.fixture(model, n)
    z, u, want, _, k = eh.exp_inputs(f)
    got, st = eh.hostsim_expmap(z, u, model)
    assert st == 0
    c = eh.DIST_SCALE[model]
    exact = c * f["unorm"].reshape(-1)
    own = np.abs(_dist(model, z, want) - exact) / exact            # the oracle on exact data
    mine = np.abs(_dist(model, z, got) - c * np.sqrt(_inner(model, z, u))) / exact
    for kk in (1, 2, 3):
        m = k == kk
        print(f"{model} n={n} |u| ~ {f['unorm'][0, kk]:.0e}: identity off by {mine[m].max():.2e}, the oracle's own error {own[m].max():.2e}")
        assert mine[m].max() <= 4.0 * own[m].max() + 4.0 * eh.EPS64, (model, n, kk)


@pytest.mark.parametrize("model", MODELS)
def test_bounded_inner_is_the_invariant_norm_at_conj_u(model):
    for n in (1, 2, 5):
        f = eh.fixture(model, n)
        z, u = eh.exp_inputs(f)[:2]
        exact = f["unorm"].reshape(-1)
        kap = np.repeat(f["kappa"], f["u"].shape[1])
        assert (np.abs(np.sqrt(_inner(model, z, u)) - exact) <= 64 * eh.EPS64 * kap * exact).all(), (model, n)
    if model == "bounded":      # the plain form is another quantity away from n = 1 / real points
        f = eh.fixture(model, 1)
        z, u = eh.exp_inputs(f)[:2]
        plain = np.sqrt(so.bounded_inner(_t(z), _t(u)).numpy())
        assert (np.abs(plain - f["unorm"].reshape(-1)) <= 64 * eh.EPS64 * np.repeat(f["kappa"], 4) * plain).all()
        f = eh.fixture(model, 3)
        z, u = eh.exp_inputs(f)[:2]
        plain = np.sqrt(so.bounded_inner(_t(z), _t(u)).numpy())
        assert (np.abs(plain - f["unorm"].reshape(-1)) / plain).max() > 1e-2


@pytest.mark.parametrize("n", eh.DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_round_trips(model, n):
    """log(exp(u)) = u and exp(log(y)) = y, in the unit of a composition of the two maps (tests/expmap_helpers.py) with the measured
    constants C_LOGEXP / C_EXPLOG.  The `far` pairs are left out of exp(log(y)) = y: with 1 - lambda down to 2e-8 the unit exceeds 1
    there and the check could not fail (their logarithm itself is pinned by test_hostsim_logmap_against_the_exact_values)."""
    f = eh.fixture(model, n)
    z, u, want, kappa, _ = eh.exp_inputs(f)
    ex, st = eh.hostsim_expmap(z, u, model)
    back, st2 = eh.hostsim_logmap(z, ex, model)
    assert st == 0 and st2 == 0
    ratio = eh.row_err(back, u) / eh.compose_unit(kappa * np.exp(2.0 * f["usigma"].reshape(-1)), want, u)
    print(f"{model} n={n}: log(exp(u)) = u worst err / unit {ratio.max():.3g}")
    assert (ratio <= eh.C_LOGEXP[model]).all(), (model, n, float(ratio.max()))
    keep = f["case"] != "far"
    z1, z2 = f["z1"][keep], f["z2"][keep]
    lg, st = eh.hostsim_logmap(z1, z2, model)
    y, st2 = eh.hostsim_expmap(z1, lg, model)
    assert st == 0 and st2 == 0
    unit = eh.compose_unit(eh.pair_condition(f)[keep], f["log"][keep], z2)
    assert (unit < 1e-3).all()          # a bound that can fail
    ratio = eh.row_err(y, z2) / unit
    print(f"{model} n={n}: exp(log(y)) = y worst err / unit {ratio.max():.3g}")
    assert (ratio <= eh.C_EXPLOG[model]).all(), (model, n, float(ratio.max()))


@pytest.mark.parametrize("model", MODELS)
def test_zero_tangent_and_equal_points_are_exact(model):
    for n in eh.DIMS:
        f = eh.fixture(model, n)
        z = f["z1"]
        ex, st = eh.hostsim_expmap(z, np.zeros_like(z), model)
        assert st == 0 and np.array_equal(ex, 0.5 * (z + z.transpose(0, 1, 3, 2))), (model, n)
        lg, st = eh.hostsim_logmap(z, z, model)
        assert st == 0 and not lg.any(), (model, n)


@pytest.mark.parametrize("model", MODELS)
def test_a_non_symmetric_tangent_gives_the_result_of_its_symmetric_part(model):
    rng = np.random.RandomState(3)
    for n in (2, 4, 7):
        z, u = eh.exp_inputs(eh.fixture(model, n))[:2]
        skew = rng.randn(*u.shape) * np.abs(u).reshape(len(u), -1).max(1)[:, None, None, None]
        skew = skew - skew.transpose(0, 1, 3, 2)
        a, st = eh.hostsim_expmap(z, u + skew, model)
        sym = 0.5 * ((u + skew) + (u + skew).transpose(0, 1, 3, 2))
        b, st2 = eh.hostsim_expmap(z, sym, model)
        assert st == 0 and st2 == 0 and np.array_equal(a, b), (model, n)


def _inside(model, x):
    """strictly inside the domain: Cholesky of Im x succeeds (upper) / spectral norm < 1 (bounded)."""
    for row in x:
        if model == "upper":
            np.linalg.cholesky(row[1])          # raises LinAlgError otherwise
        else:
            assert np.linalg.norm(row[0] + 1j * row[1], 2) < 1.0


@pytest.mark.parametrize("n", eh.DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_a_large_tangent_stays_strictly_inside_the_domain(model, n):
    f = eh.fixture(model, n)
    z, u = f["z1"], f["u"][:, 3]
    assert (f["unorm"][:, 3] > 5.9).all()
    ex, st = eh.hostsim_expmap(z, u, model)
    assert st == 0
    _inside(model, ex)


def _midpoint_check(model, n, f, keep, dist_fn, name):
    """|d(x, m) - d / 2| and |d(m, y) - d / 2| over d for m = expmap(x, logmap(x, y) / 2), against C_MID units of the composition
    plus the measuring distance's own error, taken as 4 x its error on the exact identity dist(z1, z2) = c |log| of the fixture."""
    z1, z2 = f["z1"][keep], f["z2"][keep]
    lg, st = eh.hostsim_logmap(z1, z2, model)
    mid, st2 = eh.hostsim_expmap(z1, 0.5 * lg, model)
    assert st == 0 and st2 == 0
    d = dist_fn(z1, z2)
    exact = eh.DIST_SCALE[model] * np.sqrt(_inner(model, z1, f["log"][keep]))
    own = (np.abs(d - exact) / exact).max()
    # (the midpoint is rounded to eps |x|, a length eps |x| / |log| of the distance it is measured in: the ratio of the unit)
    tol = 4.0 * own + eh.C_MID[model] * eh.compose_unit(eh.pair_condition(f)[keep], z2, f["log"][keep])
    a, b = np.abs(dist_fn(z1, mid) - 0.5 * d) / d, np.abs(dist_fn(mid, z2) - 0.5 * d) / d
    print(f"{model} n={n} {name}: |d(x,m) - d/2| / d <= {a.max():.2e}, |d(m,y) - d/2| / d <= {b.max():.2e}, worst over tol "
          f"{max((a / tol).max(), (b / tol).max()):.3g}, the distance's own error {own:.2e}")
    return a, b, tol


@pytest.mark.parametrize("n", (1, 2, 3, 5, 8))
@pytest.mark.parametrize("model", MODELS)
def test_the_midpoint_of_the_geodesic_is_equidistant(model, n):
    """geodesic(1/2, x, y) = expmap(x, logmap(x, y) / 2): at half the distance from both ends.  Every case but `far` (the clamp
    regime: the distance is clamped there) measured by the project's forward (g++ build of sympa::pair_distance, pinned to the
    50-digit values by tests/test_exact_reference.py); the cases with well separated singular values (`generic`) by the oracle
    as well.  The oracle does not measure the others: its route through torch.linalg.eigh is not dependable where singular values
    are close -- for bounded n = 3, cluster[0] (gap 1e-3, d = 0.57326) it returned 0.239 and 0.516 for the two halves when the 32
    fixture pairs were passed as one batch and the right 0.28663 (mpmath: 0.28663) when the pair was passed alone."""
    from tests.helpers import hostsim_dist
    f = eh.fixture(model, n)
    a, b, tol = _midpoint_check(model, n, f, f["case"] != "far", lambda p, q: hostsim_dist(p, q, model, "riem")[0], "forward")
    assert (a <= tol).all() and (b <= tol).all(), (model, n)
    a, b, tol = _midpoint_check(model, n, f, f["case"] == "generic", lambda p, q: _dist(model, p, q), "oracle")
    assert (a <= tol).all() and (b <= tol).all(), (model, n, "oracle")


@pytest.mark.parametrize("model", MODELS)
def test_the_geodesic_step_is_the_composition(model):
    """rsgd_exp_row = projx(expmap(x, -lr egrad2rgrad(x, g + wd x))) composed from the g++ builds of the separate rows
    (sympa::egrad2rgrad and sympa::projx through tests.helpers.hostsim_table): bit for bit at wd = 0 (with wd the row forms
    g + wd x in one fused multiply-add, numpy in two roundings), with the same rows counted as moved by the clamp."""
    from tests.helpers import hostsim_table
    rng = np.random.RandomState(11)
    for n in (1, 3, 6):
        z = eh.fixture(model, n)["z1"]
        g = rng.randn(*z.shape)
        g = g + g.transpose(0, 1, 3, 2)
        for lr in (1e-2, 0.3):
            got, moved, st = eh.hostsim_rsgd_exp(z, g, model, lr, 0.0)
            assert st == 0
            r, _ = hostsim_table("egrad2rgrad", model, z, g)
            ex, st = eh.hostsim_expmap(z, -lr * r, model)
            assert st == 0
            want, count = hostsim_table("projx", model, ex)
            assert np.array_equal(got, want), (model, n, lr)
            assert int(moved.sum()) == count, (model, n, lr)


def test_entries_validate_their_arguments_without_a_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(16)      # never dereferenced: validation happens before any launch
    D = ctypes.c_double
    bad_arg, bad_dims = _lib.DEFINES["SYMPA_ERR_BAD_ARG"], _lib.DEFINES["SYMPA_ERR_UNSUPPORTED_DIMS"]
    for entry in (lib.sympa_expmap, lib.sympa_logmap):
        assert entry(None, None, 0, 4, 0, None, None, None) == 0                   # b == 0 is a no-op
        assert entry(one, one, -1, 4, 0, one, None, None) == bad_arg
        assert entry(None, one, 3, 4, 0, one, None, None) == bad_arg
        assert entry(one, None, 3, 4, 1, one, None, None) == bad_arg
        assert entry(one, one, 3, 4, 1, None, None, None) == bad_arg
        for n in (0, 9, 16, -1):
            assert entry(one, one, 3, n, 0, one, None, None) == bad_dims, n
        for model in (2, 3, -1):                                                   # the compact dual and no model at all
            assert entry(one, one, 3, 4, model, one, None, None) == bad_arg, model
        assert b"inner product" in lib.sympa_last_error() or entry(one, one, 3, 4, 2, one, None, None) == bad_arg
    step = lib.sympa_rsgd_step_exp
    assert step(None, None, 0, 4, 0, D(1e-2), D(0.0), D(1e-5), None, None, None) == 0
    assert step(one, one, -1, 4, 0, D(1e-2), D(0.0), D(1e-5), None, None, None) == bad_arg
    assert step(None, one, 3, 4, 0, D(1e-2), D(0.0), D(1e-5), None, None, None) == bad_arg
    assert step(one, None, 3, 4, 1, D(1e-2), D(0.0), D(1e-5), None, None, None) == bad_arg
    assert step(one, one, 3, 4, 1, D(1e-2), D(0.0), D(0.0), None, None, None) == bad_arg          # eps must be > 0
    for n in (0, 9, 16):
        assert step(one, one, 3, n, 0, D(1e-2), D(0.0), D(1e-5), None, None, None) == bad_dims, n
    for model in (2, 3):
        assert step(one, one, 3, 4, model, D(1e-2), D(0.0), D(1e-5), None, None, None) == bad_arg, model


def _param(manifold, shape):
    from sympa_amd.manifolds.base import ManifoldParameter
    return ManifoldParameter(torch.zeros(*shape, dtype=torch.float64), manifold=manifold)


def test_rsgd_with_the_exponential_retraction_refuses_what_has_no_kernel():
    from sympa_amd.manifolds import BoundedDomainManifold, CompactDualManifold, UpperHalfManifold
    from sympa_amd.manifolds.spd import SymmetricPositiveDefinite
    from sympa_amd.manifolds.vector import PoincareBall
    from sympa_amd.optim import RiemannianSGD
    tables = {"dual": _param(CompactDualManifold(dims=3), (5, 2, 3, 3)),
              "spd": _param(SymmetricPositiveDefinite(), (5, 3, 3)),
              "vector": _param(PoincareBall(4), (5, 4)),
              "host table": _param(UpperHalfManifold(dims=3), (5, 2, 3, 3)),
              "host table, bounded": _param(BoundedDomainManifold(dims=3), (5, 2, 3, 3)),
              "dims 9": _param(UpperHalfManifold(dims=9), (5, 2, 9, 9))}
    for what, p in tables.items():
        with pytest.raises(NotImplementedError, match="retraction"):
            RiemannianSGD([p], lr=1e-2, retraction="exp")
        opt = RiemannianSGD([p], lr=1e-2)                       # the default is unchanged and takes every table
        assert opt.retraction == "linear", what
    with pytest.raises(ValueError):
        RiemannianSGD([tables["dual"]], lr=1e-2, retraction="cayley")
    # a parameter on no manifold (the scale) takes the Euclidean update either way
    assert RiemannianSGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-2, retraction="exp").retraction == "exp"


def test_the_fused_step_classes_refuse_the_exponential_retraction():
    from sympa_amd.optim import RiemannianSGD
    from sympa_amd.train_step import DistributedTrainStep, GraphedTrainStep
    opt = RiemannianSGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-2, retraction="exp")
    for cls in (GraphedTrainStep, DistributedTrainStep):
        with pytest.raises(NotImplementedError, match="linear retraction"):
            cls(None, opt, 8, 50.0, "cpu")


def test_the_manifold_surface():
    from sympa_amd.manifolds import BoundedDomainManifold, CompactDualManifold, UpperHalfManifold
    assert UpperHalfManifold(dims=3).dist_scale == 1.0 and BoundedDomainManifold(dims=3).dist_scale == 2.0
    x = torch.zeros(2, 2, 3, 3, dtype=torch.float64)
    dual = CompactDualManifold(dims=3)
    for call in (lambda: dual.expmap(x, x), lambda: dual.logmap(x, x), lambda: dual.geodesic(0.5, x, x), lambda: dual.dist_scale):
        with pytest.raises(NotImplementedError, match="inner product"):
            call()
    assert UpperHalfManifold(dims=9).dist_scale == 1.0 and BoundedDomainManifold(dims=16).dist_scale == 2.0     # no kernel involved
    big = UpperHalfManifold(dims=9)
    y = torch.zeros(2, 2, 9, 9, dtype=torch.float64)
    for call in (lambda: big.expmap(y, y), lambda: big.logmap(y, y), lambda: big.geodesic(0.5, y, y)):
        with pytest.raises(NotImplementedError, match="dims 1..8"):
            call()
    # the maps are kernels: a host tensor is refused, never computed some other way (and never answered with None)
    for man in (UpperHalfManifold(dims=3), BoundedDomainManifold(dims=3)):
        for call in (lambda: man.expmap(x, x), lambda: man.logmap(x, x), lambda: man.geodesic(0.5, x, x)):
            with pytest.raises(Exception) as e:
                call()
            assert not isinstance(e.value, NotImplementedError)
