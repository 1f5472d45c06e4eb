"""CPU: the geodesic RiemannianAdam step of the upper and bounded models -- the g++ build of
sympa_amd/csrc/siegel_radam_exp_math.hpp (tests/hostsim/hostsim_radam_exp.cpp) against the 100-digit fixtures
tests/golden/exact_radam_exp_*.npz, the three properties the generator asserts, the exact cases, the argument validation of the
C-ABI entry (no launch happens) and the Python surface.  Bounds: tests/radam_exp_helpers.py.

The property tests compose several rows.  Their unit is expmap_helpers.compose_unit with fac = kappa exp(2 |u|_x), the condition of
every point and map on the step's geodesic, and their constant is the sum of the constants of the rows composed, as in
tests/test_transp_cpu.py.  Every fixture row is asserted (kappa <= 1e6 by the fixture's design keeps every tolerance a bound that
can fail, below 1e-3), and the tests assert that they covered every row."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from oracle import siegel_oracle as so
from sympa_amd import _lib
from tests import expmap_helpers as eh
from tests import radam_exp_helpers as rh
from tests import transp_helpers as th

TOOLS = os.path.join(rh.ROOT, "tools")


@pytest.mark.parametrize("n", rh.DIMS)
@pytest.mark.parametrize("model", rh.MODELS)
def test_hostsim_against_the_exact_values(model, n):
    f = rh.fixture(model, n)
    rows = 0
    for c in rh.cases(f):
        y, m, s, moved, st = rh.run_case(c, model)
        assert st == 0 and moved == 0, (model, n, c["st"], c["k"], st, moved)      # projx idle on every stored row
        err = rh.errors(y, m, s, c["y"], c["m_out"], c["s1"])
        for o in rh.OUTPUTS:
            units = err[o] / (rh.EPS64 * c["kappa"])
            print(f"{model} n={n} state {c['st']} lr {c['lr']:g}: {o} g++ / exact, in eps kappa {units.max():.3g}")
            assert (err[o] <= rh.bound(model, o, c["k"], c["kappa"])).all(), (o, c["st"], c["k"], float(units.max()))
        rows += len(c["kappa"])
    assert rows == f["x"].shape[0] * 6 and f["x"].shape[0] >= 4 and (f["kappa"] <= 1e6).all()


def _checked(name, model, n, err, unit, const, covered):
    tol = const * unit
    assert (tol < 1e-3).all(), (name, model, n, float(tol.max()))      # every row: a bound that can fail
    worst = (err / tol).max()
    print(f"{model} n={n}: {name}: worst err / (constant * unit) {worst:.3g}, largest tolerance {tol.max():.2e}")
    assert worst <= 1.0, (name, model, n, float(worst))
    covered.append(len(err))


def _dist(model, z1, z2):
    t = lambda a: torch.from_numpy(np.array(a))
    return so.manifold_dist(model, t(z1), t(z2), "riem", check=False).numpy() / rh.DIST_SCALE[model]


@pytest.mark.parametrize("n", rh.DIMS)
@pytest.mark.parametrize("model", rh.MODELS)
def test_the_properties_the_generator_asserts(model, n):
    """(a) the invariant norm of exp_avg is preserved by the transport;  (b) exp_avg <- logmap(y, x) / alpha, the velocity's
    transport (g++ logmap_pair, the exact alpha);  (c) a first step without weight decay has the invariant length
    lr |g|_x / (|g|_x + eps_adam), measured by the oracle's distance over dist_scale: its tolerance adds 4 x the oracle's own
    error on the exact y of the same row."""
    f = rh.fixture(model, n)
    a_rows, b_rows, c_rows = [], [], []
    for c in rh.cases(f):
        y, m, s, moved, st = rh.run_case(c, model)
        m1 = rh.hostsim_radam_exp(c["x"], c["grad"], c["m"], c["s"], model, 0.0, c["betas"], c["eps_adam"], c["wd"], c["pow1"],
                                  c["pow2"])[1]                                     # lr = 0 returns m1 (the exact cases below)
        assert st == 0
        fac = rh.geodesic_condition(c)
        k = c["k"]
        c_y, c_m = rh.C_RADAM[model]["y"][k], rh.C_RADAM[model]["m"][k]
        u = -c["alpha"][:, None, None, None] * m1
        # (a) two numpy inner products, each two inverses of a matrix of condition <= fac: 8 n eps fac each
        before, after = th.invariant_inner(model, c["x"], m1, m1), th.invariant_inner(model, y, m, m)
        _checked("(a) norm of exp_avg", model, n, np.abs(after - before) / before, rh.compose_unit(fac, m1, m1),
                 2.0 * c_m + c_y + 16.0 * n, a_rows)
        # (b)
        back, st = eh.hostsim_logmap(y, c["x"], model)
        assert st == 0
        _checked("(b) velocity", model, n, rh.row_err(m, back / c["alpha"][:, None, None, None]), rh.compose_unit(fac, c["y"], u),
                 c_m + c_y + rh.C_LOG[model], b_rows)
        # (c)
        if c["st"] == 0 and c["wd"] == 0.0:
            gx = np.sqrt(c["s1"] / (1.0 - c["betas"][1]))
            exact = c["lr"] * gx / (gx + c["eps_adam"])
            own = np.abs(_dist(model, c["x"], c["y"]) - exact) / exact
            mine = np.abs(_dist(model, c["x"], y) - exact) / exact
            tol = 4.0 * own + 4.0 * rh.EPS64 + c_y * rh.compose_unit(fac, c["y"], u)
            print(f"{model} n={n} lr {c['lr']:g}: (c) unit step off by {mine.max():.2e}, the oracle's own error {own.max():.2e}")
            assert (tol < 1e-3).all() and (mine <= tol).all(), (model, n, k, float((mine / tol).max()))
            c_rows.append(len(mine))
    p = f["x"].shape[0]
    assert sum(a_rows) == 6 * p and sum(b_rows) == 6 * p and sum(c_rows) == 2 * p


@pytest.mark.parametrize("model", rh.MODELS)
def test_zero_gradient_on_zero_moments_returns_sym_x_bit_for_bit(model):
    rng = np.random.RandomState(7)
    for n in rh.DIMS:
        f = rh.fixture(model, n)
        x = f["x"] + 1e-3 * rng.randn(*f["x"].shape)             # not symmetric
        zero = np.zeros_like(x)
        for lr, wd_free_pows in ((1e-3, (0.9, 0.999)), (1.0, (0.9 ** 5, 0.999 ** 5))):
            y, m, s, moved, st = rh.hostsim_radam_exp(x, zero, zero, np.zeros(len(x)), model, lr, (0.9, 0.999), 1e-7, 0.0,
                                                      *wd_free_pows)
            assert st == 0 and moved == 0, (model, n)
            assert np.array_equal(y, th.sym(x)) and np.array_equal(m, zero) and np.array_equal(s, np.zeros(len(x))), (model, n)


@pytest.mark.parametrize("model", rh.MODELS)
def test_lr_zero_returns_sym_x_and_m1_bit_for_bit(model):
    """lr = 0: alpha = 0, u = 0, the short form of the transport returns its argument m1.  m1 itself has no second bit-exact
    route in Python, so: the output is exactly symmetric, the same bits whatever alpha's other factors are (pow1, pow2, eps_adam),
    left unchanged by the g++ transport along a zero tangent, and equal to numpy's m1 to the rounding of its two products."""
    rng = np.random.RandomState(11)
    for n in rh.DIMS:
        f = rh.fixture(model, n)
        x = f["x"] + 1e-3 * rng.randn(*f["x"].shape)
        for c in rh.cases(f):
            if c["k"] != 1:
                continue
            args = (x, c["grad"], c["m"], c["s"], model, 0.0, c["betas"], c["eps_adam"], c["wd"])
            y, m, s, moved, st = rh.hostsim_radam_exp(*args, c["pow1"], c["pow2"])
            assert st == 0 and moved == 0 and np.array_equal(y, th.sym(x)), (model, n)
            assert np.array_equal(m, m.transpose(0, 1, 3, 2))
            m2 = rh.hostsim_radam_exp(x, c["grad"], c["m"], c["s"], model, 0.0, c["betas"], 1e-3, c["wd"], 0.5, 0.25)[1]
            assert np.array_equal(m, m2)
            again, st = th.hostsim_transp_exp(x, np.zeros_like(x), m, model)
            assert st == 0 and np.array_equal(again, m)
            # numpy's m1
            xc, gc = th.cplx(x), th.cplx(c["grad"]) + c["wd"] * th.cplx(x)
            if model == "upper":
                r = xc.imag @ gc @ xc.imag
            else:
                a = np.eye(n) - xc.conj() @ xc
                r = a @ gc @ a
            r = 0.5 * (r + r.transpose(0, 2, 1))
            want = c["betas"][0] * th.cplx(th.sym(c["m"])) + (1.0 - c["betas"][0]) * r
            want = np.stack((want.real, want.imag), 1)
            assert (rh.row_err(m, want) <= 16.0 * n * rh.EPS64).all(), (model, n, float(rh.row_err(m, want).max()))


@pytest.mark.parametrize("model", rh.MODELS)
def test_a_non_symmetric_exp_avg_gives_the_bits_of_its_symmetric_part(model):
    rng = np.random.RandomState(13)
    for n in (1, 2, 4, 7):
        f = rh.fixture(model, n)
        for c in rh.cases(f):
            if c["st"] != 1:
                continue
            skew = rng.randn(*c["m"].shape) * eh.amax(c["m"])[:, None, None, None]
            m_ns = c["m"] + skew - skew.transpose(0, 1, 3, 2)
            args = (c["s"], model, c["lr"], c["betas"], c["eps_adam"], c["wd"], c["pow1"], c["pow2"])
            a = rh.hostsim_radam_exp(c["x"], c["grad"], m_ns, *args)
            b = rh.hostsim_radam_exp(c["x"], c["grad"], th.sym(m_ns), *args)
            assert a[4] == 0 and b[4] == 0
            assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])), (model, n, c["k"])


def test_the_clip_factor_scales_the_gradient_as_it_is_read():
    for model in rh.MODELS:
        f = rh.fixture(model, 3)
        c = next(c for c in rh.cases(f) if c["st"] == 1 and c["k"] == 1)
        args = (c["m"], c["s"], model, c["lr"], c["betas"], c["eps_adam"], c["wd"], c["pow1"], c["pow2"])
        a = rh.hostsim_radam_exp(c["x"], c["grad"], *args, coef=0.25)          # a power of two: the product is exact
        b = rh.hostsim_radam_exp(c["x"], 0.25 * c["grad"], *args)
        assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3])), model


def test_the_header_declares_the_entry():
    assert "sympa_radam_step_exp" in _lib.SYMBOLS
    restype, types = _lib.PROTOTYPES["sympa_radam_step_exp"]
    assert restype is ctypes.c_int and len(types) == 19
    names = list(_lib.SYMBOLS)
    assert names.index("sympa_radam_step_exp") == names.index("sympa_rsgd_step_exp") + 1
    d, p = ctypes.c_double, ctypes.c_void_p
    assert types == [p, p, p, p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, d, d, d, d, d, p, d, p, d, p, p, p]


def test_the_entry_validates_its_arguments_without_a_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(16)      # never dereferenced: validation happens before any launch
    bad_arg, bad_dims = _lib.DEFINES["SYMPA_ERR_BAD_ARG"], _lib.DEFINES["SYMPA_ERR_UNSUPPORTED_DIMS"]
    step = lib.sympa_radam_step_exp

    def call(rows=3, n=4, model=0, bufs=(one, one, one, one), pows=one, eps=1e-5, clip=None, max_norm=0.0):
        return step(bufs[0], bufs[1], bufs[2], bufs[3], rows, n, model, 1e-2, 0.9, 0.999, 1e-7, 0.0, pows, eps, clip, max_norm, None,
                    None, None)

    assert call(rows=0, bufs=(None, None, None, None), pows=None) == 0               # no rows: no launch
    assert call(rows=-1) == bad_arg
    assert call(model=_lib.DEFINES["SYMPA_MODEL_DUAL"]) == bad_arg and b"inner product" in lib.sympa_last_error()
    assert call(model=_lib.DEFINES["SYMPA_MODEL_DUAL"], n=9) == bad_arg               # the model is looked at first
    for model in (3, -1):
        assert call(model=model) == bad_arg and b"unknown model" in lib.sympa_last_error()
    for n in (0, 9, 16, -1):
        assert call(n=n) == bad_dims, n
        assert call(n=n, rows=0) == bad_dims, n
    assert call(eps=0.0) == bad_arg
    assert call(clip=one, max_norm=0.0) == bad_arg and b"max_norm" in lib.sympa_last_error()
    for i in range(4):
        bufs = [one] * 4
        bufs[i] = None
        assert call(bufs=tuple(bufs)) == bad_arg and b"null buffer" in lib.sympa_last_error()
    assert call(pows=None) == bad_arg and b"null buffer" in lib.sympa_last_error()
    assert call(rows=(1 << 31) * 64) == bad_arg and b"too many rows" in lib.sympa_last_error()


def _param(manifold, shape):
    from sympa_amd.manifolds.base import ManifoldParameter
    return ManifoldParameter(torch.zeros(*shape, dtype=torch.float64), manifold=manifold)


def test_radam_with_the_exponential_retraction_refuses_what_has_no_kernel():
    from sympa_amd.manifolds import BoundedDomainManifold, CompactDualManifold, UpperHalfManifold
    from sympa_amd.manifolds.spd import SymmetricPositiveDefinite
    from sympa_amd.manifolds.vector import PoincareBall
    from sympa_amd.optim import RiemannianAdam, RiemannianSGD
    tables = {"dual": _param(CompactDualManifold(dims=3), (5, 2, 3, 3)),
              "spd": _param(SymmetricPositiveDefinite(), (5, 3, 3)),
              "vector": _param(PoincareBall(4), (5, 4)),
              "host table": _param(UpperHalfManifold(dims=3), (5, 2, 3, 3)),
              "host table, bounded": _param(BoundedDomainManifold(dims=3), (5, 2, 3, 3)),
              "dims 9": _param(UpperHalfManifold(dims=9), (5, 2, 9, 9))}
    for what, p in tables.items():
        with pytest.raises(NotImplementedError, match="retraction='linear'"):
            RiemannianAdam([p], lr=1e-2, retraction="exp")
        if what != "dual":                                      # (RiemannianAdam has no dual model at all)
            assert RiemannianAdam([p], lr=1e-2).retraction == "linear", what
    with pytest.raises(ValueError, match="retraction"):
        RiemannianAdam([tables["spd"]], lr=1e-2, retraction="cayley")
    # a parameter on no manifold takes the ordinary Adam update either way
    scale = torch.nn.Parameter(torch.ones(1, dtype=torch.float64))
    opt = RiemannianAdam([scale], lr=1e-2, retraction="exp")
    assert opt.retraction == "exp"
    scale.grad = torch.ones(1, dtype=torch.float64)
    opt.step()
    assert abs(float(scale.detach()) - (1.0 - 1e-2)) < 1e-6
    # a table that turns up after construction is refused by step()
    opt.add_param_group({"params": [tables["host table"]]})
    tables["host table"].grad = torch.zeros_like(tables["host table"])
    with pytest.raises(NotImplementedError, match="retraction='linear'"):
        opt.step()
    # one function serves both optimisers
    from sympa_amd import optim
    assert RiemannianSGD._check_exp_table is optim._check_exp_table


def test_the_fused_step_classes_refuse_the_optimiser():
    from sympa_amd.optim import RiemannianAdam
    from sympa_amd.train_step import DistributedTrainStep, GraphedTrainStep
    opt = RiemannianAdam([torch.nn.Parameter(torch.zeros(1))], lr=1e-2, retraction="exp")
    for cls in (GraphedTrainStep, DistributedTrainStep):
        with pytest.raises(NotImplementedError, match="linear retraction"):
            cls(None, opt, 8, 50.0, "cpu")


def test_ops_refuses_what_has_no_kernel():
    from sympa_amd import ops
    x = torch.zeros(3, 2, 3, 3, dtype=torch.float64)
    with pytest.raises(_lib.SympaHipError, match="GPU only"):
        ops.radam_step_exp_(x, x, x.clone(), torch.zeros(3, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), "upper", 1e-2,
                            (0.9, 0.999), 1e-7, 0.0)


def test_train_siegel_parses_radam_with_the_exponential_retraction():
    sys.path.insert(0, TOOLS)
    try:
        import train_siegel
    finally:
        sys.path.remove(TOOLS)
    a = train_siegel.parser().parse_args(["--optim", "radam", "--retraction", "exp"])
    assert a.optim == "radam" and a.retraction == "exp"      # (the run itself: tests/test_radam_exp_gpu.py)
