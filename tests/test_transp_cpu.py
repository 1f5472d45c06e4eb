"""CPU: the parallel transport along geodesics of the upper and bounded models -- the g++ build of
sympa_amd/csrc/siegel_transp_math.hpp (tests/hostsim/hostsim_transp.cpp) against the 100-digit fixtures
tests/golden/exact_transp_*.npz, the properties that pin a transport, the argument validation of the C-ABI entries (no launch
happens) and the Python surface.  Bounds: tests/transp_helpers.py.

The property tests compose several rows.  Their unit is expmap_helpers.compose_unit with fac = kappa exp(2 sigma), the condition of
every point and map on the geodesic (sigma = the largest singular value of S), and their constant is the sum of the constants of
the rows composed -- each row errs by at most its own C eps (its condition), and the unit carries the first row's error through the
second.  A row is asserted when its whole tolerance, constant * unit, is below 1e-3 (above that the check could not fail: a vector
scaled by 1.001 must not pass); what is left is asserted to be most rows.  Worst err / (constant * unit) on the g++ build, upper /
bounded: (a) 0.043 / 0.084, (b) 0.010 / 0.084, (c) 0.013 / 0.0059, (d) 0.058 / 0.061, two points 0.0011 / 0.00038 (the
constants are sums of worst cases that do not occur together, and the unit squares the condition of the geodesic)."""
import ctypes

import numpy as np
import pytest
import torch

from sympa_amd import _lib
from tests import expmap_helpers as eh
from tests import transp_helpers as th

MODELS = ("upper", "bounded")


def _per_norm(r, k):
    return [float(f"{r[k == j].max():.3g}") for j in range(4)]


@pytest.mark.parametrize("n", th.DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_hostsim_transp_exp_against_the_exact_values(model, n):
    f = th.fixture(model, n)
    z, u, v, want, want_y, kappa, k = th.texp_inputs(f)
    got, st = th.hostsim_transp_exp(z, u, v, model)
    assert st == 0
    err = th.row_err(got, want)
    print(f"{model} n={n}: transp_exp g++ / exact, in eps kappa per norm {_per_norm(err / (th.EPS64 * kappa), k)}")
    assert (err <= th.texp_bound(model, kappa, k)).all(), _per_norm(err / (th.EPS64 * kappa), k)
    # the row that also produces y: the same v' bit for bit, and y under the exponential map's own bound
    y, got2, st = th.hostsim_expmap_transp(z, u, v, model)
    assert st == 0 and np.array_equal(got, got2)
    assert (th.row_err(y, want_y) <= eh.exp_bound(model, kappa, k)).all()


@pytest.mark.parametrize("n", th.DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_hostsim_transp_between_two_points_against_the_exact_values(model, n):
    f = th.fixture(model, n)
    got, st = th.hostsim_transp(f["z1"], f["z2"], f["v_pair"], model)
    assert st == 0
    err = th.row_err(got, f["transp"])
    print(f"{model} n={n}: transp g++ / exact, in eps kappa / (1 - lambda): {(err / th.t2_bound(model, f)).max() * th.C_T2[model]:.3g}")
    assert (err <= th.t2_bound(model, f)).all(), float((err / th.t2_bound(model, f)).max() * th.C_T2[model])


@pytest.mark.parametrize("model", MODELS)
def test_zero_tangent_and_equal_points_return_sym_v_bit_for_bit(model):
    rng = np.random.RandomState(5)
    for n in th.DIMS:
        f = th.fixture(model, n)
        z = f["z1"]
        v = f["v_pair"] + rng.randn(*z.shape)            # not symmetric
        got, st = th.hostsim_transp_exp(z, np.zeros_like(z), v, model)
        assert st == 0 and np.array_equal(got, th.sym(v)), (model, n)
        y, got, st = th.hostsim_expmap_transp(z, np.zeros_like(z), v, model)
        assert st == 0 and np.array_equal(got, th.sym(v)) and np.array_equal(y, th.sym(z)), (model, n)
        got, st = th.hostsim_transp(z, z, v, model)
        assert st == 0 and np.array_equal(got, th.sym(v)), (model, n)


@pytest.mark.parametrize("model", MODELS)
def test_non_symmetric_tangents_give_the_result_of_their_symmetric_parts(model):
    rng = np.random.RandomState(3)
    for n in (2, 4, 7):
        f = th.fixture(model, n)
        z, u, v = th.texp_inputs(f)[:3]
        su = rng.randn(*u.shape) * eh.amax(u)[:, None, None, None]
        su, sv = su - su.transpose(0, 1, 3, 2), rng.randn(*v.shape)
        sv = sv - sv.transpose(0, 1, 3, 2)
        a, st = th.hostsim_transp_exp(z, u + su, v + sv, model)
        b, st2 = th.hostsim_transp_exp(z, th.sym(u + su), th.sym(v + sv), model)
        assert st == 0 and st2 == 0 and np.array_equal(a, b), (model, n)
        vp = f["v_pair"] + sv[::4]
        a, st = th.hostsim_transp(f["z1"], f["z2"], vp, model)
        b, st2 = th.hostsim_transp(f["z1"], f["z2"], th.sym(vp), model)
        assert st == 0 and st2 == 0 and np.array_equal(a, b), (model, n)


def _checked(name, model, n, err, unit, const):
    """err <= const * unit on the rows whose tolerance const * unit is a bound that can fail (module docstring)."""
    tol = const * unit
    keep = tol < 1e-3
    assert keep.mean() > 0.5, (name, model, n, float(keep.mean()))
    worst = (err[keep] / tol[keep]).max()
    print(f"{model} n={n}: {name}: worst err / (constant * unit) {worst:.3g} over {int(keep.sum())} of {len(keep)} rows, "
          f"largest tolerance {tol[keep].max():.2e}")
    assert worst <= 1.0, (name, model, n, float(worst))


@pytest.mark.parametrize("n", th.DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_the_properties_that_pin_a_transport(model, n):
    """(a) the invariant inner product is preserved (polarised with a second vector);  (b) transp_exp(x, u, u) = -logmap(y, x);
    (c) the transport back along the reversed velocity returns v;  (d) two half steps equal the whole one (against the exact value).
    (a)-(c) leave a rotation about the velocity free, (d) does not."""
    f = th.fixture(model, n)
    z, u, v, want, want_y, kappa, k = th.texp_inputs(f)
    fac = kappa * np.exp(2.0 * f["usigma"].reshape(-1))
    c_t, c_e = np.asarray(th.C_TEXP[model])[k], np.asarray(eh.C_EXP[model])[k]
    rng = np.random.RandomState(17 + n)
    v2 = th.sym(rng.randn(*v.shape))
    y, tv, st = th.hostsim_expmap_transp(z, u, v, model)
    tv2, st2 = th.hostsim_transp_exp(z, u, v2, model)
    tu, st3 = th.hostsim_transp_exp(z, u, u, model)
    assert st == 0 and st2 == 0 and st3 == 0
    # (a) in units of |v| |v2|; both inner products are numpy's (two inverses of a matrix of condition <= fac: 8 n eps fac each)
    scale = np.sqrt(th.invariant_inner(model, z, v, v) * th.invariant_inner(model, z, v2, v2))
    for w2 in (tv2, np.stack((-tv2[:, 1], tv2[:, 0]), 1)):                       # v2 and i v2: the complex trace
        w0 = v2 if w2 is tv2 else np.stack((-v2[:, 1], v2[:, 0]), 1)
        d = np.abs(th.invariant_inner(model, y, tv, w2) - th.invariant_inner(model, z, v, w0)) / scale
        _checked("(a) inner product", model, n, d, th.compose_unit(fac, v, v), 2.0 * c_t + c_e + 16.0 * n)
    # (b)
    back, st = eh.hostsim_logmap(y, z, model)
    assert st == 0
    _checked("(b) velocity", model, n, th.row_err(tu, -back), th.compose_unit(fac, want_y, u), c_t + c_e + eh.C_LOG[model])
    # (c)
    rv, st = th.hostsim_transp_exp(y, -tu, tv, model)
    assert st == 0
    _checked("(c) there and back", model, n, th.row_err(rv, th.sym(v)), th.compose_unit(fac, want, v), c_e + 3.0 * c_t)
    # (d)
    yh, th_, st = th.hostsim_expmap_transp(z, 0.5 * u, v, model)
    uh, st2 = th.hostsim_transp_exp(z, 0.5 * u, 0.5 * u, model)
    got, st3 = th.hostsim_transp_exp(yh, uh, th_, model)
    assert st == 0 and st2 == 0 and st3 == 0
    _checked("(d) semigroup", model, n, th.row_err(got, want), th.compose_unit(fac, v, want), c_e + 3.0 * c_t)


@pytest.mark.parametrize("model", MODELS)
def test_the_two_point_form_is_the_tangent_form_at_the_logarithm(model):
    """transp(x, y, v) (the exact value) against transp_exp(x, logmap(x, y), v): the logarithm's constant plus the transport's at
    the norm of that logarithm (k = the first of 1e-8, 1e-3, 1, 6 that is not below it), times the composition's unit; asserted
    where that tolerance is below 1e-3, which leaves out `far` (1 - lambda down to 2e-8) and keeps most other pairs."""
    for n in (1, 3, 6):
        f = th.fixture(model, n)
        lg, st = eh.hostsim_logmap(f["z1"], f["z2"], model)
        a, st2 = th.hostsim_transp_exp(f["z1"], lg, f["v_pair"], model)
        assert st == 0 and st2 == 0
        norm = np.sqrt(th.invariant_inner(model, f["z1"], f["log"], f["log"]))
        k = np.minimum(np.searchsorted(np.array([1e-8, 1e-3, 1.0, 6.0]) * (1.0 + 1e-6), norm), 3)
        unit = th.compose_unit(eh.pair_condition(f), f["log"], f["transp"])
        _checked("two points", model, n, th.row_err(a, f["transp"]), unit, eh.C_LOG[model] + np.asarray(th.C_TEXP[model])[k])


def test_a_tangent_too_long_for_tanh_sets_the_status_word():
    for model in MODELS:
        f = th.fixture(model, 3)
        keep = f["case"] == "generic"
        z, u, v = f["z1"][keep], f["u"][keep][:, 2] * 100.0, f["v_pair"][keep]     # invariant length 100
        _, st = th.hostsim_transp_exp(z, u, v, model)
        assert st != 0, model


def test_entries_validate_their_arguments_without_a_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(16)      # never dereferenced: validation happens before any launch
    bad_arg, bad_dims = _lib.DEFINES["SYMPA_ERR_BAD_ARG"], _lib.DEFINES["SYMPA_ERR_UNSUPPORTED_DIMS"]
    te, t2 = lib.sympa_transp_exp, lib.sympa_transp
    for out_y in (None, one):
        assert te(None, None, None, 0, 4, 0, None, None, None, None) == 0                      # b == 0 is a no-op
        assert te(one, one, one, -1, 4, 0, out_y, one, None, None) == bad_arg
        for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
            assert te(args[0], args[1], args[2], 3, 4, 1, out_y, args[3], None, None) == bad_arg
            assert b"null buffer" in lib.sympa_last_error()
        for n in (0, 9, 16, -1):
            assert te(one, one, one, 3, n, 0, out_y, one, None, None) == bad_dims, n
        assert te(one, one, one, 3, 4, 2, out_y, one, None, None) == bad_arg
        assert b"inner product" in lib.sympa_last_error()
        for model in (3, -1):
            assert te(one, one, one, 3, 4, model, out_y, one, None, None) == bad_arg, model
            assert b"unknown model" in lib.sympa_last_error()
        assert te(one, one, one, (1 << 31) * 64, 4, 0, out_y, one, None, None) == bad_arg
        assert b"too many rows" in lib.sympa_last_error()
    assert t2(None, None, None, 0, 4, 0, None, None, None) == 0
    assert t2(one, one, one, -1, 4, 0, one, None, None) == bad_arg
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        assert t2(args[0], args[1], args[2], 3, 4, 1, args[3], None, None) == bad_arg
    for n in (0, 9, 16, -1):
        assert t2(one, one, one, 3, n, 0, one, None, None) == bad_dims, n
    assert t2(one, one, one, 3, 4, 2, one, None, None) == bad_arg
    assert b"inner product" in lib.sympa_last_error()
    for model in (3, -1):
        assert t2(one, one, one, 3, 4, model, one, None, None) == bad_arg, model
    assert t2(one, one, one, (1 << 31) * 64, 4, 1, one, None, None) == bad_arg


def test_transp_is_still_the_identity():
    from sympa_amd.manifolds import BoundedDomainManifold, CompactDualManifold, UpperHalfManifold
    x = torch.randn(3, 2, 4, 4, dtype=torch.float64)
    for man in (UpperHalfManifold(dims=4), BoundedDomainManifold(dims=4), CompactDualManifold(dims=4)):
        v = torch.randn(3, 2, 4, 4, dtype=torch.float64)
        assert man.transp(x, x + 1.0, v) is v


def test_the_python_surface_refuses_what_has_no_kernel():
    from sympa_amd import ops
    from sympa_amd.manifolds import BoundedDomainManifold, CompactDualManifold, UpperHalfManifold
    x = torch.zeros(2, 2, 3, 3, dtype=torch.float64)
    dual = CompactDualManifold(dims=3)
    for call in (lambda: dual.transp_follow_expmap(x, x, x), lambda: dual.expmap_transp(x, x, x),
                 lambda: dual.parallel_transport(x, x, x), lambda: dual.invariant_inner(x, x, x)):
        with pytest.raises(NotImplementedError, match="inner product"):
            call()
    big = UpperHalfManifold(dims=9)
    y = torch.zeros(2, 2, 9, 9, dtype=torch.float64)
    for call in (lambda: big.transp_follow_expmap(y, y, y), lambda: big.expmap_transp(y, y, y), lambda: big.parallel_transport(y, y, y)):
        with pytest.raises(NotImplementedError, match="dims 1..8"):
            call()
    # kernels only: a host tensor is refused, never computed some other way
    for man in (UpperHalfManifold(dims=3), BoundedDomainManifold(dims=3)):
        for call in (lambda: man.transp_follow_expmap(x, x, x), lambda: man.expmap_transp(x, x, x),
                     lambda: man.parallel_transport(x, x, x)):
            with pytest.raises(_lib.SympaHipError, match="GPU only"):
                call()
    for call in (lambda: ops.transp_exp(x, x, x, "upper"), lambda: ops.transp(x, x, x, "bounded")):
        with pytest.raises(_lib.SympaHipError, match="GPU only"):
            call()


def test_float32_is_refused_by_its_dtype(monkeypatch):
    """The device check comes first, so a float32 host tensor never reaches the dtype check; with the device check out of the way
    the dtype check is what refuses (on the GPU itself: tests/test_transp_gpu.py)."""
    from sympa_amd import ops
    monkeypatch.setattr(ops, "_need_gpu", lambda t, name: None)
    xs = torch.zeros(2, 2, 3, 3, dtype=torch.float32)
    for call in (lambda: ops.transp_exp(xs, xs, xs, "upper"), lambda: ops.transp(xs, xs, xs, "bounded")):
        with pytest.raises(ValueError, match="float64"):
            call()


def test_invariant_inner():
    """`inner` for the upper model; for the bounded model the form of the fixtures' norm, |u|^2 = unorm^2, which the reference's
    bounded inner is not (tests/test_expmap_cpu.py)."""
    from sympa_amd.manifolds import BoundedDomainManifold, UpperHalfManifold
    for model, cls in (("upper", UpperHalfManifold), ("bounded", BoundedDomainManifold)):
        f = eh.fixture(model, 3)
        z, u = eh.exp_inputs(f)[:2]
        man = cls(dims=3)
        zt, ut = torch.from_numpy(np.array(z)), torch.from_numpy(np.array(u))
        got = man.invariant_inner(zt, ut)
        assert got.shape == man.inner(zt, ut).shape
        norm = got[:, 0, 0, 0].sqrt().numpy()
        want = f["unorm"].reshape(-1)
        assert (np.abs(norm - want) <= 64 * eh.EPS64 * np.repeat(f["kappa"], 4) * want).all(), model
        if model == "upper":
            assert torch.equal(got, man.inner(zt, ut))
        v = torch.from_numpy(np.array(th.texp_inputs(th.fixture(model, 3))[2]))
        pol = man.invariant_inner(zt, ut, v)[:, 0, 0, 0].numpy()
        assert np.allclose(pol, th.invariant_inner(model, z, u, v.numpy()), rtol=1e-9, atol=0)
