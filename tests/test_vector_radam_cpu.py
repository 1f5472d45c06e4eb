"""CPU (`-m "not gpu"`): the vector models' RiemannianAdam row (sympa_amd/csrc/vector_math.hpp, built with g++ as
tests/hostsim/hostsim_vector_radam.cpp) against the 50-digit fixtures of tools/make_golden_vector_radam_exact.py within the
bounds of tests/vector_radam_helpers.py, for every lane count; the manifold's transp / inner / component_inner in torch; the
C-ABI's argument checks; the refusal of a table on the host."""
import ctypes

import numpy as np
import pytest
import torch

from tests import vector_helpers as vh
from tests import vector_radam_helpers as rh

EPS = vh.EPS64


def _pows(fx):
    return fx["pows_prev"] * np.array(rh.BETAS)


@pytest.mark.parametrize("model", vh.MODELS)
def test_hostsim_matches_every_fixture_for_every_lane_count(model):
    tally = vh.Tally()
    for dims in rh.dims_of(model):
        for state in rh.STATES:
            fx = rh.radam_fixture(model, dims, state)
            for lr, wd in rh.SETTINGS:
                want = fx[rh.setting_key(lr, wd)]
                for G in vh.LANES:
                    x, m, s, moved, st = rh.hostsim_radam(fx["x"], fx["g"], fx["m"], fx["s"], model, lr, wd, _pows(fx), G=G)
                    label = f"{model} dims {dims} {state} lr {lr} wd {wd} G={G}"
                    assert st == 0, label
                    rh.check_radam(tally, model, dims, want, x, m, s, label)
                    assert moved == int(want["moved"].sum()), label
                # the kernel's own lane count is one of them
                own = rh.hostsim_radam(fx["x"], fx["g"], fx["m"], fx["s"], model, lr, wd, _pows(fx))
                ref = rh.hostsim_radam(fx["x"], fx["g"], fx["m"], fx["s"], model, lr, wd, _pows(fx),
                                       G=vh.hostsim_vector().sympa_hostsim_vector_lanes(dims))
                assert all(np.array_equal(a, b) for a, b in zip(own[:3], ref[:3]))
    tally.report(f"hostsim radam {model}")


@pytest.mark.parametrize("model", vh.MODELS)
def test_the_fixtures_cover_what_they_are_there_for(model):
    f = vh.FACTORS[model]
    for dims in rh.dims_of(model):
        later = rh.radam_fixture(model, dims, "later")[rh.setting_key(1.0, 0.0)]
        if "P" in f:
            assert later["moved"].any(), (model, dims)                # lr = 1 makes a Poincare row leave the ball
        if "L" in f:
            assert (later["nu"] > 1.0).all(), (model, dims)           # and gives the L rows a step length above 1
        for state in rh.STATES:
            fx = rh.radam_fixture(model, dims, state)
            assert not fx[rh.setting_key(0.01, 0.0)]["moved"].any() and not fx[rh.setting_key(0.01, 0.1)]["moved"].any()
    if len(f) == 2:
        assert set(rh.EXTRA_DIMS) <= set(rh.dims_of(model))


def test_zero_gradient_and_zero_state_stay_zero():
    for model in vh.MODELS:
        fx = rh.radam_fixture(model, 8, "first")
        z = np.zeros_like(fx["x"])
        x, m, s, moved, st = rh.hostsim_radam(fx["x"], z, z, z, model, 1.0, 0.0, rh.BETAS)
        assert st == 0 and moved == 0 and (m == 0).all() and (s == 0).all() and np.isfinite(x).all(), model
        assert np.abs(x - fx["x"]).max() <= 4 * EPS * np.abs(fx["x"]).max(), model


def test_non_finite_gradient_sets_the_status_bit():
    fx = rh.radam_fixture("prod-hyeu", 8, "later")
    g = fx["g"].copy()
    g[3, 6] = np.nan
    *_, st = rh.hostsim_radam(fx["x"], g, fx["m"], fx["s"], "prod-hyeu", 0.01, 0.0, _pows(fx))
    assert st & 2                                                    # SYMPA_ST_NONFINITE


def test_euclidean_row_is_adam():
    for dims in (1, 5, 16, 65):
        for state in rh.STATES:
            fx = rh.radam_fixture("euclidean", dims, state)
            p1, p2 = _pows(fx)
            b1, b2 = rh.BETAS
            for lr, wd in rh.SETTINGS:
                g = fx["g"] + wd * fx["x"]
                m1 = b1 * fx["m"] + (1 - b1) * g
                s1 = b2 * fx["s"] + (1 - b2) * g * g
                y = fx["x"] - lr * (m1 / (1 - p1)) / (np.sqrt(s1 / (1 - p2)) + rh.EPS_ADAM)
                x, m, s, _, _ = rh.hostsim_radam(fx["x"], fx["g"], fx["m"], fx["s"], "euclidean", lr, wd, (p1, p2))
                # (8 eps of the row's largest value; for x' = x + u that includes x itself: at lr = 1 a step can cancel most of x, and
                # the two routes round u, whose size is up to |x| + |x'|, differently)
                for got, want, size in ((x, y, np.maximum(np.abs(y), np.abs(fx["x"]))), (m, m1, np.abs(m1)), (s, s1, np.abs(s1))):
                    assert (np.abs(got - want) <= 8 * EPS * size.max(1, keepdims=True)).all(), (dims, state, lr, wd)


@pytest.mark.parametrize("model", vh.MODELS)
def test_torch_transport_and_inner(model):
    """VectorManifold.transp / inner / component_inner on the fixture points: the transport is tangent at y (S, L), keeps
    I(y, T w) = I(x, w) (E, P, L; the S transport is a projection and loses <y, w>^2), and is the identity for y = x.  Tolerances: the inner products are sums of m terms, so each side carries
    (m + 8) eps sum |terms|; the transported vector carries the kappa `km` of the fixture row (the conditioning of the same
    closed forms), and I is quadratic in it: 4 (m + C_RADAM_EXTRA) eps km I in all.  T(x -> x, w) - w is the rounding of the
    coefficients alone, whose exact values are 0 (S, L: the tangency defect <x, w> of w itself, times |x|^2) or cancel (P)."""
    from sympa_amd.manifolds.vector import get_vector_manifold, _factor_slices, _lorentz_sign
    for dims in (d for d in rh.dims_of(model) if d <= 65):
        man = get_vector_manifold(model, dims)
        fx = rh.radam_fixture(model, dims, "later")
        want = fx[rh.setting_key(1.0, 0.0)]
        x, y, w = torch.from_numpy(fx["x"]), torch.from_numpy(want["x"]), torch.from_numpy(fx["m"])
        m = dims // len(vh.FACTORS[model])
        tw = man.transp(x, y, w)
        assert tw.shape == w.shape
        tol = 4 * (m + rh.C_RADAM_EXTRA) * EPS * torch.from_numpy(want["km"])
        i0 = man.inner(x, w)
        assert i0.shape == (16,) and man.inner(x, w, keepdim=True).shape == (16, 1)
        assert torch.equal(man.inner(x, w, w), i0)
        ci, ci_y = man.component_inner(x, w), man.component_inner(y, tw)
        assert ci.shape == x.shape
        if model == "euclidean":
            assert torch.equal(ci, w * w)
        elif len(vh.FACTORS[model]) == 1:
            assert torch.equal(ci, i0[:, None].expand_as(x))
        total = torch.zeros(16, dtype=torch.float64)
        for g, sl in _factor_slices(model, dims):
            ys, ts = y[:, sl], tw[:, sl]
            # E, P, L: an isometry.  S: the section-20 transport is geoopt's, the projection onto the tangent space at y, so
            # |T w|^2 = |w|^2 - <y, w>^2 (Pythagoras) -- it keeps the length only to first order in the step
            before = ci[:, sl].sum(-1) if g == "E" else ci[:, sl][:, 0]
            after = ci_y[:, sl].sum(-1) if g == "E" else ci_y[:, sl][:, 0]
            total = total + before
            expect = before - (ys * w[:, sl]).sum(-1) ** 2 if g == "S" else before
            assert bool(((after - expect).abs() <= tol * before).all()), (model, dims, g, float(((after - expect).abs() / before).max()))
            if g in "SL":
                j = _lorentz_sign(ys) if g == "L" else torch.ones(ys.shape[-1], dtype=ys.dtype)
                defect = (j * ys * ts).sum(-1).abs()
                scale = (ys.abs() * ts.abs()).sum(-1)
                assert bool((defect <= tol * scale).all()), (model, dims, g)
        assert bool(((total - i0).abs() <= 4 * EPS * i0).all())           # inner = the sum over the factors
        same = man.transp(x, x.clone(), w)
        bound = (m + rh.C_RADAM_EXTRA) * EPS * torch.from_numpy(want["km"]) * w.abs().max(-1).values
        assert bool(((same - w).abs().max(-1).values <= bound).all()), (model, dims)
        yy, tt = man.retr_transp(x, torch.zeros_like(x), w)
        assert torch.equal(tt, man.transp(x, yy, w))


@pytest.mark.parametrize("model", vh.MODELS)
def test_torch_transport_matches_the_fixtures(model):
    """the second route to m': torch's transp of m1 along x -> the exact x' is the fixture's exp_avg within its bound (twice:
    m1 and the torch sums carry roundings of their own)"""
    from sympa_amd.manifolds.vector import get_vector_manifold, torch_egrad2rgrad
    for dims in rh.dims_of(model):
        man = get_vector_manifold(model, dims)
        fx = rh.radam_fixture(model, dims, "later")
        want = fx[rh.setting_key(1.0, 0.0)]
        x = torch.from_numpy(fx["x"])
        m1 = rh.BETAS[0] * torch.from_numpy(fx["m"]) + (1 - rh.BETAS[0]) * torch_egrad2rgrad(x, torch.from_numpy(fx["g"]), model)
        got = man.transp(x, torch.from_numpy(want["x"]), m1).numpy()
        assert (np.abs(got - want["m"]).max(1) <= 2 * rh.radam_bound(model, dims, want["m"], want["km"])).all(), (model, dims)


@pytest.mark.parametrize("model", vh.MODELS)
def test_torch_restatement_of_the_row_matches_the_fixtures(model):
    """manifolds.vector.torch_radam_row (what tools/vector_time.py times the kernel against) is the same definition: within
    twice the kernel's bound (its sums are torch's, in another order)."""
    from sympa_amd.manifolds.vector import torch_radam_row
    tally = vh.Tally()
    for dims in rh.dims_of(model):
        for state in rh.STATES:
            fx = rh.radam_fixture(model, dims, state)
            for lr, wd in rh.SETTINGS:
                want = fx[rh.setting_key(lr, wd)]
                y, m, s = torch_radam_row(*(torch.from_numpy(fx[k]) for k in ("x", "g", "m", "s")), _pows(fx), model, lr, rh.BETAS,
                                          rh.EPS_ADAM, wd)
                for cls, got, exact, kappa in (("x", y, want["x"], want["kx"]), ("exp_avg", m, want["m"], want["km"]),
                                               ("exp_avg_sq", s, want["s1"], want["ks"])):
                    tally.check(cls, np.abs(got.numpy() - exact).max(1), 2 * rh.radam_bound(model, dims, exact, kappa),
                                f"{model} dims {dims} {state} lr {lr} wd {wd} {cls}")


def test_radam_entry_validates_its_arguments_without_gpu():
    from sympa_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)       # never dereferenced: validation happens before any launch
    D = ctypes.c_double

    def call(table=one, grad=one, m=one, s=one, rows=8, dims=4, model=0, b1=0.9, b2=0.999, eps=1e-7, pows=one):
        return lib.sympa_vector_radam_step(table, grad, m, s, rows, dims, model, D(0.1), D(b1), D(b2), D(eps), D(0.0), pows, None,
                                           D(0.0), None, None, None)
    assert call(rows=0) == 0                                        # no rows: a no-op
    for null in ("table", "grad", "m", "s", "pows"):
        assert call(**{null: None}) == -1, null
    assert call(b1=1.0) == -1 and call(b1=-0.1) == -1 and call(b2=1.0) == -1 and call(b2=float("nan")) == -1
    assert call(eps=0.0) == -1 and call(eps=-1e-7) == -1
    assert call(model=8) == -1 and call(model=-1) == -1
    assert call(model=4, dims=5) == -1                              # product, odd dims
    assert call(model=3, dims=1) == -1                              # sphere, one coordinate
    assert call(rows=-1) == -1
    assert call(dims=1025) == -2
    assert b"dims" in lib.sympa_last_error()


def test_radam_still_refuses_a_table_on_the_host():
    from sympa_amd.manifolds.base import ManifoldParameter
    from sympa_amd.manifolds.vector import get_vector_manifold
    from sympa_amd.optim import RiemannianAdam
    fx = rh.radam_fixture("poincare", 4, "first")
    p = ManifoldParameter(torch.from_numpy(fx["x"].copy()), manifold=get_vector_manifold("poincare", 4))
    p.grad = torch.from_numpy(fx["g"].copy())
    with pytest.raises(NotImplementedError, match="rsgd"):
        RiemannianAdam([p], lr=0.1).step()
    from sympa_amd import ops
    t = torch.zeros(2, 4, dtype=torch.float64)
    with pytest.raises(Exception):
        ops.vector_radam_step_(t, t, t.clone(), t.clone(), torch.ones(2, dtype=torch.float64), "poincare", 0.1, rh.BETAS, 1e-7, 0.0)
