"""RiemannianAdam on the spd model without a GPU: the g++ build of sympa::spd_row_radam
(tests/hostsim/hostsim_spd_radam.cpp) against the 50-digit fixtures of tools/make_golden_spd_radam_exact.py within the bounds of
tests/spd_radam_helpers.py; the manifold's transp / inner / component_inner and torch_radam_row in torch; the C entry's argument
checks; the optimiser's state."""
import ctypes

import numpy as np
import pytest
import torch

from tests import spd_radam_helpers as rh


TRANSP_ROUTE = 20.0      # the eigh route of the manifold's transp (see test_manifold_transp_agrees_with_the_fixtures)


def _run(cell, **kw):
    return rh.hostsim_radam(cell["x"], cell["g"], cell["m"], cell["s"], cell["lr"], cell["wd"], cell["pows"], **kw)


def test_hostsim_matches_every_fixture_within_the_bounds():
    tally = rh.Tally(rh.C_ONE_LANE)
    for n in rh.DIMS:
        for cell in rh.cells(n):
            y, m, s, st, bad = _run(cell)
            assert st == 0 and bad == 0, cell["label"]
            tally.check(cell, y, m, s, "hostsim")
            assert (y == np.swapaxes(y, 1, 2)).all() and (m == np.swapaxes(m, 1, 2)).all(), cell["label"]
            if cell["case"] == "diag":        # exact zeros off the diagonal
                off = ~np.eye(n, dtype=bool)
                assert (y[:, off] == 0.0).all() and (m[:, off] == 0.0).all(), cell["label"]
    tally.report("hostsim, one row per lane")


def test_no_bound_exceeds_the_cap():
    for n in rh.DIMS:
        for cell in rh.cells(n):
            for C in (rh.C_ONE_LANE, rh.C_SIXTEEN_LANES):
                unit = C * n * rh.EPS64
                for k in (cell["ky"], cell["km"], cell["ks"]):
                    assert (unit * k <= rh.CAP).all(), (cell["label"], float(k.max()))


def test_fixtures_cover_what_they_are_for():
    for n in rh.DIMS:
        for cell in rh.cells(n):
            x, w = rh.sym(cell["x"]), cell["want"]
            assert (np.linalg.eigvalsh(w["y"]) > 0.0).all(), cell["label"]          # y is SPD
            assert (w["y"] == np.swapaxes(w["y"], 1, 2)).all() and (w["m"] == np.swapaxes(w["m"], 1, 2)).all()
            if cell["lr"] == 1.0 and cell["state"] == "later":
                assert (w["cq"] > 0.5).all(), (cell["label"], w["cq"])               # the cubic term matters
            if cell["state"] == "later":
                assert cell["t"] == 7 and (cell["s"] > 0.0).all()
                assert np.array_equal(cell["pows_prev"], np.array([0.9 ** 6, 0.999 ** 6]))
                for i in range(2):          # Riemannian length of m: 0.8 .. 1.5 of |r|
                    li = np.linalg.inv(np.linalg.cholesky(x[i]))
                    r = x[i] @ rh.sym(cell["g"][i]) @ x[i]
                    ratio = np.linalg.norm(li @ cell["m"][i] @ li.T) / np.linalg.norm(li @ r @ li.T)
                    assert 0.79 < ratio < 1.51, (cell["label"], ratio)
            else:
                assert cell["t"] == 1 and not cell["m"].any() and not cell["s"].any()
            if cell["case"] == "cond1e6" and n > 1:
                assert np.allclose(np.linalg.cond(x), np.exp(14.0), rtol=1e-6)
            if cell["case"] == "init":
                assert np.abs(x - np.eye(n)).max() <= 1e-3
            if cell["case"] == "diag":
                off = ~np.eye(n, dtype=bool)
                assert not x[:, off].any() and not cell["g"][:, off].any() and not cell["m"][:, off].any()
                assert not w["y"][:, off].any() and not w["m"][:, off].any()
            if cell["case"] == "scalar" and cell["wd"] == 0.0:      # Q = alpha I: m' is a multiple of y
                for i in range(2):
                    q = np.linalg.solve(w["y"][i], w["m"][i])
                    assert np.abs(q - q[0, 0] * np.eye(n)).max() <= 1e-9 * abs(q[0, 0]), cell["label"]


def _inner(x, v):
    """tr(x^-1 v x^-1 v) = || L^-1 v L^-T ||_F^2 in extended precision (the check's own arithmetic must not count)"""
    x, v = x.astype(np.longdouble), v.astype(np.longdouble)
    b, n = x.shape[0], x.shape[1]
    L = np.zeros_like(x)
    for j in range(n):
        L[:, j, j] = np.sqrt(x[:, j, j] - (L[:, j, :j] ** 2).sum(1))
        for i in range(j + 1, n):
            L[:, i, j] = (x[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(1)) / L[:, j, j]
    w = v.copy()
    for _ in range(2):          # w <- L^-1 w, then transposed: L^-1 v L^-T
        for i in range(n):
            w[:, i, :] = (w[:, i, :] - (L[:, i, :i, None] * w[:, :i, :]).sum(1)) / L[:, i, i, None]
        w = np.swapaxes(w, 1, 2).copy()
    return (w * w).sum((1, 2))


def test_hostsim_transport_is_an_isometry():
    """tr(y^-1 m' y^-1 m') against tr(x^-1 m1 x^-1 m1) for the computed y and m': relative difference within the exp_avg bound
    doubled."""
    worst = 0.0
    for n in rh.DIMS:
        for cell in rh.cells(n):
            y, m, s, _, _ = _run(cell)
            x = rh.sym(cell["x"])
            r = x @ (rh.sym(cell["g"]) + cell["wd"] * x) @ x
            m1 = rh.BETAS[0] * rh.sym(cell["m"]) + (1.0 - rh.BETAS[0]) * r
            before, after = _inner(x, m1), _inner(y, m)
            tol = 2.0 * rh.C_ONE_LANE * n * rh.EPS64 * cell["km"]
            rel = np.abs(after - before) / before
            worst = max(worst, float((rel / tol).max()))
            assert (rel <= tol).all(), (cell["label"], rel, tol)
    print(f"[spd radam] isometry: worst relative difference / (2 x exp_avg bound) = {worst:.3g}")


@pytest.fixture(scope="module")
def manifold():
    from sympa_amd.manifolds.spd import SymmetricPositiveDefinite
    return SymmetricPositiveDefinite()


def test_manifold_transp_agrees_with_the_fixtures(manifold):
    """the eigh route of SymmetricPositiveDefinite.transp against the 50-digit m' (both are the definition E m1 E^T).  eigh is
    backward stable in the norm of its matrix only, so x^(1/2) and x^(-1/2) each carry n eps cond(x)^(1/2) and E m1 E^T twice
    that: TRANSP_ROUTE = 20 (the two eigh, the eight matrix products, both sides) n eps cond(x), relative to max |m'|."""
    for n in (1, 2, 5, 16):
        for cell in rh.cells(n):
            x = rh.sym(cell["x"])
            r = x @ (rh.sym(cell["g"]) + cell["wd"] * x) @ x
            m1 = rh.BETAS[0] * rh.sym(cell["m"]) + (1.0 - rh.BETAS[0]) * r
            got = manifold.transp(torch.from_numpy(x), torch.from_numpy(cell["want"]["y"]), torch.from_numpy(m1)).numpy()
            err = np.abs(got - cell["want"]["m"]).max((1, 2))
            scale = np.abs(cell["want"]["m"]).max((1, 2))
            rel = TRANSP_ROUTE * n * rh.EPS64 * np.linalg.cond(x)
            assert (err <= rel * scale).all(), (cell["label"], err / scale, rel)


def test_manifold_transp_identity_and_isometry(manifold):
    g = torch.Generator().manual_seed(3)
    x, y = manifold.random(6, 5, 5, dtype=torch.float64), manifold.random(6, 5, 5, dtype=torch.float64)
    v = torch.randn(6, 5, 5, generator=g, dtype=torch.float64)
    v = 0.5 * (v + v.transpose(-1, -2))          # any tangent vector: not parallel to log_x(y)
    assert torch.allclose(manifold.transp(x, x, v), v, rtol=0, atol=1e-13 * float(v.abs().max()))
    t = manifold.transp(x, y, v)
    assert torch.allclose(manifold.inner(y, t), manifold.inner(x, v), rtol=1e-11, atol=0)
    assert torch.allclose(manifold.inner(y, t, manifold.transp(x, y, x)), manifold.inner(x, v, x), rtol=1e-10, atol=1e-12)
    y2, t2 = manifold.retr_transp(x, 0.1 * v, v)
    assert torch.equal(y2, manifold.retr(x, 0.1 * v)) and torch.allclose(manifold.inner(y2, t2), manifold.inner(x, v), rtol=1e-11, atol=0)


def test_manifold_inner_and_component_inner(manifold):
    g = torch.Generator().manual_seed(4)
    x = manifold.random(3, 4, 4, dtype=torch.float64)
    u, v = (torch.randn(3, 4, 4, generator=g, dtype=torch.float64) for _ in range(2))
    u, v = 0.5 * (u + u.transpose(-1, -2)), 0.5 * (v + v.transpose(-1, -2))
    xi = torch.linalg.inv(x)
    want = torch.einsum("bij,bji->b", xi @ u, xi @ v)
    assert manifold.inner(x, u, v).shape == (3,) and torch.allclose(manifold.inner(x, u, v), want, rtol=1e-12, atol=0)
    assert manifold.inner(x, u, v, keepdim=True).shape == (3, 1, 1)
    assert torch.allclose(manifold.inner(x, u), torch.einsum("bij,bji->b", xi @ u, xi @ u), rtol=1e-12, atol=0)
    ci = manifold.component_inner(x, u)
    assert ci.shape == x.shape and torch.equal(ci, manifold.inner(x, u, keepdim=True).expand_as(x))
    assert (manifold.inner(x, u) > 0).all()


def test_torch_radam_row_against_the_fixtures(manifold):
    """manifolds.spd.torch_radam_row (what tools/spd_radam_time.py times the kernel against) is the same definition through the
    manifold's inner, retr and transp (eigh): exp_avg compared like transp above, y and exp_avg_sq at ten times the kernel's
    bound times cond(x) (torch.linalg.solve and inv in place of the factor's congruences: forward errors with cond x)."""
    from sympa_amd.manifolds.spd import torch_radam_row
    for n in (1, 3, 8, 16):
        for cell in rh.cells(n):
            y, m, s = torch_radam_row(manifold, *(torch.from_numpy(cell[k]) for k in ("x", "g", "m", "s")),
                                      torch.from_numpy(cell["pows"]), cell["lr"], rh.BETAS, rh.EPS_ADAM, cell["wd"])
            w = cell["want"]
            cond = np.linalg.cond(rh.sym(cell["x"]))
            by, bm, bs = rh.bounds(cell, 10.0 * rh.C_ONE_LANE)
            assert (np.abs(y.numpy() - w["y"]).max((1, 2)) <= by * cond).all(), cell["label"]
            assert (np.abs(s.numpy() - w["s1"]) <= bs * cond).all(), cell["label"]
            rel = TRANSP_ROUTE * n * rh.EPS64 * cond
            assert (np.abs(m.numpy() - w["m"]).max((1, 2)) <= rel * np.abs(w["m"]).max((1, 2))).all(), cell["label"]


def test_zero_gradient_and_zero_state_stay_zero():
    for n in (1, 2, 7, 16):
        cell = rh.cells(n)[0]
        z = np.zeros_like(cell["x"])
        y, m, s, st, _ = rh.hostsim_radam(cell["x"], z, z, np.zeros(2), 1.0, 0.0, rh.BETAS)
        assert st == 0 and not m.any() and not s.any() and np.array_equal(y, rh.sym(cell["x"]))


def test_lr_zero_leaves_the_point_and_gives_m1():
    for n in (1, 2, 7, 16):
        for cell in rh.cells(n):
            if cell["lr"] != 1.0:
                continue
            y, m, s, st, _ = rh.hostsim_radam(cell["x"], cell["g"], cell["m"], cell["s"], 0.0, cell["wd"], cell["pows"])
            y1, m1, s1, _, _ = _run(cell)
            x = rh.sym(cell["x"])
            assert np.array_equal(y, x) and np.array_equal(s, s1), cell["label"]
            r = x @ rh.sym(cell["g"]) @ x
            want = rh.BETAS[0] * rh.sym(cell["m"]) + (1.0 - rh.BETAS[0]) * r
            scale = np.abs(x).max() ** 2 * np.abs(cell["g"]).max() + np.abs(cell["m"]).max()
            assert np.abs(m - want).max() <= 4 * n * n * rh.EPS64 * scale, cell["label"]


def test_a_row_that_does_not_factor_sets_not_pd():
    cell = rh.cells(5)[0]
    x = cell["x"].copy()
    x[1] = -x[1]
    *_, st, bad = rh.hostsim_radam(x, cell["g"], cell["m"], cell["s"], 0.01, 0.0, cell["pows"])
    assert st == rh.ST_NOT_PD and bad == 1


def test_spd_radam_entry_validates_its_arguments_without_gpu():
    from sympa_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # never dereferenced: validation happens before any launch
    D = ctypes.c_double

    def call(table=one, grad=one, m=one, s=one, rows=8, n=4, b1=0.9, b2=0.999, eps=1e-7, pows=one, sq=None, max_norm=0.0):
        return lib.sympa_spd_radam_step(table, grad, m, s, rows, n, D(0.1), D(b1), D(b2), D(eps), D(0.0), pows, sq, D(max_norm),
                                        None, None)

    assert call(rows=0) == 0                                   # a no-op
    for null in ("table", "grad", "m", "s", "pows"):
        assert call(**{null: None}) == -1, null
    assert call(b1=1.0) == -1 and call(b2=-0.1) == -1 and call(b2=1.0) == -1
    assert call(eps=0.0) == -1
    assert call(sq=one, max_norm=0.0) == -1
    assert call(n=0) == -2 and call(n=17) == -2
    assert b"dims" in lib.sympa_last_error()


def _spd_param(n_rows=5, n=3, device=None):
    from sympa_amd.manifolds.base import ManifoldParameter
    from sympa_amd.manifolds.spd import SymmetricPositiveDefinite
    man = SymmetricPositiveDefinite()
    return ManifoldParameter(man.random(n_rows, n, n, dtype=torch.float64), manifold=man)


def test_a_host_spd_table_is_refused_naming_rsgd():
    from sympa_amd.optim import RiemannianAdam
    p = _spd_param()
    opt = RiemannianAdam([p], lr=0.1, eps=1e-7)
    p.grad = torch.ones_like(p)
    with pytest.raises(NotImplementedError, match="rsgd"):
        opt.step()


def test_exp_avg_sq_is_one_value_per_point():
    from sympa_amd.optim import RiemannianAdam
    p = _spd_param(7, 4)
    opt = RiemannianAdam([p], lr=0.1, eps=1e-7)
    opt.init_state()
    st = opt.state[p]
    assert st["exp_avg"].shape == (7, 4, 4) and st["exp_avg_sq"].shape == (7,) and st["bias_pows"].tolist() == [1.0, 1.0]
