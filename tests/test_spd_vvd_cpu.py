"""CPU (`-m "not gpu"`): the spd model's vector-valued distance -- the fixtures (tests/golden/exact_spd_vvd_n*.npz), the g++ build of
the arithmetic (tests/hostsim/hostsim_spd_vvd.cpp over spd_math.hpp / spd_math_bwd.hpp) against them on every case and n, the tie
convention, spd_metric, the options of the manifold, Model and tools/train_siegel.py, and the argument validation of the four C-ABI
entries.  Bounds and their reasoning: tests/spd_vvd_helpers.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from tests import spd_vvd_helpers as h
from tests.helpers import ROOT, hostsim_spd_bwd
from tests.test_spd_exact import EPS64, MAX_BOUND, check, fwd_errors, fwd_tol, pool, skip_same


def _args(**kw):
    class A:
        manifold, metric, dims, num_points = "spd", "riem", 3, 5
        scale_coef, scale_init, train_scale = 1.0, 1.0, False
    for k, v in kw.items():
        setattr(A, k, v)
    return A


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("n", h.DIMS)
def test_fixture_consistency(n):
    """shapes; v ascending and equal to log of the source fixture's lam (to the rounding of the stored lam); ||v|| = dist;
    sum_j dvvd_j = dsum and sum_j (v_j / dist) dvvd_j = the source's ddx / ddy; no bound of any pair near O(1); only the six scalar
    pairs exempt (n >= 2)."""
    p, vx = h.vpool(n), h.vfixture(n)
    src = np.load(os.path.join(ROOT, "tests", "golden", f"exact_spd_n{n}.npz"))
    for case in p["names"]:
        v, dv, ds = vx[f"{case}__v"], vx[f"{case}__dvvd"], vx[f"{case}__dsum"]
        assert v.shape == (6, n) and dv.shape == (6, 3, 2, n) and ds.shape == (6, 3, 2)
        for a in (v, dv, ds):
            assert a.dtype == np.float64 and np.isfinite(a).all()
        assert (np.diff(v, axis=1) >= 0).all()
        lam, dist = src[f"{case}__lam"], src[f"{case}__dist"]
        assert (np.abs(v - np.log(lam)) <= 4 * EPS64 * (1.0 + 1.0 / np.abs(lam - 1.0).clip(1e-300)) + 4 * EPS64 * np.abs(v)).all()
        np.testing.assert_allclose(np.sqrt((v ** 2).sum(1)), dist, rtol=1e-14)
        scale = np.abs(dv).sum(-1)
        assert (np.abs(dv.sum(-1) - ds) <= 4 * EPS64 * n * scale).all()
        dd = np.stack((src[f"{case}__ddx"], src[f"{case}__ddy"]), -1)
        got = np.einsum("bn,bkpn->bkp", v / dist[:, None], dv)
        assert (np.abs(got - dd) <= 4 * EPS64 * n * np.einsum("bn,bkpn->bkp", np.abs(v) / dist[:, None], np.abs(dv))).all()
    ex = h.exempt(p)
    assert int(ex.sum()) == (6 if n >= 2 else 0)
    for coop in (False, True):
        tol = h.g_tol(p, coop)
        assert tol[np.arange(len(tol)) != p["same"]].max() < MAX_BOUND
    if n >= 2:      # the smallest gap of every pair that is checked per component, relative to ||A||
        live = ~p["scalar"] & (np.arange(len(ex)) != p["same"])
        rel = np.diff(p["lam"][live], axis=1).min(1) / np.abs(p["lam"][live] - 1.0).max(1)
        assert rel.min() >= 5e-12


def test_generator_reproduces_a_committed_fixture():
    """tools/make_golden_spd_vvd_exact.py regenerates tests/golden/exact_spd_vvd_n2.npz byte for byte (its own three checks run inside)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_spd_vvd_exact as gen
    finally:
        sys.path.pop(0)
    n, arrs, _ = gen.generate(2)
    assert gen.npz_bytes(arrs) == open(os.path.join(ROOT, "tests", "golden", "exact_spd_vvd_n2.npz"), "rb").read()


# ---------------------------------------------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize("n", h.DIMS)
def test_hostsim_exact(n):
    """spd_pair_vvd and spd_pair_backward_vvd (g++ build) on every case against the 70-digit v and directional derivatives, both
    cotangent sets; the scalar pairs against c dsum; y = x exact zeros."""
    p = h.vpool(n)
    v, st = h.hostsim_spd_vvd_fwd(p["x"], p["y"])
    assert st == 0
    h.check_v(p, v, False, f"hostsim spd_pair_vvd n={n}")

    def route(x, y, gv):
        gx, gy, vb, st = h.hostsim_spd_vvd_bwd(x, y, gv)
        assert st == 0
        return gx, gy, vb
    h.check_route(n, route, f"hostsim spd_pair_backward_vvd n={n}", False)


@pytest.mark.parametrize("n", h.DIMS)
def test_hostsim_consistent_with_the_distance_backward(n):
    """gv = v / ||v|| turns the vvd backward into spd_pair_backward: the two agree within the sum of their bounds, and
    spd_metric(v, "riem") is the distance."""
    from sympa_amd.manifolds.spd import spd_metric
    p = h.vpool(n)
    out, gx0, gy0, st = hostsim_spd_bwd(p["x"], p["y"])
    assert st == 0
    gx, gy, v, st = h.hostsim_spd_vvd_bwd(p["x"], p["y"], h.unit_cotangent(p))
    assert st == 0
    h.check_against_distance_backward(n, gx, gy, gx0, gy0, False, f"vvd backward against spd_pair_backward n={n}")
    d = spd_metric(torch.from_numpy(v), "riem").numpy()
    check(fwd_errors(pool(n), d), fwd_tol(pool(n)), skip_same(pool(n)), f"spd_metric(v, riem) n={n}")


def test_ties_x_equals_y_and_zero_cotangent():
    """an exact tie (y = 2 x) with a constant cotangent is finite and equals c d log det; x == y gives v = 0 and exact zero gradients
    whatever the cotangent; a zero cotangent gives exact zeros."""
    p = h.vpool(5)
    i = int(np.flatnonzero(p["scalar"])[0])
    x, y = p["x"][i:i + 1], p["y"][i:i + 1]
    assert np.array_equal(y, 2.0 * x)
    gx, gy, v, st = h.hostsim_spd_vvd_bwd(x, y, np.full((1, 5), 0.75))
    assert st == 0 and np.isfinite(gx).all() and np.isfinite(gy).all()
    np.testing.assert_allclose(v, np.log(2.0), rtol=1e-14)
    np.testing.assert_allclose(gy[0], 0.75 * np.linalg.inv(y[0]), rtol=1e-11)
    np.testing.assert_allclose(gx[0], -0.75 * np.linalg.inv(x[0]), rtol=1e-11)
    gx, gy, v, st = h.hostsim_spd_vvd_bwd(x, x, h.cotangent("mixed", 1, 5, 3))
    assert st == 0 and not gx.any() and not gy.any() and not v.any()
    gx, gy, v, st = h.hostsim_spd_vvd_bwd(p["x"], p["y"], np.zeros_like(p["v"]))
    assert st == 0 and not gx.any() and not gy.any()
    # a point that is not positive definite is flagged (status bit 1: ST_NOT_PD)
    bad = x.copy()
    bad[0, 0, 0] = -1.0
    assert h.hostsim_spd_vvd_bwd(bad, y, np.ones((1, 5)))[3] & 1
    assert h.hostsim_spd_vvd_fwd(bad, y)[1] & 1


# ---------------------------------------------------------------------------------------------------------------- Python
def test_spd_metric():
    from sympa_amd.manifolds.spd import spd_metric
    v = torch.tensor([[-3.0, 0.5, 2.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    assert torch.equal(spd_metric(v, "fone"), torch.tensor([5.5, 0.0], dtype=torch.float64))
    assert torch.equal(spd_metric(v, "finf"), torch.tensor([3.0, 0.0], dtype=torch.float64))
    torch.testing.assert_close(spd_metric(v, "riem"), torch.tensor([np.sqrt(13.25), 0.0], dtype=torch.float64))
    with pytest.raises(ValueError):
        spd_metric(v, "fmin")
    vv = v[:1].clone().requires_grad_(True)
    spd_metric(vv, "fone").sum().backward()
    assert torch.equal(vv.grad, torch.tensor([[-1.0, 1.0, 1.0]], dtype=torch.float64))


def test_manifold_and_model_options():
    from sympa_amd.embeddings import ManifoldFactory
    from sympa_amd.manifolds import SymmetricPositiveDefinite
    from sympa_amd.model import Model
    assert SymmetricPositiveDefinite().finsler is None
    for kind in (None, "riem", "fone", "finf"):
        assert SymmetricPositiveDefinite(finsler=kind).finsler == kind
    with pytest.raises(ValueError):
        SymmetricPositiveDefinite(finsler="fmin")
    with pytest.raises(NotImplementedError):
        SymmetricPositiveDefinite(default_metric="LEM")
    assert ManifoldFactory.get_manifold("spd", "fone", 3).finsler is None          # metric_name stays ignored for spd
    assert Model(_args()).manifold.finsler is None
    assert Model(_args(spd_metric="finf")).manifold.finsler == "finf"
    assert hasattr(SymmetricPositiveDefinite, "vvd")


def test_the_ops_refuse_cpu_tensors():
    from sympa_amd import _lib, ops
    x = torch.eye(3, dtype=torch.float64).repeat(2, 1, 1)
    t = torch.zeros(2, 2, dtype=torch.int64)
    gv = torch.ones(2, 3, dtype=torch.float64)
    for call in (lambda: ops.spd_vvd_forward(x, x), lambda: ops.spd_model_vvd_forward(x, t), lambda: ops.spd_vvd_backward(x, x, gv),
                 lambda: ops.spd_model_vvd_backward(x, t, gv)):
        with pytest.raises(_lib.SympaHipError):
            call()


@pytest.mark.parametrize("kind", ("fone", "finf"))
def test_a_finsler_model_never_runs_the_riemannian_routes(kind):
    """host model: forward reaches forward_vvd, which is not built for a host table; the list, evaluation and fused-loss routes and
    the graphed / distributed steps refuse outright."""
    from sympa_amd.model import Model
    from sympa_amd.optim import RiemannianSGD
    from sympa_amd.train_step import DistributedTrainStep, GraphedTrainStep
    m = Model(_args(spd_metric=kind))
    t = torch.zeros(2, 2, dtype=torch.int64)
    gd = torch.ones(2, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="forward_vvd"):
        m(t)
    for call in (lambda: m.forward_batches([t]), lambda: m.prepare_batches([t]), lambda: m.evaluate(t, gd, 2),
                 lambda: m.evaluate_all_pairs(None), lambda: m.distance_matrix(), lambda: m.fused_loss_backward(t, gd),
                 lambda: m.mean_average_precision(None)):
        with pytest.raises(NotImplementedError, match=kind):
            call()
    opt = RiemannianSGD(m.parameters(), lr=1e-2, weight_decay=0.0, stabilize=None)
    with pytest.raises(NotImplementedError, match="GraphedTrainStep"):
        GraphedTrainStep(m, opt, 2, 50.0, "cpu")
    with pytest.raises(NotImplementedError, match="DistributedTrainStep"):
        DistributedTrainStep(m, opt, 2, 50.0, "cpu")
    # riem / None keep the existing kernel path: nothing refuses at construction
    Model(_args(spd_metric="riem"))._refuse_finsler("x")


def test_train_siegel_spd_metric_on_a_host_model():
    """tools/train_siegel.py --manifold spd --spd-metric finf: the option reaches the manifold, and the classic loop's forward on a host
    model raises forward_vvd's NotImplementedError instead of training on the Riemannian distance."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train_siegel as ts
    finally:
        sys.path.pop(0)
    from sympa_amd.model import Model
    args = ts.parser().parse_args(["--manifold", "spd", "--spd-metric", "finf", "--dims", "3"])
    assert ts.parser().parse_args([]).spd_metric == "riem" and ts.finsler_kind(args) == "finf"
    args.num_points = 5
    m = Model(args)
    assert m.manifold.finsler == "finf"
    with pytest.raises(NotImplementedError, match="forward_vvd"):
        ts.finsler_loss_backward(m, torch.zeros(2, 2, dtype=torch.int64), torch.ones(2, dtype=torch.float64))
    with pytest.raises(SystemExit):
        ts.finsler_kind(ts.parser().parse_args(["--manifold", "upper", "--spd-metric", "fone"]))


# ---------------------------------------------------------------------------------------------------------------- C-ABI
def test_abi_argument_validation_without_gpu():
    from sympa_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # never dereferenced: validation happens before any launch
    GENERIC, COOP = 2, 32
    fwd = lambda x=one, y=one, b=8, n=4, out=one, flags=0: lib.sympa_spd_vvd_fwd(x, y, b, n, out, None, flags, None)
    mfwd = lambda tab=one, rows=10, n=4, src=one, dst=one, b=8, out=one, flags=0: \
        lib.sympa_spd_model_vvd_forward(tab, rows, n, src, 2, dst, 2, b, out, None, flags, None)
    bwd = lambda x=one, y=one, gv=one, b=8, n=4, gx=one, gy=one, flags=0: \
        lib.sympa_spd_vvd_bwd(x, y, gv, b, n, gx, gy, None, None, flags, None)
    mbwd = lambda tab=one, rows=10, n=4, src=one, dst=one, b=8, gv=one, gt=one, flags=0: \
        lib.sympa_spd_model_vvd_backward(tab, rows, n, src, 2, dst, 2, b, gv, gt, None, None, flags, None)
    for f in (fwd, mfwd, bwd, mbwd):
        assert f(b=0) == 0 and f(b=0, flags=GENERIC) == 0            # b == 0 is a no-op
        assert f(b=-1) == -1
        assert f(flags=COOP) == -1 and f(flags=1) == -1 and f(flags=GENERIC | 4) == -1
        assert f(n=0) == -2 and f(n=17) == -2
        assert b"dims" in lib.sympa_last_error()
    assert fwd(x=None) == -1 and fwd(y=None) == -1 and fwd(out=None) == -1
    assert mfwd(tab=None) == -1 and mfwd(src=None) == -1 and mfwd(dst=None) == -1 and mfwd(out=None) == -1 and mfwd(rows=0) == -1
    assert bwd(x=None) == -1 and bwd(y=None) == -1 and bwd(gv=None) == -1 and bwd(gx=None) == -1 and bwd(gy=None) == -1
    assert mbwd(tab=None) == -1 and mbwd(src=None) == -1 and mbwd(dst=None) == -1 and mbwd(gv=None) == -1 and mbwd(gt=None) == -1
    assert mbwd(rows=0) == -1
