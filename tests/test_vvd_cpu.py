"""CPU (`-m "not gpu"`): the backward of the vector-valued distance (sympa::pair_backward_vvd, g++ build of tests/hostsim/
hostsim_vvd.cpp) against the 50-digit directional derivatives of the sorted v, dims 1..16, the three Siegel models, and the argument
validation of the three C-ABI entries.  Bounds and method: tests/vvd_helpers.py."""
import ctypes

import numpy as np
import pytest

from sympa_amd import _lib
from tests import vvd_helpers as vh


@pytest.mark.parametrize("n", vh.DIMS)
@pytest.mark.parametrize("model", vh.MODELS)
def test_hostsim_vvd_backward_exact(model, n):
    def route(z1, z2, gv):
        g1, g2, v, st = vh.hostsim_vvd_bwd(z1, z2, gv, model)
        assert st == 0
        return g1, g2, v
    vh.check_route(model, n, route, "hostsim")


@pytest.mark.parametrize("model", vh.MODELS)
def test_hostsim_equal_points_give_zero_gradient_and_zero_v(model):
    """dv / dlambda = 0 at lambda = 0: src == dst is a zero gradient, never NaN."""
    for n in (1, 3, 4, 5, 8, 11):
        fx = vh.fixture(model, n)
        z = fx["generic__z1"]
        gv = vh.cotangent("mixed", len(z), n, 5)
        g1, g2, v, st = vh.hostsim_vvd_bwd(z, z, gv, model)
        assert st == 0
        assert np.array_equal(g1, np.zeros_like(g1)) and np.array_equal(g2, np.zeros_like(g2)), (model, n)
        assert np.array_equal(v, np.zeros_like(v)), (model, n)


@pytest.mark.parametrize("model", vh.MODELS)
def test_hostsim_zero_cotangent_gives_zero_gradient(model):
    for n in (2, 4, 6, 9):
        fx = vh.fixture(model, n)
        z1, z2 = fx["generic__z1"], fx["generic__z2"]
        g1, g2, v, st = vh.hostsim_vvd_bwd(z1, z2, np.zeros((len(z1), n)), model)
        assert st == 0 and not g1.any() and not g2.any()
        assert (vh.v_errors(fx, "generic", v) <= vh.fwd_bound(model, fx, "generic")).all()


def test_hostsim_matches_the_scalar_backward_on_a_linear_metric():
    """fone is sum v: its backward with go is the vvd backward with gv = go in every component -- the same core, two spectral
    stages."""
    from tests.helpers import hostsim_dist_bwd
    for model in ("upper", "bounded"):
        for n in (2, 4, 7):
            fx = vh.fixture(model, n)
            z1, z2 = fx["generic__z1"], fx["generic__z2"]
            go = vh.cotangent("positive", len(z1), 1, 3)[:, 0]
            _, g1, g2, _, st = hostsim_dist_bwd(z1, z2, go, model, "fone")
            h1, h2, _, st2 = vh.hostsim_vvd_bwd(z1, z2, np.repeat(go[:, None], n, 1), model)
            assert st == 0 and st2 == 0
            assert np.array_equal(g1, h1) and np.array_equal(g2, h2), (model, n)


def test_dual_cut_locus_is_nan_and_flagged():
    """sin(v) = 1: v is not differentiable; NaN gradients, NaN v and SYMPA_ST_NONFINITE, never a silent zero."""
    z1 = np.array([0.5, 0.0]).reshape(1, 2, 1, 1)      # n = 1: x = -1 / conj(w) is exactly on the cut locus
    z2 = np.array([-2.0, 0.0]).reshape(1, 2, 1, 1)
    g1, g2, v, st = vh.hostsim_vvd_bwd(z1, z2, np.ones((1, 1)), "dual")
    assert st & 2 and not np.isfinite(g1).any() and not np.isfinite(g2).any() and np.isnan(v).all()


def test_entries_validate_their_arguments_without_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # never dereferenced: validation happens before any launch
    D = ctypes.c_double
    BAD, DIMS = -1, -2

    def fwd(table=one, rows=10, n=4, src=one, dst=one, b=8, model=0, eps=1e-5, out=one, flags=0):
        return lib.sympa_model_vvd_forward(table, rows, n, src, 2, dst, 2, b, model, D(eps), out, None, flags, None)

    def bwd(z1=one, z2=one, gv=one, b=8, n=4, model=0, eps=1e-5, g1=one, g2=one, flags=0):
        return lib.sympa_siegel_vvd_bwd(z1, z2, gv, b, n, model, D(eps), g1, g2, None, None, flags, None)

    def mbwd(table=one, rows=10, n=4, src=one, dst=one, b=8, model=0, eps=1e-5, gv=one, gt=one, flags=0):
        return lib.sympa_model_vvd_backward(table, rows, n, src, 2, dst, 2, b, model, D(eps), gv, gt, None, None, flags, None)

    for f in (fwd, bwd, mbwd):
        assert f(b=0) == 0                       # a no-op
        assert f(b=-1) == BAD
        assert f(model=3) == BAD
        assert f(flags=1) == BAD and b"flags" in lib.sympa_last_error()
        assert f(eps=0.0) == BAD
        assert f(n=0) == DIMS and f(n=17) == DIMS and b"dims" in lib.sympa_last_error()
    for name in ("table", "src", "dst", "out"):
        assert fwd(**{name: None}) == BAD, name
    assert fwd(rows=0) == BAD
    for name in ("z1", "z2", "gv", "g1", "g2"):
        assert bwd(**{name: None}) == BAD, name
    for name in ("table", "src", "dst", "gv", "gt"):
        assert mbwd(**{name: None}) == BAD, name
    assert mbwd(rows=0) == BAD


def test_ops_refuse_cpu_tensors():
    import torch
    from sympa_amd import ops
    z = torch.zeros(2, 2, 3, 3, dtype=torch.float64)
    t = torch.zeros(2, 2, dtype=torch.int64)
    gv = torch.zeros(2, 3, dtype=torch.float64)
    with pytest.raises(_lib.SympaHipError):
        ops.model_vvd_forward(z, t)
    with pytest.raises(_lib.SympaHipError):
        ops.siegel_vvd_backward(z, z, gv)
    with pytest.raises(_lib.SympaHipError):
        ops.model_vvd_backward(z, t, gv)


def test_forward_vvd_is_for_the_siegel_models_only():
    from sympa_amd.model import Model
    import torch
    for manifold in ("spd", "euclidean"):
        class A:
            metric, dims, num_points = "riem", 3, 5
            scale_coef, scale_init, train_scale = 1.0, 1.0, False
        A.manifold = manifold
        m = Model(A)
        with pytest.raises(NotImplementedError, match="forward_vvd"):
            m.forward_vvd(torch.zeros(2, 2, dtype=torch.int64))
