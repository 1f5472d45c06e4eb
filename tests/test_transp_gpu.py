"""GPU: the parallel transport along geodesics -- C-ABI sympa_transp_exp / sympa_transp through ops, and
SiegelManifold.transp_follow_expmap / expmap_transp / parallel_transport -- against the 100-digit fixtures and the g++ build of the
same arithmetic.  Bounds: tests/transp_helpers.py (the same constants as the CPU build's)."""
import numpy as np
import pytest
import torch

from tests import expmap_helpers as eh
from tests import transp_helpers as th

pytestmark = pytest.mark.gpu
MODELS = ("upper", "bounded")
ROWS = (1, 63, 64, 65, 130)      # the wave edges and a ragged tail over three one-wave blocks


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _d(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _per(x, k):
    return [float(f"{x[k == j].max():.3g}") if (k == j).any() else 0.0 for j in range(4)]


@pytest.mark.parametrize("b", ROWS)
@pytest.mark.parametrize("n", th.DIMS)
@pytest.mark.parametrize("model", MODELS)
def test_kernels_against_fixtures_and_host_build(dev, model, n, b):
    from sympa_amd import _lib, ops
    f = th.fixture(model, n)
    # 1. along a tangent, without the point: fixture rows tiled to b, against the exact values and the g++ build, per norm
    z, u, v, want, want_y, kappa, k = (th.tile_rows(a, b) for a in th.texp_inputs(f))
    zd, ud, vd = _d(z, dev), _d(u, dev), _d(v, dev)
    got = ops.transp_exp(zd, ud, vd, model)
    ops.check_status(dev)
    host, st = th.hostsim_transp_exp(z, u, v, model)
    assert st == 0
    unit = th.EPS64 * kappa
    r, rh = th.row_err(got.cpu().numpy(), want) / unit, th.row_err(got.cpu().numpy(), host) / unit
    print(f"{model} n={n} b={b}: transp_exp kernel / exact per norm {_per(r, k)}, kernel / g++ per norm {_per(rh, k)}")
    c = np.asarray(th.C_TEXP[model])[k]
    assert (r <= c).all() and (rh <= c).all(), (_per(r, k), _per(rh, k))
    # 2. with the point: v' under the same bounds, y under the exponential map's own
    y, got_p = ops.transp_exp(zd, ud, vd, model, return_point=True)
    ops.check_status(dev)
    r, rh = th.row_err(got_p.cpu().numpy(), want) / unit, th.row_err(got_p.cpu().numpy(), host) / unit
    ry = th.row_err(y.cpu().numpy(), want_y) / unit
    print(f"{model} n={n} b={b}: with the point: kernel / exact {_per(r, k)}, kernel / g++ {_per(rh, k)}, y / exact {_per(ry, k)}")
    assert (r <= c).all() and (rh <= c).all(), (_per(r, k), _per(rh, k))
    assert (ry <= np.asarray(eh.C_EXP[model])[k]).all(), _per(ry, k)
    # 3. aliased outputs: out_v = v, out_y = z (and out_v = v alone), the same bits as the separate buffers
    lib = _lib.load()
    za, va, stat = zd.clone(), vd.clone(), torch.zeros(2, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.sympa_transp_exp(za.data_ptr(), ud.data_ptr(), va.data_ptr(), b, n, th.MODEL_IDS[model], za.data_ptr(),
                                    va.data_ptr(), stat.data_ptr(), stream))
    assert torch.equal(za, y) and torch.equal(va, got_p) and not stat.tolist()[0]
    va = vd.clone()
    _lib.check(lib.sympa_transp_exp(zd.data_ptr(), ud.data_ptr(), va.data_ptr(), b, n, th.MODEL_IDS[model], None,
                                    va.data_ptr(), stat.data_ptr(), stream))
    assert torch.equal(va, got) and not stat.tolist()[0]
    # 4. between two points
    z1, z2, vp, wantp, bound = (th.tile_rows(a, b) for a in (f["z1"], f["z2"], f["v_pair"], f["transp"], th.t2_bound(model, f)))
    z1d, z2d, vpd = _d(z1, dev), _d(z2, dev), _d(vp, dev)
    got = ops.transp(z1d, z2d, vpd, model)
    ops.check_status(dev)
    host, st = th.hostsim_transp(z1, z2, vp, model)
    assert st == 0
    r, rh = th.row_err(got.cpu().numpy(), wantp) / bound, th.row_err(got.cpu().numpy(), host) / bound
    print(f"{model} n={n} b={b}: transp kernel / exact {r.max() * th.C_T2[model]:.3g}, kernel / g++ {rh.max() * th.C_T2[model]:.3g}")
    assert (r <= 1.0).all() and (rh <= 1.0).all(), (float(r.max() * th.C_T2[model]), float(rh.max() * th.C_T2[model]))
    va = vpd.clone()
    _lib.check(lib.sympa_transp(z1d.data_ptr(), z2d.data_ptr(), va.data_ptr(), b, n, th.MODEL_IDS[model], va.data_ptr(),
                                stat.data_ptr(), stream))
    assert torch.equal(va, got) and not stat.tolist()[0]


@pytest.mark.parametrize("model", MODELS)
def test_zero_tangent_and_equal_points_on_the_device(dev, model):
    from sympa_amd import ops
    for n in th.DIMS:
        f = th.fixture(model, n)
        z, v = _d(th.tile_rows(f["z1"], 70), dev), _d(th.tile_rows(f["v_pair"], 70), dev)
        v = v + torch.randn(v.shape, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(n))
        sv, sz = 0.5 * (v + v.transpose(-1, -2)), 0.5 * (z + z.transpose(-1, -2))
        y, tv = ops.transp_exp(z, torch.zeros_like(z), v, model, return_point=True)
        assert torch.equal(tv, sv) and torch.equal(y, sz), (model, n)
        assert torch.equal(ops.transp_exp(z, torch.zeros_like(z), v, model), sv), (model, n)
        assert torch.equal(ops.transp(z, z, v, model), sv), (model, n)
        ops.check_status(dev)


@pytest.mark.parametrize("model", MODELS)
def test_manifold_surface(dev, model):
    from sympa_amd import ops
    from sympa_amd.manifolds import BoundedDomainManifold, UpperHalfManifold
    n = 4
    man = (UpperHalfManifold if model == "upper" else BoundedDomainManifold)(dims=n)
    f = th.fixture(model, n)
    keep = f["case"] != "far"
    x, y, v = _d(f["z1"][keep], dev), _d(f["z2"][keep], dev), _d(f["v_pair"][keep], dev).requires_grad_()
    u = _d(f["u"][keep][:, 2], dev)
    tv = man.transp_follow_expmap(x, u, v)
    assert not tv.requires_grad and torch.equal(tv, ops.transp_exp(x, u, v, model))
    yy, tv2 = man.expmap_transp(x, u, v)
    want_y, want_v = ops.transp_exp(x, u, v, model, return_point=True)
    assert not yy.requires_grad and not tv2.requires_grad and torch.equal(yy, want_y) and torch.equal(tv2, want_v)
    pt = man.parallel_transport(x, y, v)
    assert not pt.requires_grad and torch.equal(pt, ops.transp(x, y, v, model))
    assert man.transp(x, y, v) is v                                     # the identity stays
    ops.check_status(dev)
    # the transport preserves invariant_inner: |v'|_y = |v|_x to the bound of the transport carried through the inner product at y
    before, after = man.invariant_inner(x, v.detach())[:, 0, 0, 0], man.invariant_inner(yy, tv2)[:, 0, 0, 0]
    fac = _d((f["kappa"] * np.exp(2.0 * f["usigma"][:, 2]))[keep], dev)
    tol = (2.0 * th.C_TEXP[model][2] + eh.C_EXP[model][2] + 16.0 * n) * th.EPS64 * fac * (1.0 + fac)
    assert (tol < 1e-3).float().mean() > 0.5
    assert (((after - before).abs() / before <= tol) | (tol >= 1e-3)).all()
    xs = x.float()
    for call in (lambda: ops.transp_exp(xs, xs, xs, model), lambda: ops.transp(xs, xs, xs, model)):
        with pytest.raises(ValueError, match="float64"):
            call()


@pytest.mark.parametrize("model", MODELS)
def test_a_tangent_of_invariant_length_100_sets_a_status_bit(dev, model):
    """tanh of the largest singular value rounds to 1 along such a tangent: the status word is set, the launch itself is an ordinary one."""
    from sympa_amd import ops
    f = th.fixture(model, 3)
    keep = f["case"] == "generic"
    z, u, v = _d(f["z1"][keep], dev), _d(f["u"][keep][:, 2] * 100.0, dev), _d(f["v_pair"][keep], dev)
    ops.check_status(dev)
    out = ops.transp_exp(z, u, v, model)
    assert out.shape == z.shape
    with pytest.raises(AssertionError, match="status bits"):
        ops.check_status(dev)
    assert ops.check_status(dev)[0] == 0                               # read and cleared
    good = ops.transp_exp(z, 0.01 * u, v, model)                       # the next launch is unaffected
    ops.check_status(dev)
    assert torch.isfinite(good).all()
