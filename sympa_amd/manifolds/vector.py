"""The vector models of the reference's ManifoldFactory (sympa/embeddings.py:130-158): `euclidean`, `poincare`, `lorentz`,
`sphere` and the products `prod-hysph`, `prod-hyhy`, `prod-hyeu`, `prod-sphsph`.

In the reference these classes ARE geoopt constructors (Euclidean(1), PoincareBall(), Lorentz(), Sphere(), ProductManifold):
none of their arithmetic is in the reference tree and geoopt is not installed here, so parity with geoopt is UNPINNED, as for
`spd`.  The project fixes its own definitions: a point is a row of `dims` doubles split into one or two
factors E, P, L or S, and per factor, with J = diag(-1, 1, ..., 1) for L and I otherwise,
    dd = sum J_i (x_i - y_i)^2,   xx = sum x_i^2,   yy = sum y_i^2
    E: d = sqrt(dd)   P: d = 2 asinh sqrt(dd / ((1 - xx)(1 - yy)))   L: d = 2 asinh sqrt(max(dd, 0) / 4)   S: d = 2 asin sqrt(min(dd / 4, 1))
a product's distance being sqrt(d_1^2 + d_2^2).  On the manifold these equal geoopt's 2 artanh |(-x) (+) y|, arcosh(-<x, y>_L)
and acos <x, y>; unlike those they do not cancel for close points and need no clamp constants.

Device tensors go through the HIP kernels (csrc/vector_models.hip); host tensors through the same formulas in plain torch
(initialisation, tests), as in spd.py."""
import torch

from sympa_amd import ops
from sympa_amd.config import EPS
from sympa_amd.manifolds.base import Manifold

BALL_EPS = EPS[torch.float64]        # projx keeps Poincare points at norm <= 1 - BALL_EPS


def _factor_slices(model, dims):
    factors = ops.VECTOR_FACTORS[model]
    m = dims // len(factors)
    return [(g, slice(k * m, (k + 1) * m)) for k, g in enumerate(factors)]


def _lorentz_sign(x):
    j = torch.ones(x.shape[-1], dtype=x.dtype, device=x.device)
    j[0] = -1.0
    return j


# ---- the definitions in torch ops (any device; differentiable away from q == 0)
def torch_factor_dist(x, y, geom):
    w = x - y
    if geom == "L":
        dd = (_lorentz_sign(x) * w * w).sum(-1)
    else:
        dd = (w * w).sum(-1)
    if geom == "E":
        return dd.sqrt()
    if geom == "P":
        q = dd / ((1.0 - (x * x).sum(-1)) * (1.0 - (y * y).sum(-1)))
        return 2.0 * torch.asinh(q.sqrt())
    if geom == "L":
        return 2.0 * torch.asinh((dd.clamp_min(0.0) / 4.0).sqrt())
    return 2.0 * torch.asin((dd / 4.0).clamp_max(1.0).sqrt())


def torch_dist(x, y, model):
    ds = [torch_factor_dist(x[..., s], y[..., s], g) for g, s in _factor_slices(model, x.shape[-1])]
    if len(ds) == 1:
        return ds[0]
    return (ds[0] * ds[0] + ds[1] * ds[1]).sqrt()


def torch_egrad2rgrad(x, u, model):
    out = torch.empty_like(u)
    for g, s in _factor_slices(model, x.shape[-1]):
        xs, us = x[..., s], u[..., s]
        if g == "E":
            out[..., s] = us
        elif g == "P":
            out[..., s] = us * ((1.0 - (xs * xs).sum(-1, keepdim=True)) ** 2 / 4.0)
        elif g == "S":
            out[..., s] = us - (xs * us).sum(-1, keepdim=True) * xs
        else:
            out[..., s] = _lorentz_sign(xs) * us + (xs * us).sum(-1, keepdim=True) * xs
    return out


def torch_projx(x, model):
    """-> (projected rows, mask of the rows whose Poincare factor was rescaled)"""
    out = x.clone()
    moved = torch.zeros(x.shape[:-1], dtype=torch.bool, device=x.device)
    for g, s in _factor_slices(model, x.shape[-1]):
        xs = x[..., s]
        if g == "P":
            nrm = xs.norm(dim=-1, keepdim=True)
            over = nrm > 1.0 - BALL_EPS
            out[..., s] = torch.where(over, xs * ((1.0 - BALL_EPS) / nrm), xs)
            moved |= over.squeeze(-1)
        elif g == "S":
            out[..., s] = xs / xs.norm(dim=-1, keepdim=True)
        elif g == "L":
            o = xs.clone()
            o[..., 0] = (1.0 + (xs[..., 1:] ** 2).sum(-1)).sqrt()
            out[..., s] = o
    return out, moved


def torch_retr(x, u, model):
    """geoopt's retr per factor: E, P: projx(x + u); S: (x + u) / |x + u|; L: expmap, then projx."""
    out = torch.empty_like(x)
    for g, s in _factor_slices(model, x.shape[-1]):
        xs, us = x[..., s], u[..., s]
        if g == "L":
            nu = (_lorentz_sign(us) * us * us).sum(-1, keepdim=True).clamp_min(0.0).sqrt()
            ratio = torch.where(nu > 0, torch.sinh(nu) / torch.where(nu > 0, nu, torch.ones_like(nu)), torch.ones_like(nu))
            out[..., s] = torch.cosh(nu) * xs + ratio * us
        else:
            out[..., s] = xs + us
    return torch_projx(out, model)[0]


def torch_rsgd_row(x, grad, model, lr, wd=0.0):
    g = grad + wd * x
    return torch_retr(x, -lr * torch_egrad2rgrad(x, g, model), model)


def torch_component_inner(x, u, v, model):
    """geoopt's component_inner per factor: E: u_i v_i per coordinate; P: (2 / (1 - xx))^2 <u, v>, S: <u, v>,
    L: <u, v>_L, one value per factor held in every coordinate of the factor."""
    out = torch.empty_like(u)
    for g, s in _factor_slices(model, x.shape[-1]):
        xs, us, vs = x[..., s], u[..., s], v[..., s]
        if g == "E":
            out[..., s] = us * vs
            continue
        if g == "L":
            val = (_lorentz_sign(xs) * us * vs).sum(-1, keepdim=True)
        else:
            val = (us * vs).sum(-1, keepdim=True)
        if g == "P":
            val = val * (2.0 / (1.0 - (xs * xs).sum(-1, keepdim=True))) ** 2
        out[..., s] = val.expand_as(us)
    return out


def torch_transp(x, y, v, model):
    """Parallel transport of v from x to y per factor, in forms that are the identity at y = x without a 0 / 0 (section 20):
    E: v;  S: v - <y, v> y;  L: v + <y, v>_L / (2 + dd_L / 2) (x + y), dd_L = <x - y, x - y>_L;  P: (1 - yy) / (1 - xx) gyr[y, -x] v."""
    out = torch.empty_like(v)
    for g, s in _factor_slices(model, x.shape[-1]):
        xs, ys, vs = x[..., s], y[..., s], v[..., s]
        if g == "E":
            out[..., s] = vs
        elif g == "S":
            out[..., s] = vs - (ys * vs).sum(-1, keepdim=True) * ys
        elif g == "L":
            j = _lorentz_sign(xs)
            w = xs - ys
            den = 2.0 + 0.5 * (j * w * w).sum(-1, keepdim=True)
            out[..., s] = vs + (j * ys * vs).sum(-1, keepdim=True) / den * (xs + ys)
        else:
            # gyr[a, b] v = v + 2 (A a + B b) / D with a = y, b = -x
            aw, bw = (ys * vs).sum(-1, keepdim=True), -(xs * vs).sum(-1, keepdim=True)
            ab = -(xs * ys).sum(-1, keepdim=True)
            aa, bb = (ys * ys).sum(-1, keepdim=True), (xs * xs).sum(-1, keepdim=True)
            A = -aw * bb + bw + 2.0 * ab * bw
            B = -bw * aa - aw
            D = 1.0 + 2.0 * ab + aa * bb
            out[..., s] = (1.0 - aa) / (1.0 - bb) * (vs + 2.0 * (A * ys - B * xs) / D)
    return out


def torch_radam_row(x, grad, exp_avg, exp_avg_sq, pows, model, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """The RiemannianAdam row of section 20 in torch ops -> (new rows, exp_avg, exp_avg_sq); pows = (beta1^t, beta2^t)."""
    g = grad + wd * x
    r = torch_egrad2rgrad(x, g, model)
    m1 = betas[0] * exp_avg + (1.0 - betas[0]) * r
    s1 = betas[1] * exp_avg_sq + (1.0 - betas[1]) * torch_component_inner(x, r, r, model).clamp_min(0.0)
    u = -lr * (m1 / (1.0 - pows[0])) / ((s1 / (1.0 - pows[1])).sqrt() + eps)
    y = torch_retr(x, u, model)
    return y, torch_transp(x, y, m1, model), s1


class VectorManifold(Manifold):
    """Common part of the five classes: `model_name` selects the factors; everything on the device is one kernel."""
    ndim = 1
    reversible = False
    __scaling__ = Manifold.__scaling__.copy()
    model_name = None

    def __init__(self, dims=None):
        super().__init__()
        self.dims = dims
        if dims is not None:
            ops.vector_check_dims(self.model_name, int(dims))
        self._projected_points = 0
        self._device_projected = {}       # device -> persistent int32 counter the optimiser step adds to

    @property
    def projected_points(self):
        for counter in self._device_projected.values():
            self._projected_points += int(counter.item())
            counter.zero_()
        return self._projected_points

    @projected_points.setter
    def projected_points(self, value):
        for counter in self._device_projected.values():
            counter.zero_()
        self._projected_points = value

    def projected_counter(self, device):
        key = str(device)
        if key not in self._device_projected:
            self._device_projected[key] = torch.zeros(1, dtype=torch.int32, device=device)
        return self._device_projected[key]

    def _rows(self, *ts):
        ops.vector_check_dims(self.model_name, ts[0].shape[-1])
        return [t.reshape(-1, t.shape[-1]) for t in ts]

    def dist(self, x, y, *, keepdim=False):
        if x.is_cuda:
            from sympa_amd import autograd as sa
            xr, yr = self._rows(*torch.broadcast_tensors(x, y))
            d = sa.vector_dist(xr, yr, self.model_name).reshape(torch.broadcast_shapes(x.shape, y.shape)[:-1])
        else:
            ops.vector_check_dims(self.model_name, x.shape[-1])
            d = torch_dist(x, y, self.model_name)
        return d.unsqueeze(-1) if keepdim else d

    def egrad2rgrad(self, x, u):
        if x.is_cuda:
            xr, ur = self._rows(x, u)
            return ops.vector_egrad2rgrad(xr, ur, self.model_name).reshape(x.shape)
        ops.vector_check_dims(self.model_name, x.shape[-1])
        return torch_egrad2rgrad(x, u, self.model_name)

    def proju(self, x, u):
        """Projection onto the tangent space: the identity for E and P, u - <x, u> x for S, u + <x, u>_L x for L."""
        out = u.clone()
        for g, s in _factor_slices(self.model_name, x.shape[-1]):
            xs, us = x[..., s], u[..., s]
            if g == "S":
                out[..., s] = us - (xs * us).sum(-1, keepdim=True) * xs
            elif g == "L":
                out[..., s] = us + (_lorentz_sign(xs) * xs * us).sum(-1, keepdim=True) * xs
        return out

    def retr(self, x, u):
        """Plain torch (initialisation, tests); the optimiser uses the fused sympa_vector_rsgd_step."""
        return torch_retr(x, u, self.model_name)

    def transp(self, x, y, v):
        """Parallel transport of the tangent vector v from x to y (plain torch, any device; the optimiser's is inside the fused
        sympa_vector_radam_step)."""
        ops.vector_check_dims(self.model_name, x.shape[-1])
        return torch_transp(x, y, v, self.model_name)

    def component_inner(self, x, u, v=None):
        """geoopt's component_inner, in the shape of x: what RiemannianAdam's second moment accumulates."""
        ops.vector_check_dims(self.model_name, x.shape[-1])
        return torch_component_inner(x, u, u if v is None else v, self.model_name)

    def inner(self, x, u, v=None, keepdim=False):
        """The Riemannian inner product <u, v>_x: the sum over the factors (E: the plain dot product)."""
        ops.vector_check_dims(self.model_name, x.shape[-1])
        v = u if v is None else v
        total = None
        for g, s in _factor_slices(self.model_name, x.shape[-1]):
            ci = torch_component_inner(x[..., s], u[..., s], v[..., s], {"E": "euclidean", "P": "poincare", "L": "lorentz",
                                                                         "S": "sphere"}[g])
            val = ci.sum(-1, keepdim=True) if g == "E" else ci[..., :1]
            total = val if total is None else total + val
        return total if keepdim else total.squeeze(-1)

    def projx(self, x):
        if x.is_cuda:
            (xr,) = self._rows(x)
            counter = torch.zeros(1, dtype=torch.int32, device=x.device)
            out = ops.vector_projx(xr, self.model_name, counter=counter).reshape(x.shape)
            self.projected_points += int(counter.item())
            return out
        ops.vector_check_dims(self.model_name, x.shape[-1])
        out, moved = torch_projx(x, self.model_name)
        self.projected_points += int(moved.sum())
        return out

    def _check_shape(self, shape, name):
        ok = len(shape) >= 1
        if ok:
            try:
                ops.vector_check_dims(self.model_name, shape[-1])
            except ValueError as e:
                return False, f"`{name}`: {e}"
        return ok, None if ok else f"`{name}` should be a vector"

    def bad_rows(self, x, atol=1e-5, rtol=1e-5):
        """bool [...]: rows that are off the manifold, from batched ops (no synchronisation)."""
        bad = ~torch.isfinite(x).all(-1)
        for g, s in _factor_slices(self.model_name, x.shape[-1]):
            xs = x[..., s]
            if g == "P":
                bad |= ~((xs * xs).sum(-1) < 1.0)
            elif g == "S":
                bad |= ((xs * xs).sum(-1) - 1.0).abs() > atol + rtol
            elif g == "L":
                inner = (_lorentz_sign(xs) * xs * xs).sum(-1)
                bad |= ((inner + 1.0).abs() > atol + rtol * (xs * xs).sum(-1)) | ~(xs[..., 0] > 0)
        return bad

    def _check_point_on_manifold(self, x, *, atol=1e-5, rtol=1e-5):
        ok = not bool(self.bad_rows(x, atol, rtol).any())
        return ok, None if ok else f"a factor of `x` is off the {self.name} manifold with atol={atol}, rtol={rtol}"

    def random(self, *size, dtype=None, device=None, from_=-1e-3, to=1e-3, **kwargs):
        """uniform(from_, to) in every coordinate, then projx: a point near the origin (E, P) or on the manifold (S, L)."""
        x = torch.empty(*size, dtype=torch.get_default_dtype()).uniform_(from_, to)
        return torch_projx(x, self.model_name)[0].to(device=device, dtype=dtype)


class Euclidean(VectorManifold):
    name = "Euclidean"
    model_name = "euclidean"


class PoincareBall(VectorManifold):
    name = "PoincareBall"
    model_name = "poincare"


class Lorentz(VectorManifold):
    name = "Lorentz"
    model_name = "lorentz"


class Sphere(VectorManifold):
    name = "Sphere"
    model_name = "sphere"


class ProductManifold(VectorManifold):
    """Two factors of dims / 2 coordinates each (embeddings.py:150-157): `prod-hysph`, `prod-hyhy`, `prod-hyeu`, `prod-sphsph`."""
    name = "ProductManifold"

    def __init__(self, model_name, dims=None):
        if model_name not in ops.VECTOR_MODEL_IDS or len(ops.VECTOR_FACTORS[model_name]) != 2:
            raise ValueError(f"not a product model: {model_name!r}")
        self.model_name = model_name
        super().__init__(dims)


VECTOR_MANIFOLDS = {"euclidean": Euclidean, "poincare": PoincareBall, "lorentz": Lorentz, "sphere": Sphere}


def get_vector_manifold(model_name, dims=None):
    if model_name in VECTOR_MANIFOLDS:
        return VECTOR_MANIFOLDS[model_name](dims)
    return ProductManifold(model_name, dims)
