"""SiegelManifold: base class of the complex-symmetric-matrix models
(reference sympa/manifolds/siegel_manifold.py:11-167).  Same constructor, attributes and method
signatures; `dist` runs the fused gfx950 kernel instead of ~100 ATen ops with 4 host syncs."""
from abc import ABC
from typing import Optional, Tuple, Union

import torch

from sympa_amd import ops
from sympa_amd.manifolds.base import Manifold
from sympa_amd.manifolds.metrics import Metric, MetricType


def _sym(x):
    return 0.5 * (x + x.transpose(-1, -2))


class SiegelManifold(Manifold, ABC):
    ndim = 1
    reversible = False
    name = "Siegel Space"
    __scaling__ = Manifold.__scaling__.copy()
    model_name = "upper"     # which kernel prologue `dist` uses

    def __init__(self, dims=2, ndim=2, metric=MetricType.RIEMANNIAN, use_xitorch=False):
        super().__init__()
        self.dims = dims
        self.ndim = ndim
        self._projected_points = 0
        self._device_projected = {}       # device -> persistent int32 counter the fused optimiser step adds to
        self.metric = Metric.get(metric, self.dims)

    @property
    def projected_points(self):
        """Number of points projx had to move (runner.py:47-48 logs it).  Counters produced by the fused
        optimiser kernel are folded in here, so the training loop itself never synchronises."""
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
        """The device counter sympa_rsgd_step accumulates into.  It persists across steps (nothing is allocated or
        zeroed per step), so the optimiser step can be captured in a hipGraph and replayed."""
        key = str(device)
        if key not in self._device_projected:
            self._device_projected[key] = torch.zeros(1, dtype=torch.int32, device=device)
        return self._device_projected[key]

    # ------------------------------------------------------------------ the hot path
    def _metric_weights(self):
        return self.metric.weights if self.metric.kind is MetricType.WEIGHTED_SUM else None

    def dist(self, z1: torch.Tensor, z2: torch.Tensor, *, keepdim=False) -> torch.Tensor:
        """z1, z2: b x 2 x n x n on the GPU -> b distances (siegel_manifold.py:41-72)."""
        from sympa_amd.autograd import siegel_dist
        return siegel_dist(z1, z2, self.model_name, self.metric.kind.value, self._metric_weights())

    def vvd(self, z1, z2):
        """Ascending vector-valued distance v [b, n] (the reference's intermediate, siegel_manifold.py:69-70); differentiable
        when an input requires grad (sympa_siegel_vvd_bwd).  Every metric is a function of v, so a custom one is ordinary torch code
        on it, e.g. an lp norm:
            v = manifold.vvd(z1, z2);  d = v.pow(p).sum(-1).pow(1 / p)"""
        from sympa_amd.autograd import siegel_vvd
        return siegel_vvd(z1, z2, self.model_name)

    # ------------------------------------------------------------------ geoopt surface
    def retr(self, x, u):  # siegel_manifold.py:74-87
        return self.projx(x + u)

    def _check_shape(self, shape: Tuple[int], name: str) -> Union[Tuple[bool, Optional[str]], bool]:
        ok = shape[-1] == self.dims and shape[-2] == self.dims   # siegel_manifold.py:89-118
        reason = None if ok else "'{}' on the {} requires more than {} dim".format(name, self, self.dims)
        return ok, reason

    def _check_matrices_are_symmetric(self, x, *, atol=1e-5, rtol=1e-5):  # siegel_manifold.py:120-128
        return torch.allclose(x, x.transpose(-1, -2), atol=atol, rtol=rtol)

    def projx(self, x):  # siegel_manifold.py:130-137
        return torch.stack((_sym(x[:, 0]), _sym(x[:, 1])), dim=1)

    def _projx_kernel(self, z):
        """projx of the concrete model as one HIP kernel; keeps `projected_points` like the reference
        (upper_half.py:64: the reference also synchronises here with `.item()`)."""
        counter = torch.zeros(1, dtype=torch.int32, device=z.device)
        out = ops.projx(z, self.model_name, counter=counter)
        self.projected_points += int(counter.item())
        return out

    def proju(self, x, u):
        return self.egrad2rgrad(x, u)

    def transp(self, x, y, v):  # siegel_manifold.py:142-154: Euclidean transport
        # stays the identity (RiemannianAdam is pinned to it); the transport of the invariant metric is parallel_transport /
        # transp_follow_expmap / expmap_transp below
        return v

    # The exponential and logarithm maps (empty in the reference, siegel_manifold.py:156-162).  They belong to the invariant
    # metric of the model, of which the riem distance measures `dist_scale` times the length:
    #     riem dist(x, expmap(x, u)) = dist_scale * |u|_x,    logmap(x, expmap(x, u)) = sym(u),    expmap(x, logmap(x, y)) = y.
    # |u|_x^2 is `inner(x, u, u)` for the upper model; for the bounded model it is Re tr[(I - x conj x)^-1 u (I - conj(x) x)^-1 conj u]
    # = inner(x, conj u, conj u): the reference's bounded inner (bounded_domain.py:86-116) has the two inverses the other way
    # round, which agrees at n = 1 and at real points only.
    # One HIP kernel per call (sympa_expmap / sympa_logmap): float64 [b,2,n,n] on the GPU, dims 1..8.  NOT differentiable in this
    # version: they run under no_grad and return tensors without a graph.
    @property
    def dist_scale(self):
        """c in riem dist(x, expmap(x, u)) = c * |u|_x: 1 for the upper model, 2 for the bounded one, at any dims."""
        return {"upper": 1.0, "bounded": 2.0}[self._expmap_model(any_dims=True)]

    def _expmap_model(self, any_dims=False):
        if self.model_name not in ops.EXPMAP_MODELS:
            raise NotImplementedError(f"{type(self).__name__} has no exponential / logarithm map: the model has no inner product "
                                      "to take them from (the reference's inner raises NotImplementedError, compact_dual.py:96)")
        if not any_dims and not 1 <= self.dims <= ops.EXPMAP_MAX_DIMS:
            raise NotImplementedError(f"expmap / logmap / geodesic: dims 1..{ops.EXPMAP_MAX_DIMS} (one row per lane), got dims = "
                                      f"{self.dims}")
        return self.model_name

    @torch.no_grad()
    def expmap(self, x, u):
        """expmap_x(u) of sym(u); pure, no clamp to the eps-interior (follow with projx for that).  Not differentiable."""
        return ops.expmap(x, u, self._expmap_model())

    @torch.no_grad()
    def logmap(self, x, y):
        """The symmetric tangent vector at x whose geodesic reaches y at time 1; exactly 0 for y = x.  Not differentiable."""
        return ops.logmap(x, y, self._expmap_model())

    @torch.no_grad()
    def geodesic(self, t, x, y):
        """The point at time t of the geodesic from x (t = 0) to y (t = 1): expmap(x, t * logmap(x, y)).  t: a number or a tensor
        that broadcasts against [b, 1, 1, 1].  Not differentiable."""
        model = self._expmap_model()
        return ops.expmap(x, t * ops.logmap(x, y, model), model)

    # Parallel transport along geodesics, for the same invariant metric (the reference approximates it by the identity,
    # siegel_manifold.py:142-154, which `transp` keeps).  geoopt's names; one HIP kernel per call (sympa_transp_exp /
    # sympa_transp), float64 [b,2,n,n] on the GPU, dims 1..8, under no_grad and NOT differentiable, with the refusals of expmap.
    # The transport preserves `invariant_inner`.
    @torch.no_grad()
    def transp_follow_expmap(self, x, u, v):
        """sym(v) transported from x along t -> expmap(x, t u) to expmap(x, u); u = 0 returns sym(v) bit for bit."""
        return ops.transp_exp(x, u, v, self._expmap_model())

    @torch.no_grad()
    def expmap_transp(self, x, u, v):
        """(expmap(x, u), the transport of sym(v) to it) from one kernel."""
        return ops.transp_exp(x, u, v, self._expmap_model(), return_point=True)

    @torch.no_grad()
    def parallel_transport(self, x, y, v):
        """sym(v) transported from x to y along the geodesic between them; y = x returns sym(v) bit for bit."""
        return ops.transp(x, y, v, self._expmap_model())

    def invariant_inner(self, x, u, v=None):
        """The inner product of the invariant metric, the one the maps and the transport belong to, in the layout of `inner`
        (host torch, any device): `inner` itself for the upper model; Re tr[(I - x conj x)^-1 u (I - conj(x) x)^-1 conj v] for the
        bounded model, whose reference `inner` has the two inverses the other way round."""
        model = self._expmap_model(any_dims=True)
        if v is None:
            v = u
        if model == "upper":
            return self.inner(x, u, v)
        xc, uc, vc = (torch.complex(t[:, 0], t[:, 1]) for t in (x, u, v))
        eye = torch.eye(x.shape[-1], dtype=xc.dtype, device=x.device)
        res = torch.linalg.inv(eye - xc @ xc.conj()) @ uc @ torch.linalg.inv(eye - xc.conj() @ xc) @ vc.conj()
        real = res.real.diagonal(dim1=-2, dim2=-1).sum(-1, keepdim=True).unsqueeze(-1)
        return torch.stack((real, real), dim=1)

    def _check_vector_on_tangent(self, x, u, *, atol=1e-5, rtol=1e-5):
        pass
