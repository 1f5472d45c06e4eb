"""SymmetricPositiveDefinite: the `spd` model of the reference (sympa/embeddings.py:6,70-72,142).

In the reference this class IS geoopt.manifolds.SymmetricPositiveDefinite() (default affine-invariant metric):
none of its arithmetic is in the reference tree, geoopt is not installed here, and no reference test touches
it -- parity is UNPINNED with respect to geoopt: the oracle restates geoopt's published formulas, and the
kernels are checked against that restatement and against 50-digit mpmath evaluations of the same formulas
(tests/golden/spd_n*.npz).  dist (forward and backward), egrad2rgrad, retr, projx are HIP kernels."""
import torch

from sympa_amd import ops
from sympa_amd.manifolds.base import Manifold


def _sym(x):
    return 0.5 * (x + x.transpose(-1, -2))


def torch_radam_row(manifold, x, grad, exp_avg, exp_avg_sq, bias_pows, lr, betas=(0.9, 0.999), eps_adam=1e-8, weight_decay=0.0,
                    coef=1.0):
    """One RiemannianAdam step of an spd table in torch ops on any device, built on the manifold's own egrad2rgrad formula,
    inner, retr and transp (what sympa_spd_radam_step computes in one kernel).  x, grad, exp_avg [N, n, n],
    exp_avg_sq [N], bias_pows = (beta1^t, beta2^t) of this step.  Returns (y, exp_avg', exp_avg_sq'); the inputs are left alone."""
    b1, b2 = betas
    xs = _sym(x)
    r = xs @ (coef * _sym(grad) + weight_decay * xs) @ xs
    m1 = b1 * _sym(exp_avg) + (1.0 - b1) * r
    s1 = b2 * exp_avg_sq + (1.0 - b2) * manifold.inner(xs, r).clamp_min(0.0)
    c = -lr / (1.0 - bias_pows[0]) / ((s1 / (1.0 - bias_pows[1])).sqrt() + eps_adam)
    y, mt = manifold.retr_transp(xs, c.reshape(-1, 1, 1) * m1, m1)
    return y, _sym(mt), s1


FINSLER_KINDS = ("riem", "fone", "finf")


def spd_metric(v, kind):
    """A distance from the vector-valued distance v [..., n] of the spd model (SymmetricPositiveDefinite.vvd; signed,
    v_j = log lam_j):  riem = sqrt(sum v^2) (the affine-invariant distance),  fone = sum |v_j|,  finf = max |v_j|  (the Finsler
    distances of the symmetric space).  Ordinary torch code: differentiable through v."""
    if kind == "riem":
        return v.pow(2).sum(-1).sqrt()
    if kind == "fone":
        return v.abs().sum(-1)
    if kind == "finf":
        return v.abs().amax(-1)
    raise ValueError(f"spd_metric: kind must be one of {FINSLER_KINDS}, got {kind!r}")


class SymmetricPositiveDefinite(Manifold):
    name = "SymmetricPositiveDefinite"
    ndim = 2
    reversible = False
    __scaling__ = Manifold.__scaling__.copy()
    model_name = "spd"

    def __init__(self, default_metric="AIM", finsler=None):
        super().__init__()
        if str(default_metric).upper() not in ("AIM", "SPDMETRIC.AIM"):
            raise NotImplementedError("only geoopt's default affine-invariant metric (AIM) is built")
        if finsler is not None and finsler not in FINSLER_KINDS:
            raise ValueError(f"finsler must be None or one of {FINSLER_KINDS}, got {finsler!r}")
        self.finsler = finsler
        self.projected_points = 0

    def vvd(self, x, y):
        """[b, n]: the vector-valued distance, log of the eigenvalues of x^-1 y, ascending and signed; differentiable with respect
        to both points (HIP kernels forward and backward)."""
        from sympa_amd import autograd as sa
        return sa.spd_vvd(x, y)

    def dist(self, x, y, *, keepdim=False):
        """|| log(x^-1/2 y x^-1/2) ||_F  (geoopt SymmetricPositiveDefinite.dist, AIM); differentiable.  With finsler = "fone" /
        "finf": spd_metric(self.vvd(x, y), finsler)."""
        from sympa_amd import autograd as sa
        d = spd_metric(self.vvd(x, y), self.finsler) if self.finsler in ("fone", "finf") else sa.spd_dist(x, y)
        return d.unsqueeze(-1).unsqueeze(-1) if keepdim else d

    def egrad2rgrad(self, x, u):
        """geoopt: x @ sym(u) @ x."""
        return ops.spd_egrad2rgrad(x, u)

    def proju(self, x, u):
        return _sym(u)

    def retr(self, x, u):
        """geoopt: sym(x + u + 1/2 u x^-1 u), evaluated by the step kernel with lr = -1 on egrad-free input: host-side
        torch here (init / tests); the optimiser uses the fused sympa_spd_rsgd_step."""
        return _sym(x + u + 0.5 * u @ torch.linalg.inv(x) @ u)

    def expmap(self, x, u):
        """The affine-invariant exponential map x^1/2 exp(x^-1/2 sym(u) x^-1/2) x^1/2 (geoopt SymmetricPositiveDefinite.expmap, AIM):
        HIP kernels over [b, n, n] float64 device tensors (ops.spd_expmap); not differentiable, no host
        version.  retr stays geoopt's second-order retraction."""
        return ops.spd_expmap(x, u)

    def logmap(self, x, y):
        """x^1/2 log(x^-1/2 y x^-1/2) x^1/2: the tangent at x with expmap(x, .) = y (ops.spd_logmap)."""
        return ops.spd_logmap(x, y)

    def geodesic(self, t, x, y):
        """The point of the geodesic from x (t = 0) to y (t = 1) at the real parameter t, one value for all pairs
        (ops.spd_geodesic)."""
        return ops.spd_geodesic(x, y, t)

    def inner(self, x, u, v=None, keepdim=False):
        """geoopt (AIM): tr(x^-1 u x^-1 v), one number per point; plain torch on any device."""
        xu = torch.linalg.solve(x, u)
        xv = xu if v is None else torch.linalg.solve(x, v)
        out = (xu * xv.transpose(-1, -2)).sum((-1, -2))
        return out.unsqueeze(-1).unsqueeze(-1) if keepdim else out

    def component_inner(self, x, u, v=None):
        """geoopt's default: the point's inner product, broadcast over the point's components."""
        return self.inner(x, u, v, keepdim=True).expand_as(x)

    def transp(self, x, y, v):
        """Affine-invariant parallel transport of ANY tangent vector v along the geodesic x -> y, by its definition:
        E v E^T with E = (y x^-1)^(1/2) = x^(1/2) (x^(-1/2) y x^(-1/2))^(1/2) x^(-1/2)  (two torch.linalg.eigh).  The step
        kernel transports exp_avg along its own step, where this collapses to a cubic polynomial."""
        lam, q = torch.linalg.eigh(_sym(x))
        xh = q @ (lam.sqrt().unsqueeze(-1) * q.transpose(-1, -2))
        xmh = q @ (lam.rsqrt().unsqueeze(-1) * q.transpose(-1, -2))
        mu, w = torch.linalg.eigh(_sym(xmh @ _sym(y) @ xmh))
        e = xh @ (w @ (mu.sqrt().unsqueeze(-1) * w.transpose(-1, -2))) @ xmh
        return e @ v @ e.transpose(-1, -2)

    def _check_shape(self, shape, name):
        ok = len(shape) >= 2 and shape[-1] == shape[-2]
        return ok, None if ok else f"`{name}` should be a square matrix"

    def _check_point_on_manifold(self, x, *, atol=1e-5, rtol=1e-5):
        if not torch.allclose(x, x.transpose(-1, -2), atol=atol, rtol=rtol):
            return False, "`x != x.transpose` with atol={}, rtol={}".format(atol, rtol)
        ok = bool((torch.linalg.eigvalsh(x) > -atol).all())
        return ok, None if ok else "eigenvalues of x are not all greater than 0."

    def projx(self, x):
        """geoopt: sym_funcm(sym(x), abs) -- HIP kernel for device tensors, torch on the host (initialisation)."""
        if x.is_cuda:
            return ops.spd_projx(x)
        s = _sym(x)
        lam, v = torch.linalg.eigh(s)
        return v @ torch.diag_embed(lam.abs()) @ v.transpose(-1, -2)

    def random(self, *size, dtype=None, device=None, **kwargs):
        """geoopt SymmetricPositiveDefinite.random: expm(sym(0.5 * randn))."""
        t = _sym(0.5 * torch.randn(*size, dtype=torch.get_default_dtype()))
        lam, v = torch.linalg.eigh(t)
        return (v @ torch.diag_embed(torch.exp(lam)) @ v.transpose(-1, -2)).to(device=device, dtype=dtype)
