"""CompactDualManifold  M_n = {Z in Sym(n, C)}: every complex symmetric matrix is a point
(reference sympa/manifolds/compact_dual.py).

`dist`: the reference factorises W (Takagi, with eigenvectors), moves X by the isometry that sends W to 0, factorises the image
again and takes arctan of its Takagi values (compact_dual.py:25-62).  The HIP kernels evaluate the same vector-valued distance as
the bounded domain with the signs turned round:
    A(Z) = I + Z Z^H = C C^H,   E = C1^-1 (Z2 - Z1) C2^-T,   sin(v_i) = sigma_i(E),   v_i in [0, pi/2].
`egrad2rgrad` and `projx` are HIP kernels as well; `inner` does not exist in the reference either, so RiemannianAdam declines this
manifold."""
import torch

from sympa_amd import ops
from sympa_amd.manifolds.base import Manifold
from sympa_amd.manifolds.metrics import MetricType
from sympa_amd.manifolds.siegel_manifold import SiegelManifold


class CompactDualManifold(SiegelManifold):
    ndim = 1
    reversible = False
    name = "Compact Dual"
    __scaling__ = Manifold.__scaling__.copy()
    model_name = "dual"

    def __init__(self, dims=2, ndim=2, metric=MetricType.RIEMANNIAN):
        # (the reference passes use_xitorch=True to pick its eigen-solver, compact_dual.py:21-23; no solver is picked here)
        super().__init__(dims=dims, ndim=ndim, metric=metric)

    def egrad2rgrad(self, z, u):  # compact_dual.py:64-79: (I + conj(Z) Z) G (I + Z conj(Z))  (HIP kernel)
        return ops.egrad2rgrad(z, u, self.model_name)

    def projx(self, z):
        """Symmetrise (the reference inherits SiegelManifold.projx, siegel_manifold.py:130-137).  On the GPU one HIP kernel and no
        host synchronisation: no row can leave this manifold, so there is no counter to read back."""
        if z.is_cuda and z.dtype == torch.float64:
            return ops.projx(z, self.model_name)
        return super().projx(z)

    def inner(self, z, u, v=None, *, keepdim=False):  # compact_dual.py:95-96
        raise NotImplementedError()

    def _check_point_on_manifold(self, z, *, atol=1e-5, rtol=1e-5):  # compact_dual.py:81-93
        if not self._check_matrices_are_symmetric(z, atol=atol, rtol=rtol):
            return False, "Matrices are not symmetric"
        return True, None

    def random(self, *size, dtype=None, device=None, **kwargs):  # compact_dual.py:98-105: the bounded domain's base points
        from sympa_amd.manifolds.bounded_domain import BoundedDomainManifold
        return BoundedDomainManifold(dims=self.dims).random(*size, dtype=dtype, device=device, **kwargs)
