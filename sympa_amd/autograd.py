"""autograd glue for the hot path: forward and backward are both HIP kernels behind the C-ABI.
The backward kernels recompute the forward quantities (nothing but the inputs is saved)."""
import torch

from sympa_amd import ops


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class _SiegelDistFn(torch.autograd.Function):
    """manifold.dist(z1, z2) with the analytic backward (sympa_siegel_dist_bwd)."""

    @staticmethod
    def forward(ctx, z1, z2, weights, model, metric):
        ctx.save_for_backward(z1, z2, weights if weights is not None else torch.empty(0, device=z1.device))
        ctx.model, ctx.metric, ctx.has_w = model, metric, weights is not None
        return ops.siegel_dist_forward(z1, z2, model, metric, weights)

    @staticmethod
    def backward(ctx, grad_out):
        z1, z2, w = ctx.saved_tensors
        w = w if ctx.has_w else None
        g1, g2, gw = ops.siegel_dist_backward(z1, z2, grad_out, ctx.model, ctx.metric, w)
        if gw is not None and w is not None:
            gw = gw.reshape(w.shape)
        return g1, g2, (gw if ctx.has_w and ctx.metric == "wsum" else None), None, None


def siegel_dist(z1, z2, model, metric, weights=None):
    if _needs_grad(z1, z2, weights):
        return _SiegelDistFn.apply(z1, z2, weights, model, metric)
    return ops.siegel_dist_forward(z1, z2, model, metric, weights)


class _ModelForwardFn(torch.autograd.Function):
    """Fused Model.forward with the scatter-add backward (sympa_model_backward): the gradient of the
    table is the dense [N,2,n,n] tensor the reference's DDP all-reduces (train.py:59, runner.py:105)."""

    @staticmethod
    def forward(ctx, table, triplets, weights, scale, model, metric, scale_coef):
        dev = table.device
        ctx.save_for_backward(table, triplets, weights if weights is not None else torch.empty(0, device=dev),
                              scale if scale is not None else torch.empty(0, device=dev))
        ctx.cfg = (model, metric, scale_coef, weights is not None, scale is not None)
        return ops.model_forward(table, triplets, model, metric, weights, scale, scale_coef)

    @staticmethod
    def backward(ctx, grad_out):
        table, triplets, w, scale = ctx.saved_tensors
        model, metric, scale_coef, has_w, has_scale = ctx.cfg
        w = w if has_w else None
        scale = scale if has_scale else None
        gt, gw, gs = ops.model_backward(table, triplets, grad_out, model, metric, w, scale, scale_coef)
        if gw is not None and w is not None:
            gw = gw.reshape(w.shape)
        if gs is not None and scale is not None:
            gs = gs.reshape(scale.shape)
        return (gt if ctx.needs_input_grad[0] else None, None,
                gw if (has_w and metric == "wsum" and ctx.needs_input_grad[2]) else None,
                gs if (has_scale and ctx.needs_input_grad[3]) else None, None, None, None)


def model_forward(table, triplets, model, metric, weights=None, scale=None, scale_coef=1.0):
    if _needs_grad(table, weights, scale):
        return _ModelForwardFn.apply(table, triplets, weights, scale, model, metric, scale_coef)
    return ops.model_forward(table, triplets, model, metric, weights, scale, scale_coef)


class _SiegelVvdFn(torch.autograd.Function):
    """The ascending vector-valued distance v [b, n] of pre-gathered points with the analytic backward (sympa_siegel_vvd_bwd)."""

    @staticmethod
    def forward(ctx, z1, z2, model):
        ctx.save_for_backward(z1, z2)
        ctx.model = model
        return ops.siegel_dist_forward(z1, z2, model, "riem", return_vvd=True)[1]

    @staticmethod
    def backward(ctx, grad_v):
        z1, z2 = ctx.saved_tensors
        g1, g2 = ops.siegel_vvd_backward(z1, z2, grad_v, ctx.model)
        return (g1 if ctx.needs_input_grad[0] else None, g2 if ctx.needs_input_grad[1] else None, None)


def siegel_vvd(z1, z2, model):
    """v [b, n], ascending; differentiable with respect to both points.  Any function of v is a metric, e.g. an lp norm:
        v = siegel_vvd(z1, z2, "upper");  d = v.pow(3).sum(-1).pow(1 / 3)"""
    if _needs_grad(z1, z2):
        return _SiegelVvdFn.apply(z1, z2, model)
    return ops.siegel_dist_forward(z1, z2, model, "riem", return_vvd=True)[1]


class _ModelVvdFn(torch.autograd.Function):
    """v [b, n] of the pairs of a triplet batch gathered from the table (sympa_model_vvd_forward) with the scatter-add backward
    (sympa_model_vvd_backward) into the dense [N,2,n,n] table gradient."""

    @staticmethod
    def forward(ctx, table, triplets, model):
        ctx.save_for_backward(table, triplets)
        ctx.model = model
        return ops.model_vvd_forward(table, triplets, model)

    @staticmethod
    def backward(ctx, grad_v):
        table, triplets = ctx.saved_tensors
        return ops.model_vvd_backward(table, triplets, grad_v, ctx.model), None, None


def model_vvd(table, triplets, model):
    if _needs_grad(table):
        return _ModelVvdFn.apply(table, triplets, model)
    return ops.model_vvd_forward(table, triplets, model)


class _SpdDistFn(torch.autograd.Function):
    """SymmetricPositiveDefinite.dist(x, y) with the analytic backward (sympa_spd_backward_rows)."""

    @staticmethod
    def forward(ctx, x, y):
        ctx.save_for_backward(x, y)
        return ops.spd_dist_forward(x, y)

    @staticmethod
    def backward(ctx, grad_out):
        x, y = ctx.saved_tensors
        rows, _ = ops.spd_backward_rows(x, y, grad_out=grad_out)
        b = x.shape[0]
        return rows[:b], rows[b:]


def spd_dist(x, y):
    if _needs_grad(x, y):
        return _SpdDistFn.apply(x, y)
    return ops.spd_dist_forward(x, y)


class _SpdModelForwardFn(torch.autograd.Function):
    """Model.forward for the spd model: dense [N, n, n] table gradient = per-pair rows + scatter-add kernel."""

    @staticmethod
    def forward(ctx, table, triplets, scale, scale_coef):
        ctx.save_for_backward(table, triplets, scale if scale is not None else torch.empty(0, device=table.device))
        ctx.cfg = (scale_coef, scale is not None)
        return ops.spd_model_forward(table, triplets, scale, scale_coef)

    @staticmethod
    def backward(ctx, grad_out):
        table, triplets, scale = ctx.saved_tensors
        scale_coef, has_scale = ctx.cfg
        scale = scale if has_scale else None
        gs = torch.zeros(1, dtype=torch.float64, device=table.device) if has_scale else None
        rows, _ = ops.spd_backward_rows(table, table, triplets, grad_out=grad_out, scale=scale, scale_coef=scale_coef,
                                        grad_scale=gs)
        gt = torch.zeros_like(table)
        b = triplets.shape[0]
        idx = torch.cat((triplets[:, 0], triplets[:, 1])).contiguous()
        ops.scatter_add_flat_rows_(gt, rows.reshape(2 * b, -1), idx)
        return (gt if ctx.needs_input_grad[0] else None, None,
                gs.reshape(scale.shape) if (has_scale and ctx.needs_input_grad[2]) else None, None)


def spd_model_forward(table, triplets, scale=None, scale_coef=1.0):
    if _needs_grad(table, scale):
        return _SpdModelForwardFn.apply(table, triplets, scale, scale_coef)
    return ops.spd_model_forward(table, triplets, scale, scale_coef)


class _SpdVvdFn(torch.autograd.Function):
    """The spd model's vector-valued distance v [b, n] (ascending, signed) of pre-gathered points with the analytic backward
    (sympa_spd_vvd_bwd)."""

    @staticmethod
    def forward(ctx, x, y):
        ctx.save_for_backward(x, y)
        return ops.spd_vvd_forward(x, y)

    @staticmethod
    def backward(ctx, grad_v):
        x, y = ctx.saved_tensors
        gx, gy = ops.spd_vvd_backward(x, y, grad_v)
        return (gx if ctx.needs_input_grad[0] else None, gy if ctx.needs_input_grad[1] else None)


def spd_vvd(x, y):
    """v [b, n] = log of the eigenvalues of x^-1 y, ascending; differentiable with respect to both points.  Any function of v is a
    metric:  v.norm(dim=-1) is the affine-invariant distance, v.abs().sum(-1) and v.abs().amax(-1) the Finsler distances."""
    if _needs_grad(x, y):
        return _SpdVvdFn.apply(x, y)
    return ops.spd_vvd_forward(x, y)


class _SpdModelVvdFn(torch.autograd.Function):
    """v [b, n] of the pairs of a triplet batch gathered from the spd table (sympa_spd_model_vvd_forward) with the scatter-add
    backward (sympa_spd_model_vvd_backward) into the dense [N, n, n] table gradient."""

    @staticmethod
    def forward(ctx, table, triplets):
        ctx.save_for_backward(table, triplets)
        return ops.spd_model_vvd_forward(table, triplets)

    @staticmethod
    def backward(ctx, grad_v):
        table, triplets = ctx.saved_tensors
        return ops.spd_model_vvd_backward(table, triplets, grad_v), None


def spd_model_vvd(table, triplets):
    if _needs_grad(table):
        return _SpdModelVvdFn.apply(table, triplets)
    return ops.spd_model_vvd_forward(table, triplets)


class _VectorDistFn(torch.autograd.Function):
    """dist(x, y) of a vector model on [b, dims] rows with the analytic backward (sympa_vector_backward_rows)."""

    @staticmethod
    def forward(ctx, x, y, model):
        ctx.save_for_backward(x, y)
        ctx.model = model
        return ops.vector_dist_forward(x, y, model)

    @staticmethod
    def backward(ctx, grad_out):
        x, y = ctx.saved_tensors
        rows, _ = ops.vector_backward_rows(x, y, ctx.model, grad_out=grad_out)
        b = x.shape[0]
        return rows[:b], rows[b:], None


def vector_dist(x, y, model):
    if _needs_grad(x, y):
        return _VectorDistFn.apply(x, y, model)
    return ops.vector_dist_forward(x, y, model)


class _VectorModelForwardFn(torch.autograd.Function):
    """Model.forward for a vector model: dense [N, dims] table gradient = per-pair rows + the scatter-add kernel."""

    @staticmethod
    def forward(ctx, table, triplets, model, scale, scale_coef):
        ctx.save_for_backward(table, triplets, scale if scale is not None else torch.empty(0, device=table.device))
        ctx.cfg = (model, scale_coef, scale is not None)
        return ops.vector_model_forward(table, triplets, model, scale, scale_coef)

    @staticmethod
    def backward(ctx, grad_out):
        table, triplets, scale = ctx.saved_tensors
        model, scale_coef, has_scale = ctx.cfg
        scale = scale if has_scale else None
        gs = torch.zeros(1, dtype=torch.float64, device=table.device) if has_scale else None
        rows, _ = ops.vector_backward_rows(table, table, model, triplets, grad_out=grad_out, scale=scale, scale_coef=scale_coef,
                                           grad_scale=gs)
        gt = torch.zeros_like(table, memory_format=torch.contiguous_format)
        idx = torch.cat((triplets[:, 0], triplets[:, 1])).contiguous()
        ops.scatter_add_flat_rows_(gt, rows, idx)
        return (gt if ctx.needs_input_grad[0] else None, None, None,
                gs.reshape(scale.shape) if (has_scale and ctx.needs_input_grad[3]) else None, None)


def vector_model_forward(table, triplets, model, scale=None, scale_coef=1.0):
    if _needs_grad(table, scale):
        return _VectorModelForwardFn.apply(table, triplets, model, scale, scale_coef)
    return ops.vector_model_forward(table, triplets, model, scale, scale_coef)
