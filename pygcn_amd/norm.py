"""ReLU + training-mode BatchNorm over the vertices, as the fork's live model applies it after its
first two layers (reference pygcn/models.py:49,53 `self.apply_bn(F.relu(self.gc1(x, adj)))`, with
apply_bn = `nn.BatchNorm1d(x.size()[1]).cuda()(x)`, :41-45) — four full-height HIP sweeps
(pygcn_amd/csrc/gcn_norm.hip) behind ONE autograd node:

    forward    gcn_bn_stats           reads z            -> mean, var, rstd     (fp32 [F], on the device)
               gcn_bn_apply           reads z, writes y
    backward   gcn_bn_backward_sums   reads g, z         -> sum g (= dbeta), sum g * xhat (= dgamma), coef
               gcn_bn_backward_apply  reads g, z, writes dz   (in double, from the double [4, F] coef)

The ReLU and its backward mask ride in the loads, xhat is recomputed from the saved z, the sums are
deterministic (carried in double, added in block order) and nothing synchronises with the host.

`batch=k`: z is [n, k*F], k samples over the same vertices side by side (GraphConvolution's batched
layout; the fork loops over its samples, reference pygcn/models.py:343-349), each normalised on its
own: the same four sweeps, once each, over k column windows of width F (gcn_bn_*_batched) — a
window's result is bitwise the 2-D call's on a contiguous copy of the window.
"""
import torch
import torch.nn.functional as F

from . import _native
from .graph import _require_cuda

_DTYPES = {torch.float32: _native.GCN_DTYPE_F32, torch.bfloat16: _native.GCN_DTYPE_BF16}


def supported(z, batch=1):
    """True when the HIP sweeps take `z`: a contiguous 2-D fp32 / bf16 tensor on the HIP device of
    `batch` column windows whose width F = z.shape[1] / batch is a multiple of the 16-byte lane width
    v (4 fp32 / 8 bf16) with F/v dividing 256."""
    return (isinstance(z, torch.Tensor) and z.is_cuda and z.dim() == 2 and z.dtype in _DTYPES
            and z.is_contiguous() and batch >= 1 and z.shape[1] % batch == 0
            and _native.lib().gcn_bn_batched_workspace_bytes(max(z.shape[0], 2), z.shape[1] // batch, batch,
                                                             _DTYPES[z.dtype]) != 0)


def _columns(n, device):
    return torch.empty(n, dtype=torch.float32, device=device)


def _window(z, batch):
    n, width = z.shape
    if batch < 1 or width % batch:
        raise RuntimeError(f"{width} columns are not {batch} windows of equal width")
    return n, width // batch, _DTYPES[z.dtype]


def bn_stats(z, relu=True, eps=1e-5, batch=1):
    """(mean, biased var, rstd = 1/sqrt(var + eps)) of the columns of relu(z) (or z): fp32 [batch*F]."""
    _require_cuda(z, "z")
    n, nf, dt = _window(z, batch)
    mean, var, rstd = (_columns(z.shape[1], z.device) for _ in range(3))
    _native.launch("gcn_bn_stats_batched", z.device, dt, z.data_ptr(), n, nf, batch, int(relu), float(eps),
                   mean.data_ptr(), var.data_ptr(), rstd.data_ptr(),
                   workspace=_native.lib().gcn_bn_batched_workspace_bytes(n, nf, batch, dt))
    return mean, var, rstd


def bn_apply(z, mean, rstd, gamma=None, beta=None, relu=True, batch=1):
    """y = (relu(z) - mean) * rstd * gamma + beta (gamma, beta: fp32 [batch*F] or None)."""
    n, nf, dt = _window(z, batch)
    y = torch.empty_like(z)
    _native.launch("gcn_bn_apply_batched", z.device, dt, z.data_ptr(), y.data_ptr(), n, nf, batch, int(relu),
                   mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr() if gamma is not None else None,
                   beta.data_ptr() if beta is not None else None)
    return y


def bn_backward_sums(g, z, mean, relu=True, eps=1e-5, batch=1):
    """(sum_r g, sum_r g * xhat, coef): the gradients of beta and gamma, fp32 [batch*F], and the double
    [4, batch*F] columns (mean, rstd, sum_g / n, rstd^2 * sum g (x - mean) / n) that bn_backward_apply
    evaluates dz from — `mean` (fp32, of bn_stats) is only the centre the sums are taken about."""
    n, nf, dt = _window(z, batch)
    sum_g, sum_gxhat = _columns(z.shape[1], z.device), _columns(z.shape[1], z.device)
    coef = torch.empty(4, z.shape[1], dtype=torch.float64, device=z.device)
    _native.launch("gcn_bn_backward_sums_batched", z.device, dt, g.data_ptr(), z.data_ptr(), n, nf, batch, int(relu),
                   float(eps), mean.data_ptr(), sum_g.data_ptr(), sum_gxhat.data_ptr(), coef.data_ptr(),
                   workspace=_native.lib().gcn_bn_batched_workspace_bytes(n, nf, batch, dt))
    return sum_g, sum_gxhat, coef


def bn_backward_apply(g, z, coef, gamma=None, relu=True, batch=1):
    """dz = [z > 0] * gamma * rstd * (g - sum_g / n - xhat * sum_gxhat / n), in double from `coef`."""
    n, nf, dt = _window(z, batch)
    dz = torch.empty_like(z)
    _native.launch("gcn_bn_backward_apply_batched", z.device, dt, g.data_ptr(), z.data_ptr(), dz.data_ptr(), n, nf,
                   batch, int(relu), gamma.data_ptr() if gamma is not None else None, coef.data_ptr())
    return dz


class ReluBatchNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, weight, bias, eps, relu, batch=1):
        # one BatchNorm1d applied to every sample in turn: its [F] parameters repeat over the windows
        gamma = weight.detach().float().repeat(batch).contiguous() if weight is not None else None
        beta = bias.detach().float().repeat(batch).contiguous() if bias is not None else None
        mean, _, rstd = bn_stats(z, relu, eps, batch)
        ctx.relu, ctx.eps, ctx.batch = bool(relu), float(eps), int(batch)
        ctx.has_weight = weight is not None
        ctx.param_dtypes = (weight.dtype if weight is not None else None, bias.dtype if bias is not None else None)
        # rstd is not saved: the backward sums recover it, with the mean's rounding error, in double
        ctx.save_for_backward(z, mean, *([gamma] if gamma is not None else []))
        return bn_apply(z, mean, rstd, gamma, beta, relu, batch)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        z, mean = ctx.saved_tensors[:2]
        gamma = ctx.saved_tensors[2] if ctx.has_weight else None
        g = g.to(z.dtype).contiguous()
        sum_g, sum_gxhat, coef = bn_backward_sums(g, z, mean, ctx.relu, ctx.eps, ctx.batch)
        dz = bn_backward_apply(g, z, coef, gamma, ctx.relu, ctx.batch) if ctx.needs_input_grad[0] else None
        if ctx.batch > 1:       # the shared parameters collect every window's sums
            sum_g, sum_gxhat = sum_g.view(ctx.batch, -1).sum(0), sum_gxhat.view(ctx.batch, -1).sum(0)
        dw = sum_gxhat.to(ctx.param_dtypes[0]) if ctx.needs_input_grad[1] else None
        db = sum_g.to(ctx.param_dtypes[1]) if ctx.needs_input_grad[2] else None
        return dz, dw, db, None, None, None


def relu_batch_norm(z, weight=None, bias=None, eps=1e-5, relu=True, batch=1):
    """`F.batch_norm(torch.relu(z), None, None, weight, bias, True, 0.0, eps)` — BatchNorm1d in
    training mode (batch statistics over the rows of z [n, F], biased variance, no running
    statistics) of relu(z) (`relu=False`: of z itself) — as one autograd node over the HIP sweeps
    when `supported(z)`, and as that literal torch composition otherwise.  Gradients for z, weight
    and bias; n < 2 raises torch's ValueError.

    `batch=k`: z is [n, k*F] — k samples side by side, each normalised on its own with the SAME
    weight / bias [F] (one BatchNorm1d applied to each sample in turn: per-column BatchNorm of z with
    the parameters repeated k times, their gradients summed over the samples).  Still one node and one
    launch per sweep when `supported(z, k)` — F, not k*F, obeys the width rule; otherwise
    `F.batch_norm(relu(z), None, None, weight.repeat(k), bias.repeat(k), True, 0.0, eps)`."""
    batch = int(batch)
    if batch < 1 or (batch > 1 and (z.dim() != 2 or z.shape[1] % batch)):
        raise RuntimeError(f"relu_batch_norm: z must be [n, batch*F], got {tuple(z.shape)} with batch={batch}")
    if not supported(z, batch):
        if batch > 1:
            weight = weight.repeat(batch) if weight is not None else None
            bias = bias.repeat(batch) if bias is not None else None
        return F.batch_norm(torch.relu(z) if relu else z, None, None, weight, bias, True, 0.0, eps)
    if z.shape[0] < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {z.size()}")
    nf = z.shape[1] // batch
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None and (t.device != z.device or t.shape != (nf,)):
            raise RuntimeError(f"relu_batch_norm: {name} must be a [{nf}] tensor on {z.device}, "
                               f"got {tuple(t.shape)} on {t.device}")
    return ReluBatchNormFunction.apply(z, weight, bias, float(eps), bool(relu), batch)
