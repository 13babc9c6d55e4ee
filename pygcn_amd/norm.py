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
"""
import torch
import torch.nn.functional as F

from . import _native
from .graph import _require_cuda

_DTYPES = {torch.float32: _native.GCN_DTYPE_F32, torch.bfloat16: _native.GCN_DTYPE_BF16}


def supported(z):
    """True when the HIP sweeps take `z`: a contiguous 2-D fp32 / bf16 tensor on the HIP device whose
    width F is a multiple of the 16-byte lane width v (4 fp32 / 8 bf16) with F/v dividing 256."""
    return (isinstance(z, torch.Tensor) and z.is_cuda and z.dim() == 2 and z.dtype in _DTYPES
            and z.is_contiguous()
            and _native.lib().gcn_bn_workspace_bytes(max(z.shape[0], 2), z.shape[1], _DTYPES[z.dtype]) != 0)


def _columns(n, device):
    return torch.empty(n, dtype=torch.float32, device=device)


def bn_stats(z, relu=True, eps=1e-5):
    """(mean, biased var, rstd = 1/sqrt(var + eps)) of the columns of relu(z) (or z): fp32 [F]."""
    _require_cuda(z, "z")
    n, nf = z.shape
    dt = _DTYPES[z.dtype]
    mean, var, rstd = (_columns(nf, z.device) for _ in range(3))
    _native.launch("gcn_bn_stats", z.device, dt, z.data_ptr(), n, nf, int(relu), float(eps), mean.data_ptr(),
                   var.data_ptr(), rstd.data_ptr(), workspace=_native.lib().gcn_bn_workspace_bytes(n, nf, dt))
    return mean, var, rstd


def bn_apply(z, mean, rstd, gamma=None, beta=None, relu=True):
    """y = (relu(z) - mean) * rstd * gamma + beta (gamma, beta: fp32 [F] or None)."""
    n, nf = z.shape
    y = torch.empty_like(z)
    _native.launch("gcn_bn_apply", z.device, _DTYPES[z.dtype], z.data_ptr(), y.data_ptr(), n, nf, int(relu),
                   mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr() if gamma is not None else None,
                   beta.data_ptr() if beta is not None else None)
    return y


def bn_backward_sums(g, z, mean, relu=True, eps=1e-5):
    """(sum_r g, sum_r g * xhat, coef): the gradients of beta and gamma, fp32 [F], and the double
    [4, F] columns (mean, rstd, sum_g / n, rstd^2 * sum g (x - mean) / n) that bn_backward_apply
    evaluates dz from — `mean` (fp32, of bn_stats) is only the centre the sums are taken about."""
    n, nf = z.shape
    dt = _DTYPES[z.dtype]
    sum_g, sum_gxhat = _columns(nf, z.device), _columns(nf, z.device)
    coef = torch.empty(4, nf, dtype=torch.float64, device=z.device)
    _native.launch("gcn_bn_backward_sums", z.device, dt, g.data_ptr(), z.data_ptr(), n, nf, int(relu), float(eps),
                   mean.data_ptr(), sum_g.data_ptr(), sum_gxhat.data_ptr(), coef.data_ptr(),
                   workspace=_native.lib().gcn_bn_workspace_bytes(n, nf, dt))
    return sum_g, sum_gxhat, coef


def bn_backward_apply(g, z, coef, gamma=None, relu=True):
    """dz = [z > 0] * gamma * rstd * (g - sum_g / n - xhat * sum_gxhat / n), in double from `coef`."""
    n, nf = z.shape
    dz = torch.empty_like(z)
    _native.launch("gcn_bn_backward_apply", z.device, _DTYPES[z.dtype], g.data_ptr(), z.data_ptr(), dz.data_ptr(),
                   n, nf, int(relu), gamma.data_ptr() if gamma is not None else None, coef.data_ptr())
    return dz


class ReluBatchNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, weight, bias, eps, relu):
        gamma = weight.detach().float().contiguous() if weight is not None else None
        beta = bias.detach().float().contiguous() if bias is not None else None
        mean, _, rstd = bn_stats(z, relu, eps)
        ctx.relu, ctx.eps = bool(relu), float(eps)
        ctx.has_weight = weight is not None
        ctx.param_dtypes = (weight.dtype if weight is not None else None, bias.dtype if bias is not None else None)
        # rstd is not saved: the backward sums recover it, with the mean's rounding error, in double
        ctx.save_for_backward(z, mean, *([gamma] if gamma is not None else []))
        return bn_apply(z, mean, rstd, gamma, beta, relu)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        z, mean = ctx.saved_tensors[:2]
        gamma = ctx.saved_tensors[2] if ctx.has_weight else None
        g = g.to(z.dtype).contiguous()
        sum_g, sum_gxhat, coef = bn_backward_sums(g, z, mean, ctx.relu, ctx.eps)
        dz = bn_backward_apply(g, z, coef, gamma, ctx.relu) if ctx.needs_input_grad[0] else None
        dw = sum_gxhat.to(ctx.param_dtypes[0]) if ctx.needs_input_grad[1] else None
        db = sum_g.to(ctx.param_dtypes[1]) if ctx.needs_input_grad[2] else None
        return dz, dw, db, None, None


def relu_batch_norm(z, weight=None, bias=None, eps=1e-5, relu=True):
    """`F.batch_norm(torch.relu(z), None, None, weight, bias, True, 0.0, eps)` — BatchNorm1d in
    training mode (batch statistics over the rows of z [n, F], biased variance, no running
    statistics) of relu(z) (`relu=False`: of z itself) — as one autograd node over the HIP sweeps
    when `supported(z)`, and as that literal torch composition otherwise.  Gradients for z, weight
    and bias; n < 2 raises torch's ValueError."""
    if not supported(z):
        return F.batch_norm(torch.relu(z) if relu else z, None, None, weight, bias, True, 0.0, eps)
    if z.shape[0] < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {z.size()}")
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None and (t.device != z.device or t.shape != (z.shape[1],)):
            raise RuntimeError(f"relu_batch_norm: {name} must be a [{z.shape[1]}] tensor on {z.device}, "
                               f"got {tuple(t.shape)} on {t.device}")
    return ReluBatchNormFunction.apply(z, weight, bias, float(eps), bool(relu))
