"""ReLU + training-mode BatchNorm folded into the NEXT layer's X·W, for the 32-wide layers of the fork's live
model (reference pygcn/models.py:49-56: `x = apply_bn(F.relu(gc1(x, adj)))` feeds `gc2`'s
`torch.mm(input, self.weight)`, pygcn/layers.py:33) — HIP sweeps (pygcn_amd/csrc/gcn_normlin.hip) behind ONE
autograd node that never forms the normalised activation:

    forward    gcn_bn_stats_batched          reads z           -> mean, rstd       (fp32 [k·32], on the device)
               gcn_bn_linear_forward         reads z, writes s = BN(relu(z)) · W
    backward   gcn_bn_linear_backward_sums   reads dS, z       -> grad_W, coef     (double [4, k·32])
               gcn_bn_linear_backward_apply  reads dS, z, writes dz                (skipped when z needs no gradient)

The node saves z, W, mean and rstd; y = BN(relu(z)) and dy = dS·Wᵀ exist in registers only.  Sums are deterministic
(fp32 over one wavefront's slab at most, then double in a fixed order) and nothing synchronises with the host.
"""
import torch

from . import _native
from .gemm import DenseMMFunction
from .norm import bn_stats, relu_batch_norm

WIDTH = 32        # the one width the sweeps are built for


def supported(z, weight, batch=1):
    """True when the HIP sweeps take the call: z [n, batch·32] and weight [32, 32], both contiguous fp32 on the
    same HIP device, n >= 2, and a non-zero gcn_bn_linear_workspace_bytes."""
    if not (isinstance(z, torch.Tensor) and isinstance(weight, torch.Tensor) and z.is_cuda
            and weight.device == z.device and z.dim() == 2 and weight.dim() == 2
            and z.dtype == torch.float32 and weight.dtype == torch.float32
            and z.is_contiguous() and weight.is_contiguous() and batch >= 1 and z.shape[1] % batch == 0
            and z.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0):
        return False
    fin, fout = weight.shape
    return (z.shape[1] // batch == fin
            and _native.lib().gcn_bn_linear_workspace_bytes(z.shape[0], fin, fout, batch) != 0)


class ReluBatchNormLinearFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, weight, eps, relu, batch):
        n = z.shape[0]
        fin, fout = weight.shape
        w = weight.detach()
        mean, _, rstd = bn_stats(z, relu, eps, batch)
        s = torch.empty((n, batch * fout), dtype=torch.float32, device=z.device)
        _native.launch("gcn_bn_linear_forward", z.device, z.data_ptr(), w.data_ptr(), mean.data_ptr(),
                       rstd.data_ptr(), s.data_ptr(), n, fin, fout, batch, int(relu))
        ctx.eps, ctx.relu, ctx.batch = float(eps), bool(relu), int(batch)
        ctx.save_for_backward(z, w, mean, rstd)
        return s

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        z, w, mean, rstd = ctx.saved_tensors
        n = z.shape[0]
        fin, fout = w.shape
        g = g.to(torch.float32).contiguous()
        grad_w = torch.empty_like(w)
        coef = torch.empty(4, z.shape[1], dtype=torch.float64, device=z.device)
        _native.launch("gcn_bn_linear_backward_sums", z.device, g.data_ptr(), z.data_ptr(), w.data_ptr(),
                       mean.data_ptr(), rstd.data_ptr(), n, fin, fout, ctx.batch, int(ctx.relu), ctx.eps,
                       grad_w.data_ptr(), coef.data_ptr(),
                       workspace=_native.lib().gcn_bn_linear_workspace_bytes(n, fin, fout, ctx.batch))
        dz = None
        if ctx.needs_input_grad[0]:
            dz = torch.empty_like(z)
            _native.launch("gcn_bn_linear_backward_apply", z.device, g.data_ptr(), z.data_ptr(), w.data_ptr(),
                           coef.data_ptr(), dz.data_ptr(), n, fin, fout, ctx.batch, int(ctx.relu))
        return dz, (grad_w if ctx.needs_input_grad[1] else None), None, None, None


def _composition(z, weight, eps, relu, batch):
    n = z.shape[0]
    fin, fout = weight.shape
    y = relu_batch_norm(z, eps=eps, relu=relu, batch=batch)
    return DenseMMFunction.apply(y.reshape(n * batch, fin), weight).view(n, batch * fout)


def relu_batch_norm_linear(z, weight, eps=1e-5, relu=True, batch=1):
    """`F.batch_norm(relu(z_j), None, None, None, None, True, 0.0, eps) @ weight` for each of the `batch` column
    windows z_j = z[:, j·Fin:(j+1)·Fin] of z [n, batch·Fin] (k samples side by side, `relu_batch_norm(batch=k)`'s
    layout), the results side by side as [n, batch·Fout]; weight is [Fin, Fout] (GraphConvolution's).  The fork's
    BatchNorm is fresh on every call: no affine parameters.  `relu=False` normalises z itself.

    Inside the rule (`supported`: contiguous fp32 on the HIP device, Fin = Fout = 32, n >= 2) this is one autograd
    node over the sweeps of pygcn_amd/csrc/gcn_normlin.hip, with gradients for z and weight: the normalised
    activation is never written, the node keeps z, weight and the [batch·Fin] statistics, and a window's result
    is bitwise the batch = 1 call's on a contiguous copy of the window.  Everything else is the literal
    composition `DenseMMFunction.apply(relu_batch_norm(z, batch=k).reshape(n·k, Fin), weight).view(n, k·Fout)`."""
    batch = int(batch)
    if z.dim() != 2 or weight.dim() != 2 or batch < 1 or z.shape[1] != batch * weight.shape[0]:
        raise RuntimeError(f"relu_batch_norm_linear: z must be [n, batch*Fin] and weight [Fin, Fout], got "
                           f"{tuple(z.shape)} and {tuple(weight.shape)} with batch={batch}")
    if not supported(z, weight, batch):
        return _composition(z, weight, eps, relu, batch)
    return ReluBatchNormLinearFunction.apply(z, weight, float(eps), bool(relu), batch)
