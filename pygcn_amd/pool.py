"""Masked mean pool over the vertices — the readout of the fork's evaluator GCN_OVER_MLP (reference
pygcn/models.py:341-355): every sample's GCN output [N, C] is multiplied by a 0/1 vertex mask, summed
over the vertices and divided by a vertex count (PoolLayer, :267-286), and the [k, C] result goes to a
small MLP.

    out[j, c] = sum_n mask[j, n] * h[j, n, c] / count[j]

Two full-height HIP sweeps (pygcn_amd/csrc/gcn_norm.hip) behind ONE autograd node, over the layout
GCNBatchNorm returns its batched result in — the [k, N, C] permuted view of contiguous [N, k*C]
storage, read in place:

    forward    gcn_masked_colsum      reads h            -> double [k*C] sums (fixed order, reproducible)
    backward   gcn_masked_broadcast   writes dh = mask[j, n] * (g[j, c] / count[j])
               gcn_attn_scores        (mask_grad=True only) reads h -> dmask[j, n] = sum_c h[j, n, c] * g[j, c] / count[j]

The division by the count and the [k*C] coefficient vector are torch ops on [k, C] tensors; nothing
synchronises with the host.
"""
import torch

from . import _native
from .norm import _DTYPES


def _wide_storage(h):
    """(n, k, C) when `h` is a contiguous [N, C] tensor or the [k, N, C] permuted view of contiguous
    [N, k*C] storage, on the HIP device, of a dtype and width the sweeps take; else None."""
    if not (isinstance(h, torch.Tensor) and h.is_cuda and h.dtype in _DTYPES and h.dim() in (2, 3)
            and h.numel() > 0 and h.data_ptr() % 16 == 0):
        return None
    if h.dim() == 2:
        n, k, c = h.shape[0], 1, h.shape[1]
        if not h.is_contiguous():
            return None
    else:
        k, n, c = h.shape
        if h.stride(2) != 1 or (n > 1 and h.stride(1) != k * c) or (k > 1 and h.stride(0) != c):
            return None
    if _native.lib().gcn_pool_workspace_bytes(n, c, k, _DTYPES[h.dtype]) == 0:
        return None
    return n, k, c


def masked_colsum(h, mask_kn, n, k, c):
    """double [k*C]: sum_r mask_kn[j, r] * h[r, j*C + c] over storage [n, k*C] starting at h.data_ptr()."""
    dt = _DTYPES[h.dtype]
    sums = torch.empty(k * c, dtype=torch.float64, device=h.device)
    _native.launch("gcn_masked_colsum", h.device, dt, h.data_ptr(), mask_kn.data_ptr(), n, c, k, sums.data_ptr(),
                   workspace=_native.lib().gcn_pool_workspace_bytes(n, c, k, dt))
    return sums


def masked_broadcast(mask_kn, coef, n, k, c, dtype):
    """[n, k*C] of `dtype`: mask_kn[j, r] * coef[j*C + c]."""
    dh = torch.empty((n, k * c), dtype=dtype, device=coef.device)
    _native.launch("gcn_masked_broadcast", coef.device, _DTYPES[dtype], mask_kn.data_ptr(), coef.data_ptr(),
                   dh.data_ptr(), n, c, k)
    return dh


def masked_rowdot(h, coef, n, k, c):
    """fp32 [k, n]: sum_c h[r, j*C + c] * coef[j*C + c] over storage [n, k*C] starting at h.data_ptr() — the
    per-vertex dot product of the attention scores (gcn_attn_scores with key = coef; its softmax statistics
    are not used)."""
    dt = _DTYPES[h.dtype]
    dots = torch.empty((k, n), dtype=torch.float32, device=h.device)
    stats = torch.empty((k, 2), dtype=torch.float64, device=h.device)
    _native.launch("gcn_attn_scores", h.device, dt, h.data_ptr(), coef.data_ptr(), n, c, k, dots.data_ptr(),
                   stats.data_ptr(), workspace=_native.lib().gcn_attn_workspace_bytes(n, c, k, dt))
    return dots


class MaskedMeanPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, mask_kn, count, n, k, c, mask_grad=False):
        ctx.dims, ctx.h_dim = (n, k, c), h.dim()
        ctx.mask_grad = bool(mask_grad)
        ctx.save_for_backward(mask_kn, count, *([h] if mask_grad else []))
        ctx.set_materialize_grads(True)
        sums = masked_colsum(h, mask_kn, n, k, c).view(k, c)
        return (sums / count.double().view(-1, 1)).to(h.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        mask_kn, count = ctx.saved_tensors[:2]
        n, k, c = ctx.dims
        coef = (g.float() / count.view(-1, 1)).contiguous().view(k * c)
        dh = None
        if ctx.needs_input_grad[0]:
            dh = masked_broadcast(mask_kn, coef, n, k, c, g.dtype)
            dh = dh if ctx.h_dim == 2 else dh.view(n, k, c).permute(1, 0, 2)
        dmask = None
        if ctx.mask_grad and ctx.needs_input_grad[1]:
            dmask = masked_rowdot(ctx.saved_tensors[2], coef, n, k, c)          # fp32 [k, N], as mask_kn
        return dh, dmask, None, None, None, None, None


def masked_mean_pool(h, mask, count=None, mask_grad=False):
    """`(h * mask[:, :, None]).sum(1) / count[:, None]` -> [k, C]: the fork's PoolLayer (reference
    pygcn/models.py:267-286) for all k samples at once.

    h [k, N, C] with mask [k, N], or h [N, C] with mask [N] (k = 1); `mask` in float.  `count`: a
    number, a 0-d tensor or a [k] tensor; by default the number of non-zero entries of mask[j],
    computed on the device.  The fork divides every sample by the count of sample 0:
    `count=(mask[0] != 0).sum()`.  The mask multiplies (a NaN under a zero mask stays NaN), a zero
    count gives what torch's division gives, `mask` and `count` get no gradient.

    `mask_grad=True`: the mask is an input like `h` and receives sum_c h[j, n, c] * g[j, c] / count[j] — what
    the fork's evaluator hands back to a generator through the vertex flag (reference
    pygcn/policy-generator.py:398-420).  `count` never gets a gradient.

    On the HIP device, for fp32 / bf16 `h` that is the [k, N, C] permuted view of contiguous [N, k*C]
    storage (what GCNBatchNorm returns for a batched input) or a contiguous [N, C] tensor, with C a
    multiple of the 16-byte lane width v (4 fp32 / 8 bf16) and C/v dividing 256, this is one autograd
    node over two HIP sweeps that read `h` in place (with `mask_grad`, a third: the per-vertex dot product
    of gcn_attn_scores with key = g / count); any other layout, width or device takes the torch composition
    above."""
    if h.dim() == 2:
        if mask.dim() != 1:
            raise RuntimeError("masked_mean_pool: h [N, C] takes mask [N]")
        mask = mask.unsqueeze(0)
    if h.dim() not in (2, 3) or mask.dim() != 2 or tuple(mask.shape) != ((1,) if h.dim() == 2 else (h.shape[0],)) \
            + (h.shape[-2],):
        raise RuntimeError(f"masked_mean_pool: h {tuple(h.shape)} does not go with mask {tuple(mask.shape)}")
    if not mask_grad:
        mask = mask.detach()
    if count is None:
        count = (mask.detach() != 0).sum(1)
    count = torch.as_tensor(count, device=h.device).detach()
    dims = _wide_storage(h) if mask.device == h.device else None
    if dims is None:
        h3 = h.unsqueeze(0) if h.dim() == 2 else h
        return (h3 * mask.to(h.dtype).unsqueeze(2)).sum(1) / count.to(h.dtype).reshape(-1, 1)
    n, k, c = dims
    mask_kn = mask.to(torch.float32).contiguous()                    # [k, N] as given: k*N floats, no transpose
    count = count.to(torch.float32).reshape(-1).expand(k).contiguous()
    if mask_grad:
        return MaskedMeanPoolFunction.apply(h, mask_kn, count, n, k, c, True)
    return MaskedMeanPoolFunction.apply(h, mask_kn, count, n, k, c)
