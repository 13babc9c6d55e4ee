"""Vertex attention — the head of the fork's policy generator SoftGenerator (reference
pygcn/models.py:412-433): a key vector, made by a small MLP from the mean of the trunk's [N, C] result
(SoftGeneratorPoolMLP, :303-312), is multiplied into every vertex's row, and a softmax over the VERTICES
gives the probability of picking each (SoftGeneratorAttention, :324-329):

    attn = softmax_n( sum_c key[c] * h[n, c] )

The fork writes `torch.mul(key, x).sum(dim=1)`: an [N, C] product in forward and two [N, C] gradients in
backward.  Here it is full-height HIP sweeps (pygcn_amd/csrc/gcn_norm.hip) behind ONE autograd node, over
the layout of pool.py — a contiguous [N, C] tensor, or the [k, N, C] permuted view of contiguous [N, k*C]
storage with one key per sample, read in place:

    forward    gcn_attn_scores      reads h          -> fp32 scores [k, N], double (max, sum exp) [k, 2]
               gcn_attn_normalize   [k, N] floats    -> attn, in place of the scores
    backward   gcn_attn_backward    reads h, ds      -> writes dh = ds[n] * key, double dkey [k*C]

ds = attn * (g - sum_n g * attn) is elementwise and reduction work on [k, N] floats, 1/C of a sweep's bytes:
torch ops inside the node.  Nothing synchronises with the host.
"""
import torch

from . import _native
from .norm import _DTYPES
from .pool import _wide_storage, masked_mean_pool


def attn_scores(h, key, n, k, c):
    """(scores fp32 [k, n], stats double [k, 2] = (max, sum exp(s - max))) over storage [n, k*C] starting
    at h.data_ptr(); `key` fp32 [k*C]."""
    dt = _DTYPES[h.dtype]
    scores = torch.empty((k, n), dtype=torch.float32, device=h.device)
    stats = torch.empty((k, 2), dtype=torch.float64, device=h.device)
    _native.launch("gcn_attn_scores", h.device, dt, h.data_ptr(), key.data_ptr(), n, c, k, scores.data_ptr(),
                   stats.data_ptr(), workspace=_native.lib().gcn_attn_workspace_bytes(n, c, k, dt))
    return scores, stats


def attn_normalize(scores, stats, out=None):
    """fp32 [k, n]: exp(scores - max) / sum, into `out` (default: in place of the scores)."""
    k, n = scores.shape
    out = scores if out is None else out
    _native.launch("gcn_attn_normalize", scores.device, scores.data_ptr(), stats.data_ptr(), out.data_ptr(), n, k)
    return out


def attn_backward(h, ds, key, n, k, c, need_dh=True):
    """(dh [n, k*C] of h's dtype or None, dkey double [k*C]) for ds fp32 [k, n]."""
    dt = _DTYPES[h.dtype]
    dh = torch.empty((n, k * c), dtype=h.dtype, device=h.device) if need_dh else None
    dkey = torch.empty(k * c, dtype=torch.float64, device=h.device)
    _native.launch("gcn_attn_backward", h.device, dt, h.data_ptr(), ds.data_ptr(), key.data_ptr(),
                   dh.data_ptr() if need_dh else None, dkey.data_ptr(), n, c, k,
                   workspace=_native.lib().gcn_attn_workspace_bytes(n, c, k, dt))
    return dh, dkey


class VertexAttentionFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, key, n, k, c):
        key32 = key.detach().to(torch.float32).contiguous().view(k * c)
        scores, stats = attn_scores(h, key32, n, k, c)
        attn = attn_normalize(scores, stats)
        ctx.dims, ctx.h_dim, ctx.key_like = (n, k, c), h.dim(), (key.shape, key.dtype)
        ctx.save_for_backward(h, key32, attn)
        ctx.set_materialize_grads(True)
        out = attn.to(h.dtype)
        return out.view(n) if h.dim() == 2 else out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        h, key32, attn = ctx.saved_tensors
        n, k, c = ctx.dims
        g32 = g.to(torch.float32).reshape(k, n)
        t = (g32 * attn).sum(1, keepdim=True, dtype=torch.float64).to(torch.float32)
        ds = (attn * (g32 - t)).contiguous()
        dh, dkey = attn_backward(h, ds, key32, n, k, c, need_dh=ctx.needs_input_grad[0])
        if dh is not None and ctx.h_dim == 3:
            dh = dh.view(n, k, c).permute(1, 0, 2)
        shape, dtype = ctx.key_like
        dkey = dkey.to(dtype).view(shape) if ctx.needs_input_grad[1] else None
        return dh, dkey, None, None, None


def _literal(h, key):
    return torch.softmax((h * (key if h.dim() == 2 else key.unsqueeze(-2))).sum(-1), dim=-1)


def vertex_attention(h, key):
    """`softmax((h * key).sum(-1), dim=-1)`: the probability of every vertex under one key per sample — the
    fork's SoftGeneratorAttention (reference pygcn/models.py:324-329).

    h [N, C] with key [C] or [1, C] -> [N]; h [k, N, C] with key [k, C] -> [k, N].  The result has h's dtype
    (bf16: rounded once from the fp32 value); gradients go to `h` and to `key`, in their own dtypes and shapes.

    On the HIP device, for fp32 / bf16 `h` that is a contiguous [N, C] tensor or the [k, N, C] permuted view
    of contiguous [N, k*C] storage (what GCNBatchNorm returns for a batched input), with C a multiple of the
    16-byte lane width v (4 fp32 / 8 bf16) and C/v dividing 256, and a floating `key` on the same device,
    this is one autograd node over HIP sweeps that read `h` in place; any other layout, width, dtype or
    device takes the torch composition above."""
    if h.dim() == 2:
        ok = key.dim() in (1, 2) and key.numel() == h.shape[1] and key.shape[-1] == h.shape[1]
    else:
        ok = h.dim() == 3 and tuple(key.shape) == (h.shape[0], h.shape[2])
    if not ok:
        raise RuntimeError(f"vertex_attention: h {tuple(h.shape)} does not go with key {tuple(key.shape)}")
    dims = _wide_storage(h) if (key.device == h.device and key.dtype in _DTYPES) else None
    if dims is None:
        return _literal(h, key)
    return VertexAttentionFunction.apply(h, key, *dims)


def vertex_mean(h):
    """The mean over the vertices, [1, C] for h [N, C] (the fork's `torch.mean(x, dim=0).unsqueeze(0)`,
    reference pygcn/models.py:304) and [k, C] for h [k, N, C].  On the layouts `vertex_attention` takes it
    runs through the pool node (`masked_mean_pool` with an all-ones mask and count = N: one read sweep,
    double sums in a fixed order); anything else is `h.mean(-2)`."""
    if h.dim() not in (2, 3):
        raise RuntimeError(f"vertex_mean: h {tuple(h.shape)} is neither [N, C] nor [k, N, C]")
    if _wide_storage(h) is None:
        return h.mean(-2, keepdim=h.dim() == 2)
    ones = torch.ones(h.shape[:-1], dtype=torch.float32, device=h.device)
    # (the count as a tensor FILLED on the device: a Python number would reach it by a host-to-device copy,
    #  which synchronises the stream)
    return masked_mean_pool(h, ones, count=torch.full((1,), float(h.shape[-2]), dtype=torch.float32, device=h.device))
