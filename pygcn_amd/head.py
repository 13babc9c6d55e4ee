"""The per-vertex score head of the fork's Generator and Hierarchical_Generator (reference pygcn/models.py:368-370,
:391-393, the two MLPs :195-241) as fused HIP sweeps (pygcn_amd/csrc/gcn_head.hip) behind ONE autograd node:

    score = linear3( bn(relu( linear2( bn(relu( linear1( cat(h, x[:, d : F - skip_last]) ))) )) ))      [N, 1]

The tail of x is read in place — the [N, C + T] concatenation never exists — and the hidden activations are
recomputed in every sweep instead of being stored: the node saves h, x, the six parameters and the four statistics
vectors, nothing of size [N, H].

    forward    gcn_vmlp_forward    3 sweeps with BatchNorm (statistics of layer 1, of layer 2, the score), 1 without
    backward   gcn_vmlp_backward   3 sweeps with BatchNorm, 1 without: dh and the six parameter gradients

Column sums are carried in double and added in a fixed order: no float atomics, bitwise reproducible, and nothing
synchronises with the host.
"""
import torch

from . import _native
from .norm import relu_batch_norm

_STATS = 4 * 64       # mean1, rstd1, mean2, rstd2 at the pitch of include/gcn_spmm.h


def _layers(mlp):
    return mlp.linear1, mlp.linear2, mlp.linear3


def supported(h, x, d, mlp, skip_last=0):
    """True when the HIP sweeps take the call: h [N, C] and x [N, F] contiguous fp32 on the same HIP device, x
    without requires_grad, fp32 contiguous parameters on that device, linear3 one output wide, and the widths
    inside the shape rule of gcn_vmlp_workspace_bytes (1 <= C <= 64, 0 <= T <= 32, 1 <= H1, H2 <= 64, N >= 64)."""
    if not (isinstance(h, torch.Tensor) and isinstance(x, torch.Tensor) and h.is_cuda and x.device == h.device
            and h.dim() == 2 and x.dim() == 2 and h.dtype == torch.float32 and x.dtype == torch.float32
            and h.is_contiguous() and x.is_contiguous() and not x.requires_grad and x.shape[0] == h.shape[0]):
        return False
    l1, l2, l3 = _layers(mlp)
    for lin in (l1, l2, l3):
        for t in (lin.weight, lin.bias):
            if t is not None and not (t.device == h.device and t.dtype == torch.float32 and t.is_contiguous()):
                return False
    n, c = h.shape
    t = x.shape[1] - skip_last - d
    if l3.out_features != 1 or l1.in_features != c + t or l2.in_features != l1.out_features \
            or l3.in_features != l2.out_features:
        return False
    return _native.lib().gcn_vmlp_workspace_bytes(n, c, t, l1.out_features, l2.out_features) != 0


def _ptr(t):
    return t.data_ptr() if t is not None else None


class VertexMLPFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, x, d, tail, batch_norm, return_masks, w1, b1, w2, b2, w3, b3):
        n, c = h.shape
        h1, h2 = w1.shape[0], w2.shape[0]
        dev = h.device
        scores = torch.empty((n, 1), dtype=torch.float32, device=dev)
        stats = torch.empty(_STATS, dtype=torch.float32, device=dev) if batch_norm else None
        masks = tuple(torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2)) if return_masks else (None, None)
        params = tuple(t.detach() if t is not None else None for t in (w1, b1, w2, b2, w3, b3))
        _native.launch("gcn_vmlp_forward", dev, h.data_ptr(), x.data_ptr(), x.shape[1], d, n, c, tail,
                       _ptr(params[0]), _ptr(params[1]), h1, _ptr(params[2]), _ptr(params[3]), h2, _ptr(params[4]),
                       _ptr(params[5]), int(batch_norm), _ptr(stats), scores.data_ptr(), _ptr(masks[0]),
                       _ptr(masks[1]), workspace=_native.lib().gcn_vmlp_workspace_bytes(n, c, tail, h1, h2))
        ctx.d, ctx.tail, ctx.batch_norm = d, tail, bool(batch_norm)
        ctx.has = tuple(t is not None for t in params) + (stats is not None,)
        ctx.save_for_backward(h, x, *(t for t in params + (stats,) if t is not None))
        if return_masks:
            ctx.mark_non_differentiable(*masks)
            return scores, masks[0], masks[1]
        return scores

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        saved = list(ctx.saved_tensors)
        h, x = saved[:2]
        rest = iter(saved[2:])
        w1, b1, w2, b2, w3, b3, stats = (next(rest) if has else None for has in ctx.has)
        n, c = h.shape
        h1, h2 = w1.shape[0], w2.shape[0]
        g = g.to(torch.float32).contiguous()
        dh = torch.empty_like(h) if ctx.needs_input_grad[0] else None       # (NULL: the sweep skips it)
        grads = [torch.empty_like(t) if t is not None and need else None
                 for t, need in zip((w1, b1, w2, b2, w3, b3), ctx.needs_input_grad[6:12])]
        _native.launch("gcn_vmlp_backward", h.device, h.data_ptr(), x.data_ptr(), x.shape[1], ctx.d, n, c, ctx.tail,
                       _ptr(w1), _ptr(b1), h1, _ptr(w2), _ptr(b2), h2, _ptr(w3), _ptr(b3), int(ctx.batch_norm),
                       _ptr(stats), g.data_ptr(), _ptr(dh), *(_ptr(t) for t in grads),
                       workspace=_native.lib().gcn_vmlp_workspace_bytes(n, c, ctx.tail, h1, h2))
        return (dh, None, None, None, None, None, *grads)


def _bits(z):
    """int64 [N]: bit j set when z[:, j] > 0."""
    return ((z > 0).to(torch.int64) << torch.arange(z.shape[1], device=z.device)).sum(1)


def _composition(h, x, d, mlp, batch_norm, skip_last, return_masks):
    """What GeneratorMLPLayers / MLPLayers run on the concatenation (pygcn_amd/models.py), literally."""
    l1, l2, l3 = _layers(mlp)
    act = relu_batch_norm if batch_norm else torch.relu
    z1 = l1(torch.cat((h, x[:, d:x.shape[1] - skip_last]), dim=1))
    z2 = l2(act(z1))
    scores = l3(act(z2))
    if return_masks:
        return scores, _bits(z1.detach()), _bits(z2.detach())
    return scores


def vertex_mlp(h, x, d, mlp, batch_norm, skip_last=0, return_masks=False):
    """The score head of the fork's generators: `mlp(cat(h, x[:, d : F - skip_last]))` -> scores [N, 1], where
    `mlp` is any module with linear1..linear3 in the nn.Linear layout (a bias may be None; linear3 one output
    wide), `batch_norm=True` puts the fork's fresh BatchNorm1d after each ReLU (GeneratorMLPLayers: batch statistics
    over all N also under eval(), biased variance, eps 1e-5, gamma 1, beta 0) and `batch_norm=False` is the plain
    MLPLayers.  `skip_last=1` serves Hierarchical_Generator, whose last column of x is the group label.  h [N, C]
    receives a gradient, and so do the six parameters; x [N, F] is a constant.

    On the HIP device, inside the shape rule (`supported`), this is one autograd node over the fused sweeps of
    pygcn_amd/csrc/gcn_head.hip: the tail of x is read in place, hidden activations are recomputed, nothing of size
    [N, H] is saved, nothing synchronises with the host, and the result is bitwise reproducible.  Everything else
    — CPU tensors, other dtypes, an x that requires a gradient, N < 64, wider layers — takes the literal
    composition and gives bitwise what the module gives.

    `return_masks=True`: `(scores, mask1, mask2)`, two int64 [N] tensors with bit j set when column j of that
    hidden layer counted as > 0 — the ReLU derivative the sweeps used (written only when asked for)."""
    d, skip_last = int(d), int(skip_last)
    if h.dim() != 2 or x.dim() != 2 or x.shape[0] != h.shape[0]:
        raise RuntimeError(f"vertex_mlp: h must be [N, C] and x [N, F], got {tuple(h.shape)} and {tuple(x.shape)}")
    tail = x.shape[1] - skip_last - d
    if d < 0 or skip_last < 0 or tail < 0:
        raise RuntimeError(f"vertex_mlp: d = {d}, skip_last = {skip_last} do not go with {x.shape[1]} columns of x")
    if not supported(h, x, d, mlp, skip_last):
        return _composition(h, x, d, mlp, batch_norm, skip_last, return_masks)
    l1, l2, l3 = _layers(mlp)
    return VertexMLPFunction.apply(h, x, d, tail, bool(batch_norm), bool(return_masks), l1.weight, l1.bias,
                                   l2.weight, l2.bias, l3.weight, l3.bias)
