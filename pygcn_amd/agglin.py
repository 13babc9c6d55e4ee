"""An AGGREGATE-FIRST input layer, (Â·X)·W + b, for the narrow first layers of the fork's live models: its
evaluator feeds 4, 8 or 16 columns into a 32-wide GCN (reference pygcn/gnn-over-mlp.py:221-237), its generators
16 (policy-generator.py:330-350), and in all of them layer 1's input needs no gradient.  The reference's
association Â·(X·W) + b (pygcn/layers.py:33-38) gathers k·32-float rows in the sparse product and needs a transpose
product of the same width for grad_W alone; this one gathers k·Fin floats per stored entry and has NO sparse product
in its backward pass — HIP sweeps (pygcn_amd/csrc/gcn_agglin.hip) behind ONE autograd node:

    forward    fused.input_product           z = Â·X            (spmm_csr on Fin-wide rows; the opt-in cache of Â·X)
               gcn_agg_linear_forward        reads z, writes y = act(z · W + b)
    backward   gcn_agg_linear_backward       reads g, z (y with relu)  -> grad_W, grad_b   (double, fixed order)

The node saves z and W, and y only with relu.  There is no input gradient: an input that requires one takes the
default route.  Sums are deterministic and nothing synchronises with the host.
"""
import torch

from . import _native
from .gemm import DenseMMFunction
from .graph import CSRGraph
from .spmm import SpMMFunction

WIDTH = 32        # the one output width the sweeps are built for


def _graph_of(adj):
    """The CSRGraph `adj` resolves to without a conversion that could fail, else None (dense, sharded, CPU)."""
    if isinstance(adj, CSRGraph):
        return adj
    if isinstance(adj, torch.Tensor) and adj.layout in (torch.sparse_coo, torch.sparse_csr) and adj.is_cuda:
        from .graph import as_graph
        return as_graph(adj)
    return None


def supported(x, adj, weight, bias=None, batch=1):
    """True when the HIP sweeps take the call: `adj` resolves to a CSRGraph (never sharded or dense); x
    [n, batch·Fin], weight [Fin, 32] and bias [32] (or None) are contiguous fp32 on the graph's HIP device, 16-byte
    aligned; x does NOT require grad; and gcn_agg_linear_partial_rows is non-zero (Fin in {4, 8, ..., 32})."""
    graph = _graph_of(adj)
    if graph is None or not (isinstance(x, torch.Tensor) and isinstance(weight, torch.Tensor)):
        return False
    tensors = [x, weight] + ([bias] if bias is not None else [])
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == graph.device and t.dtype == torch.float32
               and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in tensors):
        return False
    if x.requires_grad or x.dim() != 2 or weight.dim() != 2 or batch < 1 or x.shape[0] != graph.shape[1]:
        return False
    fin, fout = weight.shape
    if x.shape[1] != batch * fin or (bias is not None and tuple(bias.shape) != (fout,)):
        return False
    return _native.lib().gcn_agg_linear_partial_rows(graph.shape[0], fin, fout, batch) != 0


class AggregateLinearFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, graph, batch, relu):
        from .fused import input_product
        fin, fout = weight.shape
        w = weight.detach()
        b = bias.detach() if bias is not None else None
        z = input_product(graph, x)
        n = z.shape[0]
        y = torch.empty((n, batch * fout), dtype=torch.float32, device=z.device)
        _native.launch("gcn_agg_linear_forward", z.device, z.data_ptr(), w.data_ptr(),
                       b.data_ptr() if b is not None else None, y.data_ptr(), n, fin, fout, batch, int(relu))
        ctx.batch, ctx.relu, ctx.has_bias = int(batch), bool(relu), bias is not None
        ctx.save_for_backward(z, w, *((y,) if relu else ()))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        z, w = ctx.saved_tensors[:2]
        y = ctx.saved_tensors[2] if ctx.relu else None
        n = z.shape[0]
        fin, fout = w.shape
        g = g.to(torch.float32).contiguous()
        rows = _native.lib().gcn_agg_linear_partial_rows(n, fin, fout, ctx.batch)
        partials = torch.empty((rows, fin * fout + fout), dtype=torch.float64, device=z.device)
        grad_w = torch.empty_like(w)
        grad_b = torch.empty(fout, dtype=torch.float32, device=z.device) if ctx.has_bias else None
        _native.launch("gcn_agg_linear_backward", z.device, g.data_ptr(), y.data_ptr() if y is not None else None,
                       z.data_ptr(), n, fin, fout, ctx.batch, int(ctx.relu), grad_w.data_ptr(),
                       grad_b.data_ptr() if grad_b is not None else None, partials.data_ptr(), rows)
        return (None, grad_w if ctx.needs_input_grad[1] else None,
                grad_b if ctx.has_bias and ctx.needs_input_grad[2] else None, None, None, None)


def _composition(x, adj, weight, bias, batch, relu):
    """What GraphConvolution.forward_wide runs: X·W on the free view [n·batch, Fin], then adj · support + bias."""
    from .sharded import ShardedGraph, ShardedSpMMFunction
    n = x.shape[0]
    fin, fout = weight.shape
    support = DenseMMFunction.apply(x.reshape(n * batch, fin), weight).view(n, batch * fout)
    wide_bias = bias.repeat(batch) if bias is not None else None
    if isinstance(adj, torch.Tensor) and adj.layout == torch.strided:
        out = torch.mm(adj, support)
        out = out + wide_bias if wide_bias is not None else out
        return torch.relu(out) if relu else out
    if isinstance(adj, ShardedGraph):
        return ShardedSpMMFunction.apply(adj, support.contiguous(), wide_bias, relu)
    from .graph import _require_cuda, as_graph
    _require_cuda(support, "input")
    return SpMMFunction.apply(as_graph(adj), support, wide_bias, relu)


def aggregate_linear(x, adj, weight, bias=None, batch=1, relu=False):
    """`act(adj @ (x_j @ weight) + bias)` (reference pygcn/layers.py:33-38, then F.relu with `relu=True`) for each
    of the `batch` column windows x_j = x[:, j·Fin:(j+1)·Fin] of x [n, batch·Fin] (k samples side by side), the
    results side by side as [n, batch·Fout]; weight is [Fin, Fout] and bias [Fout] (GraphConvolution's).

    Inside the rule (`supported`: a CSRGraph adjacency; contiguous, 16-byte aligned fp32 on the HIP device; Fin in
    {4, 8, ..., 32}, Fout = 32; x requires no gradient) this is one autograd node that evaluates the layer
    aggregate-first, (adj·x)·weight + bias: z = adj·x from `fused.input_product` (the existing sparse product on
    Fin-wide rows, kept across steps under `fused.set_input_product_cache(True)`), then the sweeps of
    pygcn_amd/csrc/gcn_agglin.hip.  It has gradients for weight and bias ONLY, no sparse product in its backward
    pass, bitwise reproducible sums, and a window's result is bitwise the batch = 1 call's on a contiguous copy of
    the window.  The association differs from the reference's, so results agree with it to rounding (the
    project's 1e-5 against float64), not bit for bit.

    Everything else — an x that requires grad, a dense or sharded adjacency, other widths or dtypes, the CPU — is
    the literal composition the layers run by default, `GraphConvolution.forward_wide`: X·W as one GEMM on the view
    [n·batch, Fin], then adj · support + bias (ReLU)."""
    batch = int(batch)
    if x.dim() != 2 or weight.dim() != 2 or batch < 1 or x.shape[1] != batch * weight.shape[0]:
        raise RuntimeError(f"aggregate_linear: x must be [n, batch*Fin] and weight [Fin, Fout], got "
                           f"{tuple(x.shape)} and {tuple(weight.shape)} with batch={batch}")
    if not supported(x, adj, weight, bias, batch):
        return _composition(x, adj, weight, bias, batch, relu)
    return AggregateLinearFunction.apply(x, weight, bias, _graph_of(adj), batch, bool(relu))
