"""GCN — the 2-layer model of upstream pygcn, which the reference fork keeps as comments around
its 3-layer edit (reference pygcn/models.py:23 `gc2 = GraphConvolution(nhid, nclass)`, :48
`F.relu(self.gc1(x, adj))`, :50 `F.dropout`, :68 `F.log_softmax(x, dim=1)`).

Parameter names gc1.weight/bias, gc2.weight/bias as in the reference (models.py:21-26).
"""
import os
import sys

import torch
import torch.nn as nn

if not __package__:   # flat import, the reference's convention (`from models import GCN`)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from layers import GraphConvolution
else:
    from pygcn_amd.layers import GraphConvolution
from pygcn_amd.attention import vertex_attention, vertex_mean  # noqa: E402
from pygcn_amd.evaluator import evaluator_ingest  # noqa: E402
from pygcn_amd.head import vertex_mlp  # noqa: E402
from pygcn_amd.norm import relu_batch_norm  # noqa: E402
from pygcn_amd.normlin import relu_batch_norm_linear  # noqa: E402
from pygcn_amd.pool import masked_mean_pool  # noqa: E402
from pygcn_amd.select import sample_without_replacement, selection_log_prob, topk_flag  # noqa: E402
from pygcn_amd.sharded import ShardedGraph  # noqa: E402
from pygcn_amd.tuning import ROWGRAD_MIN_ROWS  # noqa: E402


class GCN(nn.Module):
    def __init__(self, nfeat, nhid, nclass, dropout):
        super(GCN, self).__init__()
        self.gc1 = GraphConvolution(nfeat, nhid)
        self.gc2 = GraphConvolution(nhid, nclass)
        self.dropout = dropout

    def forward(self, x, adj, rows=None, keep_full=False, restrict_forward=False):
        """`model(x, adj)`: the reference call — log-probabilities of every vertex.

        `model(x, adj, rows=idx)` (extension): the same forward pass, returning `output[idx]` —
        what upstream's epoch feeds to the loss, `F.nll_loss(output[idx_train], labels[idx_train])`
        (pygcn/train.py:153).  Telling the model which rows the loss reads lets the whole backward
        pass run on the rows that can be non-zero (pygcn_amd/fused.py): same gradients, no
        [N, ·]-sized zero fills, scatters or sweeps, no host synchronisation.  With
        `keep_full=True` the result is `(output[idx], output.detach())` — the full matrix for
        validation on other rows, as upstream's --fastmode uses it.

        `model(x, adj, rows=idx, restrict_forward=True)` (opt-in): the FORWARD pass too runs on the
        receptive field of `idx` only — layer 2 on the rows idx, layer 1 on the rows those read — with
        the same result and, at the same generator state, the same dropout mask.  It needs a CSRGraph
        the one-node path covers and cannot keep the full matrix (it never exists); anything else
        raises, there is no fallback to the full pass.  Works in eval() and under no_grad (validation
        on idx_val is its own restricted pass)."""
        if restrict_forward:
            return self._forward_restricted(x, adj, rows, keep_full)
        if rows is not None:
            return self._forward_rows(x, adj, rows, keep_full)
        # (below ROWGRAD_MIN_ROWS vertices an epoch is launch-bound — Cora: ~1 ms — and the plain
        #  layer-by-layer composition issues fewer launches than the node's generic fallbacks)
        graph = self._one_node_graph(x, adj) if (x.dim() == 2 and x.shape[0] >= ROWGRAD_MIN_ROWS) else None
        if graph is not None:
            # the whole model as ONE autograd node (pygcn_amd/fused.py): its backward pass takes the
            # row-restricted route when the caller selected `output[idx_train]` (upstream's next
            # line, pygcn/train.py:153) and the full-height route for a loss over all vertices
            fused, _, _, dropout_seed_for = self._imports()
            p = self.dropout if self.training else 0.0
            out = fused.gcn2_full(x, self.gc1, self.gc2, graph, p, dropout_seed_for(x) if p > 0.0 else 0)
        else:
            # F.dropout(F.relu(gc1(x, adj)), p, training) with ReLU and dropout fused into the SpMM store
            h = self.gc1(x, adj, relu=True, dropout=self.dropout if self.training else 0.0)
            # F.log_softmax(gc2(x, adj), dim=1) — in the SpMM's store when a row fits one wavefront
            # (dim=1 for the reference's [N, C]; the last dim if batched)
            out = self.gc2(h, adj, log_softmax=True)
        if (self.training and out.requires_grad and out.dim() == 2 and out.is_cuda
                and out.shape[0] >= ROWGRAD_MIN_ROWS     # (pygcn_amd/tuning.py)
                and type(adj).__name__ != "ShardedGraph"):
            # upstream's next line is `output[idx_train]`: let that selection hand the backward pass
            # the rows instead of a dense gradient (pygcn_amd/rowgrad.py)
            from pygcn_amd.rowgrad import RowSelectable
            out = out.as_subclass(RowSelectable)
        return out

    @staticmethod
    def _imports():
        import pygcn_amd.fused as fused
        from pygcn_amd.graph import CSRGraph, as_graph
        from pygcn_amd.spmm import dropout_seed_for
        return fused, CSRGraph, as_graph, dropout_seed_for

    def _one_node_graph(self, x, adj):
        """The prepared graph handle if the one-node path covers this call, else None (sharded /
        dense adjacency, batched input, class counts the fused log_softmax does not take)."""
        import torch
        fused, CSRGraph, as_graph, _ = self._imports()
        graph = adj
        if isinstance(adj, torch.Tensor) and adj.layout in (torch.sparse_coo, torch.sparse_csr) \
                and adj.is_cuda:
            graph = as_graph(adj)
        if (isinstance(graph, CSRGraph) and isinstance(x, torch.Tensor) and x.dim() == 2
                and x.dtype == self.gc1.weight.dtype and self.gc1.weight.is_cuda
                and fused.fusable(self.gc2.weight.dtype, self.gc2.out_features, graph, x)):
            return graph
        return None

    def _forward_rows(self, x, adj, rows, keep_full):
        graph = self._one_node_graph(x, adj)
        if graph is not None:
            fused, _, _, dropout_seed_for = self._imports()
            p = self.dropout if self.training else 0.0
            seed = dropout_seed_for(x) if p > 0.0 else 0
            out, full = fused.gcn2_rows(x, self.gc1, self.gc2, graph, rows, p, seed, keep_full)
            return (out, full) if keep_full else out
        full = self.forward(x, adj)          # layer-by-layer path (sharded / dense adjacency / odd shapes)
        return (full[rows], full.detach()) if keep_full else full[rows]

    def _forward_restricted(self, x, adj, rows, keep_full):
        fused, CSRGraph, _, dropout_seed_for = self._imports()
        why = None
        if rows is None:
            why = "it needs `rows`, the rows the loss (or the validation) reads"
        elif keep_full:
            why = "keep_full=True asks for the full log-probability matrix, which a restricted pass never forms"
        elif isinstance(adj, ShardedGraph):
            why = "a ShardedGraph adjacency is not supported (the sharded path restricts its backward pass only)"
        elif not isinstance(adj, CSRGraph):
            kind = f"a {adj.layout} tensor" if isinstance(adj, torch.Tensor) else type(adj).__name__
            why = f"the adjacency must be a CSRGraph, got {kind} (dense and COO adjacencies take the full pass)"
        elif self._one_node_graph(x, adj) is None:
            why = ("the one-node path does not cover this call (fused.fusable: a square CSRGraph, a 2-D device "
                   "input of the parameters' dtype, a class count the fused log_softmax takes)")
        if why is not None:
            raise RuntimeError(f"GCN.forward(restrict_forward=True): {why}")
        p = self.dropout if self.training else 0.0
        seed = dropout_seed_for(x) if p > 0.0 else 0
        return fused.gcn2_rows_restricted(x, self.gc1, self.gc2, adj, rows, p, seed)


class GCNStack(nn.Module):
    """k x (GraphConvolution + ReLU), the shape of the fork's GeneratorGCN
    (reference pygcn/models.py:74-124: gc1..gc3, ReLU after each, no BatchNorm).

    `aggregate_first=True` (opt-in): layer 1 only runs as `GraphConvolution.forward_aggregate_first` —
    (adj·x)·W + b with the ReLU in the sweep, where `functional.aggregate_linear` takes the call, the default
    layer everywhere else.  Parameters and state_dict keys do not change."""

    def __init__(self, nfeat, nhid, nclass, dropout=0.0, nlayers=3, aggregate_first=False):
        super(GCNStack, self).__init__()
        dims = [nfeat] + [nhid] * (nlayers - 1) + [nclass]
        for i in range(nlayers):
            setattr(self, f"gc{i + 1}", GraphConvolution(dims[i], dims[i + 1]))
        self.nlayers = nlayers
        self.dropout = dropout
        self.aggregate_first = bool(aggregate_first)

    def forward(self, x, adj):
        first = 0
        if self.aggregate_first and x.dim() == 2:
            x = self.gc1.forward_aggregate_first(x, adj, relu=True)       # (ReLU inside the sweep)
            first = 1
        for i in range(first, self.nlayers):
            x = getattr(self, f"gc{i + 1}")(x, adj, relu=True)
        return x


class GCNBatchNorm(nn.Module):
    """The model the reference fork runs today (reference pygcn/models.py:17-71, its `GCN`): three
    GraphConvolutions, ReLU + BatchNorm after the first two, ReLU after the third, the result
    returned as is (:71):

        x = apply_bn(F.relu(gc1(x, adj)))      :49   apply_bn = nn.BatchNorm1d(x.size(1)).cuda()(x), :41-45
        x = apply_bn(F.relu(gc2(x, adj)))      :53
        x = F.relu(gc3(x, adj))                :56

    Parameters gc1..gc3 with weight / bias: the fork's state_dict keys, and nothing else — the fork
    builds a FRESH BatchNorm1d on every call, so the normalisation has no learned or running state
    (gamma = 1, beta = 0) and uses batch statistics under `model.eval()` too; so does this class.
    `dropout` and `NN` are stored and unused, as in the fork.  ReLU + BatchNorm run as the HIP
    sweeps of pygcn_amd/norm.py, the last ReLU in the store of gc3's sparse product.

    A 3-D input [k, N, nfeat] is k samples over the same graph (the fork's evaluator GCN_OVER_MLP
    loops over them, :343-349): the result is [k, N, nclass], each sample normalised on its own, all
    k in one pass (_forward_batched).

    `fused_norm=True` (opt-in): layers 2 and 3 take ReLU + BatchNorm and their own X·W as ONE node,
    `functional.relu_batch_norm_linear` — the normalised activation is neither written nor kept for the
    backward pass — and aggregate its result (GraphConvolution.aggregate); layer 1 is unchanged.  The HIP
    sweeps carry 32 -> 32 layers (the fork's widths); other widths run the same composition of nodes as the
    default.  Parameters and state_dict keys do not change.

    `aggregate_first=True` (opt-in): layer 1 ONLY is evaluated as (adj·x)·W + b,
    `GraphConvolution.forward_aggregate_first` — for the fork's narrow inputs (4 .. 32 columns into 32) on a
    CSRGraph with an input that needs no gradient, the sparse product gathers k·nfeat floats per entry instead of
    k·nhid and layer 1's backward pass has none; its pre-activation output feeds ReLU + BatchNorm unchanged, so the
    flag composes with `fused_norm`.  Any other call runs the default layer.  Same parameters, same state_dict."""

    def __init__(self, nfeat, nhid, nclass, dropout, NN=None, fused_norm=False, aggregate_first=False):
        super(GCNBatchNorm, self).__init__()
        self.gc1 = GraphConvolution(nfeat, nhid)
        self.gc2 = GraphConvolution(nhid, nhid)
        self.gc3 = GraphConvolution(nhid, nclass)
        self.dropout = dropout
        self.NN = NN
        self.fused_norm = bool(fused_norm)
        self.aggregate_first = bool(aggregate_first)

    def _layer1(self, x, adj, k=None):
        """gc1's pre-activation output on x [N, k·nfeat] (k None: the single sample [N, nfeat])."""
        if self.aggregate_first:
            return self.gc1.forward_aggregate_first(x, adj, k)
        return self.gc1(x, adj) if k is None else self.gc1.forward_wide(x, adj, k)

    def forward(self, x, adj):
        if isinstance(adj, ShardedGraph):
            raise RuntimeError("GCNBatchNorm: a ShardedGraph adjacency is not supported — BatchNorm's "
                               "statistics run over all vertices, and cross-rank statistics are not built")
        if x.dim() == 3:
            return self._forward_batched(x, adj)
        if self.fused_norm:
            return self._fused_tail(self._layer1(x, adj), adj, 1)
        x = relu_batch_norm(self._layer1(x, adj))
        x = relu_batch_norm(self.gc2(x, adj))
        return self.gc3(x, adj, relu=True)

    def _forward_batched(self, x, adj):
        """x [k, N, nfeat] -> [k, N, nclass], equal to `torch.stack([self(x[j], adj) for j in range(k)])`
        — the loop the fork's evaluator runs ("cannot batch yet", reference pygcn/models.py:343-349) —
        in one pass: ONE permute of the input to [N, k, nfeat], then `forward_wide`.  The result is the
        permuted view of the [N, k·nclass] storage — the layout `functional.masked_mean_pool` reads in
        place."""
        k, n, nfeat = x.shape
        out = self.forward_wide(x.permute(1, 0, 2).reshape(n, k * nfeat), adj, k)
        return out.view(n, k, self.gc3.out_features).permute(1, 0, 2)

    def forward_wide(self, wide, adj, k):
        """k samples that are ALREADY side by side: wide [N, k·nfeat] -> [N, k·nclass] storage, sample j in
        the columns [j·F, (j+1)·F) of both (what `functional.evaluator_ingest` writes and
        `functional.masked_mean_pool` reads as the view `.view(N, k, nclass).permute(1, 0, 2)`).  Every
        layer works on the k samples side by side (GraphConvolution.forward_wide), where per-sample
        BatchNorm is per-column BatchNorm (`relu_batch_norm(batch=k)`) and the next X·W a GEMM on the free
        view [N·k, F]: no transpose between the layers."""
        if isinstance(adj, ShardedGraph):
            raise RuntimeError("GCNBatchNorm: a ShardedGraph adjacency is not supported — BatchNorm's "
                               "statistics run over all vertices, and cross-rank statistics are not built")
        if self.fused_norm:
            return self._fused_tail(self._layer1(wide, adj, k), adj, k)
        h = relu_batch_norm(self._layer1(wide, adj, k), batch=k)
        h = relu_batch_norm(self.gc2.forward_wide(h, adj, k), batch=k)
        return self.gc3.forward_wide(h, adj, k, relu=True)

    def _fused_tail(self, z, adj, k):
        """Layers 2 and 3 on layer 1's output z [N, k·nhid], BatchNorm(relu(.)) · W as one node each."""
        z = self.gc2.aggregate(relu_batch_norm_linear(z, self.gc2.weight, batch=k), adj, k)
        return self.gc3.aggregate(relu_batch_norm_linear(z, self.gc3.weight, batch=k), adj, k, relu=True)


class SoftGeneratorPoolMLP(nn.Module):
    """The key MLP of the fork's SoftGenerator (reference pygcn/models.py:289-312) on the mean over the
    vertices: linear1..linear3, ReLU after the first two, the result as wide as the input."""

    def __init__(self, nin, nhid1, nhid2, bias=True):
        super(SoftGeneratorPoolMLP, self).__init__()
        self.linear1 = nn.Linear(nin, nhid1, bias=bias)
        self.linear2 = nn.Linear(nhid1, nhid2, bias=bias)
        self.linear3 = nn.Linear(nhid2, nin, bias=bias)

    def forward(self, h):
        x = vertex_mean(h)                                            # :304
        x = torch.relu(self.linear1(x))
        x = torch.relu(self.linear2(x))
        return self.linear3(x)


class SoftGenerator(nn.Module):
    """The fork's policy generator (reference pygcn/models.py:412-433, `get_model(config, 'SoftGenerator')`):
    the probability of picking each vertex,

        h    = GCN(x[:, :dim_touched], adj)        three GraphConvolutions, ReLU after each   :428, :127-177
        key  = PoolMLP(mean over vertices of h)    [1, nclass]                                :430, :303-312
        attn = softmax over vertices of (h . key)  [N]                                        :431, :324-329

    Submodule and parameter names are the fork's (GCN.gc1..gc3.{weight,bias}, PoolMLP.linear1..3.{weight,bias}),
    so its checkpoints load.  The fork hard-codes PoolMLP's input width as 32, the value of its gcn_nclass;
    here it is `nclass`.  `NN`, `dim_touched` and the plain lists `saved_log_probs` / `rewards` (the fork's
    driver appends to them) are kept as attributes; its ReplayBuffer and the driver are not part of the
    model.  The mean and the attention run as HIP sweeps (pygcn_amd/attention.py); `h` receives gradient
    from both, which autograd adds with one [N, nclass] addition.

    The policy step of the fork's driver is here as two methods over pygcn_amd/select.py: `select_action`
    (its `select_action`, reference pygcn/rl-policy-generator.py:324-370) and `log_prob` (its
    ReplayBuffer.get_log_prob, pygcn/utils.py:516-522), neither with a host synchronisation.

    `aggregate_first=True` (opt-in) is passed on to GCNStack."""

    def __init__(self, nfeat, nhid, nclass, dropout, NN, linear_nhid1, linear_nhid2, dim_touched=None,
                 linear_bias=True, aggregate_first=False):
        super(SoftGenerator, self).__init__()
        self.GCN = GCNStack(nfeat, nhid, nclass, dropout, nlayers=3, aggregate_first=aggregate_first)
        self.PoolMLP = SoftGeneratorPoolMLP(nclass, linear_nhid1, linear_nhid2, bias=linear_bias)
        self.dim_touched = dim_touched
        self.NN = NN
        self.saved_log_probs = []
        self.rewards = []

    def forward(self, x, adj):
        if isinstance(adj, ShardedGraph):
            raise RuntimeError("SoftGenerator: a ShardedGraph adjacency is not supported — the softmax and the "
                               "mean run over all vertices, and cross-rank reductions are not built")
        h = self.GCN(x[:, :self.dim_touched].contiguous(), adj)     # (a copy only if the slice drops columns)
        key = self.PoolMLP(h)
        return vertex_attention(h, key)

    def select_action(self, x, adj, seed=None):
        """The fork's `select_action` (reference pygcn/rl-policy-generator.py:324-370): attn = self(x, adj), NN
        vertices drawn without replacement with probabilities attn, the sum of their Categorical
        log-probabilities appended to `saved_log_probs`, and the result `(vac_flag, idx)` — vac_flag the
        zeros of attn's shape with ones at the picks (its reset_vac_flag), idx the int64 [NN] picks in draw
        order ON THE DEVICE, where the fork holds a Python list after `.tolist()`.  `seed` as in
        `functional.sample_without_replacement`."""
        attn = self(x, adj)
        idx = sample_without_replacement(attn, self.NN, seed=seed)
        self.saved_log_probs.append(selection_log_prob(attn, idx))
        vac_flag = torch.zeros_like(attn.detach()).scatter_(0, idx, 1.0)
        return vac_flag, idx

    def log_prob(self, x, adj, idx):
        """The fork's ReplayBuffer.get_log_prob (reference pygcn/utils.py:516-522): the summed Categorical
        log-probability of the picks `idx` (int64 tensor or list) under the CURRENT parameters."""
        attn = self(x, adj)
        idx = torch.as_tensor(idx, dtype=torch.int64, device=attn.device)
        return selection_log_prob(attn, idx)


class MLPLayers(nn.Module):
    """The fork's MLPLayers (reference pygcn/models.py:195-217): linear1..linear3, ReLU after the first two."""

    def __init__(self, nin, nhid1, nhid2, nout=1, bias=True):
        super(MLPLayers, self).__init__()
        self.linear1 = nn.Linear(nin, nhid1, bias=bias)
        self.linear2 = nn.Linear(nhid1, nhid2, bias=bias)
        self.linear3 = nn.Linear(nhid2, nout, bias=bias)

    def forward(self, x):
        x = torch.relu(self.linear1(x))
        x = torch.relu(self.linear2(x))
        return self.linear3(x)


class GeneratorMLPLayers(nn.Module):
    """The fork's GeneratorMLPLayers (reference pygcn/models.py:220-241): linear1..linear3 with
    `apply_bn(F.relu(.))` after the first two — ReLU + BatchNorm as the HIP sweeps of pygcn_amd/norm.py
    where the width obeys their shape rule.  The fork builds a FRESH BatchNorm1d on every call (:228-232), so
    there is no learned or running state and batch statistics are used under `eval()` too, as GCNBatchNorm
    documents."""

    def __init__(self, nin, nhid1, nhid2, nout=1, bias=True):
        super(GeneratorMLPLayers, self).__init__()
        self.linear1 = nn.Linear(nin, nhid1, bias=bias)
        self.linear2 = nn.Linear(nhid1, nhid2, bias=bias)
        self.linear3 = nn.Linear(nhid2, nout, bias=bias)

    def forward(self, x):
        x = relu_batch_norm(self.linear1(x))                 # :235
        x = relu_batch_norm(self.linear2(x))                 # :236
        return self.linear3(x)


class Generator(nn.Module):
    """The fork's Generator (reference pygcn/models.py:358-379, `get_model(config, 'Generator')`): a 0/1 flag
    on the NN vertices with the largest score,

        h      = GCNLayer(x[:, :dim_touched], adj)           three GraphConvolutions, ReLU after each  :368, :74-124
        score  = MLPLayers(cat(h, x[:, dim_touched:]))       [N, 1], ReLU + BatchNorm inside           :369-370
        flag   = score * where(score > score[argsort(score)[NN]], 1 / score, 0)                       :373-377

    The last three lines are `functional.topk_flag`: a radix select instead of the sort, no host
    synchronisation.  The fork's `print` of four `.item()` values of the scores (:371) — four host
    synchronisations per call — is dropped.  Submodule and parameter names are the fork's
    (GCNLayer.gc1..gc3, MLPLayers.linear1..linear3), so its checkpoints load; `linear_nin` must be
    nclass + (columns of x past dim_touched).

    `fused_head=True` (opt-in): the MLP runs as `functional.vertex_mlp` — fused HIP sweeps that read the tail of
    x in place and recompute the hidden activations (pygcn_amd/head.py); same parameters, same state_dict.
    `aggregate_first=True` (opt-in) is passed on to GCNStack: layer 1 as (adj·x)·W + b."""

    def __init__(self, nfeat, nhid, nclass, dropout, NN, linear_nin, linear_nhid1, linear_nhid2, dim_touched=None,
                 linear_nout=1, linear_bias=True, fused_head=False, aggregate_first=False):
        super(Generator, self).__init__()
        self.GCNLayer = GCNStack(nfeat, nhid, nclass, dropout, nlayers=3, aggregate_first=aggregate_first)
        self.MLPLayers = GeneratorMLPLayers(linear_nin, linear_nhid1, linear_nhid2, linear_nout, bias=linear_bias)
        self.dim_touched = dim_touched
        self.NN = NN
        self.fused_head = bool(fused_head)

    def scores(self, x, adj):
        """The per-vertex score [N, 1] the flag is taken from (the fork's `mlp_output`)."""
        if isinstance(adj, ShardedGraph):
            raise RuntimeError("Generator: a ShardedGraph adjacency is not supported — the selection and the "
                               "BatchNorm statistics run over all vertices, and cross-rank reductions are not built")
        d = x.shape[1] if self.dim_touched is None else self.dim_touched
        h = self.GCNLayer(x[:, :d].contiguous(), adj)
        if self.fused_head:
            return vertex_mlp(h, x, d, self.MLPLayers, batch_norm=True)
        return self.MLPLayers(torch.cat((h, x[:, d:]), dim=1))

    def forward(self, x, adj):
        return topk_flag(self.scores(x, adj), self.NN)


class Hierarchical_Generator(nn.Module):
    """The fork's Hierarchical_Generator (reference pygcn/models.py:382-408): Generator over the plain
    MLPLayers, where the LAST column of x is a group label that does not enter the MLP (:392) and every
    vertex of `target_group` (0, as the fork hard-codes it, :394) gets the minimum score before the flag
    is taken (:395-397) — torch ops on [N], the minimum stays on the device.  `fused_head=True` as in Generator,
    without BatchNorm and without the label column; `aggregate_first=True` as in Generator."""

    target_group = 0

    def __init__(self, nfeat, nhid, nclass, dropout, NN, linear_nin, linear_nhid1, linear_nhid2, dim_touched=None,
                 linear_nout=1, linear_bias=True, fused_head=False, aggregate_first=False):
        super(Hierarchical_Generator, self).__init__()
        self.GCNLayer = GCNStack(nfeat, nhid, nclass, dropout, nlayers=3, aggregate_first=aggregate_first)
        self.MLPLayers = MLPLayers(linear_nin, linear_nhid1, linear_nhid2, linear_nout, bias=linear_bias)
        self.dim_touched = dim_touched
        self.NN = NN
        self.fused_head = bool(fused_head)

    def scores(self, x, adj):
        """The masked per-vertex score [N, 1] the flag is taken from."""
        if isinstance(adj, ShardedGraph):
            raise RuntimeError("Hierarchical_Generator: a ShardedGraph adjacency is not supported — the selection "
                               "runs over all vertices, and cross-rank reductions are not built")
        d = x.shape[1] - 1 if self.dim_touched is None else self.dim_touched
        h = self.GCNLayer(x[:, :d].contiguous(), adj)
        if self.fused_head:
            mlp_output = vertex_mlp(h, x, d, self.MLPLayers, batch_norm=False, skip_last=1)
        else:
            mlp_output = self.MLPLayers(torch.cat((h, x[:, d:-1]), dim=1))
        min_value = (torch.ones_like(mlp_output) * torch.min(mlp_output)).squeeze(1)
        return torch.where(x[:, -1] == self.target_group, min_value, mlp_output.squeeze(1)).unsqueeze(1)

    def forward(self, x, adj):
        return topk_flag(self.scores(x, adj), self.NN)


class PoolLayer(nn.Module):
    """The fork's PoolLayer (reference pygcn/models.py:267-286; no parameters): x [k, N, F] -> [k, F-1],

        out[j, c] = sum_n x[j, n, F-1] * x[j, n, c] / (number of non-zero x[0, :, F-1])            :272, :279

    — every sample divided by the count of sample 0, as the fork divides.  On the device this is
    `functional.evaluator_ingest(x, 0)`: one read of x, double sums in a fixed order, and the count stays on
    the device where the fork has `len(torch.nonzero(...))`, a host read."""

    def forward(self, x):
        _, _, esum, nonzero = evaluator_ingest(x, 0)
        return esum / nonzero[0]


class GCN_OVER_MLP(nn.Module):
    """The fork's evaluator (reference pygcn/models.py:333-355, `get_model(config, 'GNN_OVER_MLP')`): for k samples
    x [k, N, F] over one graph,

        h      = GCNLayer(x[j, :, :dim_touched], adj) for every sample j          :343-349, the fork's live GCN
        pooled = PoolLayer(cat(h, x[:, :, dim_touched:]))                          :351-353
        out    = MLPLayers(pooled)                                                 :354      [k, linear_nout]

    Here: `functional.evaluator_ingest` reads x once (the GCN's columns side by side, the last column as the
    pool's mask, the masked sums of the untouched columns, the flag's count), GCNLayer.forward_wide runs all k
    samples in one pass, `functional.masked_mean_pool` reads its result in place, and the two pooled parts are
    concatenated as [k, ·] — the fork's [k, N, nclass + F - dim_touched] concatenation, its masked product and
    their gradients never exist, and nothing synchronises with the host.  Submodule and parameter names are the
    fork's (GCNLayer.gc1..gc3, MLPLayers.linear1..linear3), so its checkpoints load; `linear_nin` must be
    nclass + F - 1 - dim_touched.

    `forward(x, adj, flag=None)`: with `flag` ([k, N]; for k = 1 also [N] or [N, 1], what `Generator` returns)
    the vertex flag arrives on its own instead of as the last column of x, which is then ignored — the
    device-friendly form of `cat(..., vac_flag)` in the fork's generator training (reference
    pygcn/policy-generator.py:398-420), where the flag is the only thing that receives gradient: x stays a
    constant, and layer 1 of the GCN forms no input gradient.

    `fused_norm=True` and `aggregate_first=True` (both opt-in) are passed on to GCNBatchNorm.  The latter takes
    effect when x needs no gradient — the flag inside a constant x, or the flag on its own."""

    def __init__(self, nfeat, nhid, nclass, dropout, NN, linear_nin, linear_nhid1, linear_nhid2, dim_touched=None,
                 linear_nout=1, linear_bias=True, fused_norm=False, aggregate_first=False):
        super(GCN_OVER_MLP, self).__init__()
        self.GCNLayer = GCNBatchNorm(nfeat, nhid, nclass, dropout, NN, fused_norm=fused_norm,
                                     aggregate_first=aggregate_first)
        self.PoolLayer = PoolLayer()
        self.MLPLayers = MLPLayers(linear_nin, linear_nhid1, linear_nhid2, linear_nout, bias=linear_bias)
        self.dim_touched = dim_touched

    def forward(self, x, adj, flag=None):
        if x.dim() != 3:
            raise RuntimeError(f"GCN_OVER_MLP: x must be [k, N, F] (k samples over one graph), got {tuple(x.shape)}")
        if isinstance(adj, ShardedGraph):
            raise RuntimeError("GCN_OVER_MLP: a ShardedGraph adjacency is not supported — BatchNorm's statistics "
                               "and the pool run over all vertices, and cross-rank reductions are not built")
        k, n, f = x.shape
        d = f - 1 if self.dim_touched is None else self.dim_touched
        wide, mask, esum, nonzero = evaluator_ingest(x, d, flag)
        h = self.GCNLayer.forward_wide(wide, adj, k)
        h = h.view(n, k, self.GCNLayer.gc3.out_features).permute(1, 0, 2)
        count = nonzero[0]                                             # the fork divides by sample 0's count (:279)
        pooled = masked_mean_pool(h, mask, count=count, mask_grad=mask.requires_grad)
        return self.MLPLayers(torch.cat((pooled, esum / count), dim=1))


def get_model(config, model_name='GCN'):
    """The fork's `get_model` (reference pygcn/models.py:440-460): `config` is any object with its attribute
    names — gcn_nfeat, gcn_nhid, gcn_nclass, gcn_dropout, NN, dim_touched, linear_nin, linear_nhid1,
    linear_nhid2, linear_nout, linear_bias, and optionally fused_head (the two generators' opt-in), fused_norm
    (the evaluator's) and aggregate_first (every model with a GCN).  'MLP',
    'GNN_OVER_MLP', 'Generator', 'Hierarchical_Generator' and 'SoftGenerator' give the classes of this module.
    'GCN', the default, is broken in the fork (it passes six
    arguments to a five-argument GCN, :444: a TypeError) and raises TypeError here too; the fork lets an unknown
    name fall through to an unbound local, here it is a ValueError."""
    if model_name == 'GCN':
        raise TypeError("get_model(config, 'GCN') is broken in the fork (reference pygcn/models.py:444 passes six "
                        "arguments to its five-argument GCN): build GCNBatchNorm(nfeat, nhid, nclass, dropout, NN) "
                        "directly")
    if model_name not in ('MLP', 'GNN_OVER_MLP', 'Generator', 'Hierarchical_Generator', 'SoftGenerator'):
        raise ValueError(f"get_model: unknown model name {model_name!r} (MLP, GNN_OVER_MLP, Generator, "
                         "Hierarchical_Generator, SoftGenerator)")
    c = config
    agg = getattr(c, 'aggregate_first', False)
    gcn = (c.gcn_nfeat, c.gcn_nhid, c.gcn_nclass, c.gcn_dropout, c.NN)
    if model_name == 'MLP':
        return nn.Sequential(PoolLayer(), MLPLayers(c.linear_nin, c.linear_nhid1, c.linear_nhid2, c.linear_nout,
                                                    bias=c.linear_bias))
    if model_name == 'GNN_OVER_MLP':
        return GCN_OVER_MLP(*gcn, c.linear_nin, c.linear_nhid1, c.linear_nhid2, c.dim_touched, c.linear_nout,
                            c.linear_bias, getattr(c, 'fused_norm', False), agg)
    if model_name == 'Generator':
        return Generator(*gcn, c.linear_nin, c.linear_nhid1, c.linear_nhid2, c.dim_touched, c.linear_nout,
                         c.linear_bias, getattr(c, 'fused_head', False), agg)
    if model_name == 'Hierarchical_Generator':
        return Hierarchical_Generator(*gcn, c.linear_nin, c.linear_nhid1, c.linear_nhid2, c.dim_touched,
                                      c.linear_nout, c.linear_bias, getattr(c, 'fused_head', False), agg)
    return SoftGenerator(*gcn, c.linear_nhid1, c.linear_nhid2, c.dim_touched, c.linear_bias, agg)
