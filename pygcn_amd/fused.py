"""The 2-layer GCN training step as ONE autograd node when the loss reads a known set of rows.

Upstream's epoch (reference pygcn/train.py:140-157, kept there as comments) is

    output = model(features, adj)                                   models.py:47-71 (upstream form)
    loss_train = F.nll_loss(output[idx_train], labels[idx_train])   train.py:153
    loss_train.backward()                                           train.py:157

so the gradient that enters the model is non-zero on the rows `idx_train` only — and which rows of
every later gradient CAN be non-zero follows from the graph alone:

    grad_pre2 = d loss / d (Â·h1·W2 + b2)      rows  R  = idx_train
    grad_sup2 = Âᵀ · grad_pre2                 rows  R2 = vertices that have a neighbour in R
    grad_W2   = h1ᵀ · grad_sup2,  grad_h1 = grad_sup2 · W2ᵀ,  grad_pre1 = mask(grad_h1)   rows R2
    grad_W1   = (Â·X)ᵀ · grad_pre1 = (Â·X)[R2]ᵀ · grad_pre1[R2]
                (Â·X is the first product of the forward pass itself when the layer is evaluated
                 as (Â·X)·W1 — 256 -> 256 fp32 — so layer 1 needs no sparse product in backward)

`model(features, adj, rows=idx_train)` returns `output[idx_train]` from a node that keeps all of
this inside: R2 and the block of Âᵀ with rows R2 and columns R are cut once per (graph, rows) from
the CSR structure, every intermediate gradient lives in COMPACT form ([|R|, C] and [|R2|, H]
tensors), the layer-2 transpose product is the HIP kernel on that block (layer 1 needs none, see
below; other widths use the row-restricted launch, `gcn_epilogue.c_row_select`), and nothing of
size [N, ·] is allocated, zero-filled, scattered into, or swept to find its non-zero rows.  Compared with letting the dense
`grad_output [N, C]` travel through autograd this removes per epoch at config C4: the 10 GB zero
fill of index_put's backward and its scatter, the NLL kernels over [N, C], two full-height
backward sweeps and the scatter of grad_h1 — ≈ 11 ms of an 84 ms epoch — and every host
synchronisation of the backward pass (the row sets are static, their sizes are known on the host).
Only structurally-zero rows are skipped: the result is the same sum of the same products.

The forward pass is the ordinary one (both products over all rows, fused bias / ReLU / dropout /
log_softmax epilogues): the full log-probability matrix exists and can be kept (`keep_full=True`)
for validation on other rows, as upstream's --fastmode does.  Opt-in, `restrict_forward=True`
(GCN2RestrictedFunction): the forward pass too runs on the receptive field of the loss rows — layer 2
on R, layer 1 on R2, compact activations, the dropout mask of the full pass (spmm.dropout_rows) — and
the full matrix never exists.

Each pass is written ONCE; the three autograd nodes (GCN2RowsFunction, GCN2Function,
GCN2RestrictedFunction) only name their route:

  * `_gcn2_forward(..., rs=None)`: the full pass, or with `rs` the restricted one; what the two do
    differently is listed in its docstring and nowhere else.  It leaves `ctx.fw`, ONE record of what
    the backward pass reads (scale, x_bound, z_bound, h_bound, reassoc, keep_bits, bias_dtypes).
  * `_gcn2_backward(..., rs=None, restricted=False)`: loss rows (`_loss_rows_stage`: grad_pre2,
    grad_b2) -> early return -> the layer-2 transpose product -> hidden layer (`_hidden_layer_stage`:
    grad_W2, grad_pre1, grad_b1, grad_W1 from the saved Â·X) -> layer-1 tail; the routes — rows, dense,
    restricted — differ in the operands its docstring tabulates.  `_gcn2_backward_rows` and
    `_gcn2_backward_dense` are the first two by name (GCN2Function.backward picks between them).
  * `input_product(graph, x, rs=None)`: the one cache of Â·X (and of Â[R2,:]·X).

The two stages have two more callers: the sharded pass of pygcn_amd/sharded_fused.py (the block plus a
halo of gradient rows between them; it fills the same record) and, for the first stage, the last-layer
branch of `GraphConvFunction._backward_rows` (pygcn_amd/spmm.py).
"""
import os
import weakref
from types import SimpleNamespace

import torch

from .graph import CSRGraph
from . import gemm as _gemm, spmm as _spmm
from .gemm import _dense_forward, _weight_grad, gemm_xw256
from .spmm import log_softmax_fusable, pack_row_flags, spmm_csr


def _describe_rows(rs, rows):
    """Fills what every row-set object says about the loss rows themselves (int64 `rows`, in the
    user's order): rows_user, rows_u (sorted, unique), inverse, n_u, has_duplicates, sorted_unique."""
    rs.rows_user = rows
    rs.rows_u, rs.inverse = torch.unique(rows, return_inverse=True)             # sorted
    rs.n_u = int(rs.rows_u.numel())
    rs.has_duplicates = rs.n_u != rows.numel()
    rs.sorted_unique = bool(not rs.has_duplicates and (rs.n_u == 0 or bool((rows == rs.rows_u).all())))


def _list_rows2(rs, rows2):
    """Fills the forms of R2 (sorted int64 `rows2`) the kernels read: rows2, n2, rows2_i32 (the
    mask rows of the grad_input GEMM), rows2_padded (the weight-gradient kernel's list)."""
    rs.rows2, rs.n2 = rows2, int(rows2.numel())
    rs.rows2_i32 = rows2.to(torch.int32)
    rs.rows2_padded = _gemm.padded_row_list(rows2)


class RowSets:
    """What the backward pass needs to know about the loss rows R, computed ONCE per
    (graph, rows tensor): R sorted and unique, R2 = the columns that occur in rows R of Â (= the
    rows of Âᵀ·grad_pre2 that can be non-zero) with its bitmap / count, and `at_block` = the
    [|R2|, |R|] block of Âᵀ the layer-2 backward product runs on.  The block's values, and the blocks of
    restricted(), follow in-place edits of graph.val (row_sets() -> follow_values)."""

    def __init__(self, graph, rows):
        dev, n = graph.device, graph.shape[0]
        rows = rows.to(device=dev, dtype=torch.int64)
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
            raise RuntimeError("rows: index out of range")
        _describe_rows(self, rows)
        rp = graph.rowptr.to(torch.int64)
        starts, lens = rp[self.rows_u], rp[self.rows_u + 1] - rp[self.rows_u]
        total = int(lens.sum())
        idx = torch.repeat_interleave(starts - torch.cumsum(lens, 0) + lens, lens) + \
            torch.arange(total, device=dev)
        cols = graph.col[idx].to(torch.int64)
        _list_rows2(self, torch.unique(cols))                                     # sorted
        # The block of Âᵀ the backward product needs — rows R2, columns R — as its own small CSR
        # (compact row / column numbering): entry (r, c) of Â with r in R becomes entry
        # (pos of c in R2, pos of r in R) of the block.  Sorted by (row, source row): within a row
        # the entries come in the order of the full CSR(Âᵀ).  Built once per (graph, rows).
        src = torch.repeat_interleave(torch.arange(self.n_u, device=dev, dtype=torch.int64), lens)
        dst = torch.searchsorted(self.rows2, cols)
        order = torch.argsort(dst * max(self.n_u, 1) + src)
        rp = torch.zeros(self.n2 + 1, dtype=torch.int64, device=dev)
        if total:
            torch.cumsum(torch.bincount(dst, minlength=self.n2), 0, out=rp[1:])
        # The block's VALUES follow graph.val (follow_values); rows2, hint2 and every schedule hang on the
        # pattern alone.
        self._val_from = idx[order]                # position in graph.val of every entry of the block
        self._val_version = graph.val._version
        self.at_block = CSRGraph(rp.to(torch.int32 if total < 2 ** 31 - 1 else torch.int64),
                                 src[order].to(torch.int32), graph.val.detach().index_select(0, self._val_from),
                                 (self.n2, self.n_u))
        mask2 = torch.zeros(graph.shape[1], dtype=torch.bool, device=dev)
        mask2[self.rows2] = True
        self.hint2 = pack_row_flags(mask2)

    _restricted = None       # (graph.val version, a_rows2, a_block), built by restricted()
    _input_product = None    # (weakref of X, its version, graph.val version, a_rows2·X): input_product(.., rs)

    def follow_values(self, graph):
        """at_block's values again from graph.val when that was edited in place since they were gathered: one
        index_select into the block's own array (same address: its schedules stay), no host read.  An unedited
        graph costs the comparison of two host integers."""
        if self._val_version != graph.val._version:
            torch.index_select(graph.val.detach(), 0, self._val_from, out=self.at_block.val)
            self._val_version = graph.val._version

    def restricted(self, graph):
        """The two row blocks of Â the RESTRICTED forward pass multiplies with (GCN2RestrictedFunction),
        cut on the device by CSRGraph.take_rows on first use and again when graph.val was edited in
        place — the routes that do not restrict the forward pass never pay for them:
            a_rows2 = Â[R2, :]     [n2, N], global columns: layer 1 on the rows layer 2 reads
            a_block = Â[R, R2]     [n_u, n2], columns numbered by position in R2: layer 2 on the loss rows
        (every column of a row of R lies in R2 — that is R2's definition — so no entry is unmapped)."""
        hit = self._restricted
        if hit is None or hit[0] != graph.val._version:
            a_rows2 = graph.take_rows(self.rows2)
            pos = torch.full((graph.shape[1],), -1, dtype=torch.int32, device=graph.device)
            pos[self.rows2] = torch.arange(self.n2, dtype=torch.int32, device=graph.device)
            a_block = graph.take_rows(self.rows_u, col_map=pos, n_cols=self.n2)
            if a_block.n_unmapped:
                raise RuntimeError(f"row sets: {a_block.n_unmapped} entries of the loss rows fall outside R2 "
                                   "(the graph's structure changed since the row sets were built)")
            hit = self._restricted = (graph.val._version, a_rows2, a_block)
        return hit[1], hit[2]


_ROWSETS = weakref.WeakKeyDictionary()    # graph -> {index-tensor identity: (RowSets, rows)}


def rows_key(rows):
    """Identity of an index tensor for the row-set caches: everything that determines WHICH
    elements it reads (two strided views of one storage share pointer, length and version counter
    — idx[:100] vs idx[0:200:2] — so stride and storage offset are part of it), plus the version
    counter for in-place edits."""
    return (rows.data_ptr(), rows.numel(), rows._version, rows.dtype, tuple(rows.stride()),
            rows.storage_offset(), str(rows.device))


def row_sets(graph, rows):
    per_graph = _ROWSETS.setdefault(graph, {})
    key = rows_key(rows)
    rs = per_graph.get(key)
    if rs is None:
        if len(per_graph) >= 4:
            per_graph.clear()
        rs = per_graph[key] = (RowSets(graph, rows), rows)     # (keeps `rows` alive: ptr stays unique)
    rs[0].follow_values(graph)
    return rs[0]


def fusable(model_dtype, nclass, graph, x):
    """Shapes / layouts the one-node path covers; anything else takes the layer-by-layer path."""
    return (isinstance(graph, CSRGraph) and x.dim() == 2 and x.is_cuda and graph.shape[0] == graph.shape[1]
            and log_softmax_fusable(nclass, model_dtype))


def _operand_buffer(n, width, dtype, device, rows, values, count):
    """[n, width] tensor holding `values` at `rows`; the other rows are left UNWRITTEN when the
    product that reads it is certain to honour the row hint (it then never touches them), and are
    zero otherwise."""
    honoured = _spmm._hint_will_be_used(n, width, torch.finfo(dtype).bits // 8, True, count)   # (fresh: aligned)
    buf = _spmm._maybe_poisoned((n, width), dtype, device) if honoured \
        else torch.zeros((n, width), dtype=dtype, device=device)
    if rows is not None:           # (None: the caller writes the rows itself)
        buf.index_copy_(0, rows, values)
    return buf


_CACHE_INPUT_PRODUCT = False


def set_input_product_cache(enabled):
    """OPT-IN (default off).  With layer 1 evaluated as (Â·X)·W1, its sparse product z = Â·X is a
    product of two CONSTANTS of a training run (the adjacency and the feature matrix): switched on,
    z is computed once per (graph, feature tensor, their version counters) and reused by every later
    step — an epoch then contains ONE forward sparse product instead of two (−16 ms of 50 at C4).
    The result is bitwise the same.  Off by default because the benchmark's epoch is defined with
    both forward products inside it; bench.py reports the cached figure beside it."""
    global _CACHE_INPUT_PRODUCT
    _CACHE_INPUT_PRODUCT = bool(enabled)


def input_product(graph, x, rs=None):
    """z = Â·X for the layer-1 input, from the per-graph cache when set_input_product_cache(True), X
    needs no gradient, and neither the graph's values nor X changed since it was computed.  With `rs`:
    z_c = Â[R2, :]·X, the compact input of the restricted pass, under the same rule; that product
    hangs on the row sets (`rs._input_product`) where the full one hangs on the graph.  While the stream
    is being captured into a hipGraph the cache is neither consulted nor filled: the product is recorded
    in the graph, so a replay follows in-place refills of X."""
    a, holder = (graph, graph) if rs is None else (rs.restricted(graph)[0], rs)
    if not _CACHE_INPUT_PRODUCT or x.requires_grad or torch.cuda.is_current_stream_capturing():
        return spmm_csr(a, x)
    hit = getattr(holder, "_input_product", None)
    if (hit is not None and hit[0]() is x and hit[1] == x._version and hit[2] == graph.val._version):
        return hit[3]
    z = spmm_csr(a, x)
    holder._input_product = (weakref.ref(x), x._version, graph.val._version, z)
    return z


# ON by default (22.2 -> 21.0 ms of kernels, 51.7 -> 49.9 ms per epoch at C4).  PYGCN_PACKED_HIDDEN=0 in
# the environment starts with the dense route: an A/B switch for bench.py, which has no flag for it.
_PACKED_HIDDEN = os.environ.get("PYGCN_PACKED_HIDDEN", "1") != "0"


def set_packed_hidden(enabled):
    """Layer 2 of the training-mode forward pass as (Â·h1)·W2 over PACKED hidden rows:

        P    = rows_pack384(h1)                     384-byte slots: masks + the non-zero values (>= 75 % of h1 is 0)
        z2   = Â·P                                  the wide SpMM gathering 3/8 of the bytes per stored entry
        logp = log_softmax(z2·W2 + b2)              the contiguous-row GEMM with the log_softmax epilogue

    instead of log_softmax(Â·(h1·W2) + b2).  Taken where packed_hidden_applies(); every other call, eval mode
    and dropout 0 keep the dense route.  The backward pass is the same for both (h1 itself is still written)."""
    global _PACKED_HIDDEN
    _PACKED_HIDDEN = bool(enabled)


def packed_hidden():
    """Is the packed route switched on (set_packed_hidden)?"""
    return _PACKED_HIDDEN


def packed_hidden_applies(h1, w2, b2, dropout_p):
    """fp32, hidden width 256, 256 classes, dropout > 0 (a training-mode pass: h1 is mostly zeros) and the
    hand-written three-part GEMMs."""
    return (_PACKED_HIDDEN and dropout_p > 0.0 and h1.dtype == torch.float32 and _gemm.gemm_scheme() == "bf16x3"
            and tuple(w2.shape) == (256, 256) and w2.dtype == torch.float32 and w2.stride(1) == 1
            and _spmm.rows_pack512_usable(h1) and h1.stride(0) < (1 << 21)
            and (b2 is None or (b2.dtype == torch.float32 and b2.is_contiguous() and b2.data_ptr() % 16 == 0)))


def _layer2_packed(graph, h1, w2, b2):
    """logp by the packed route, or None where the log_softmax GEMM declines the operands."""
    z2 = spmm_csr(graph, packed=_spmm.rows_pack384(h1))
    return _gemm.gemm_xw256_log_softmax(z2, w2, b2)


def _forward_record(dropout_p, b1, b2):
    """`ctx.fw`: everything a one-node forward pass leaves for its backward pass besides the saved
    tensors (the sharded pass of pygcn_amd/sharded_fused.py fills the same record):
        scale                      1 / (1 - p) of the dropout
        x_bound, z_bound, h_bound  bounds of max|X|, max|Â·X|, max|h1| for the scaled GEMMs ("h2"), else None
        reassoc                    layer 1 ran as (Â·X)·W1: the tensor saved in place of X is z = Â·X
        keep_bits                  `h1 > 0` as one bit per element where the layer GEMM wrote it, else None
        bias_dtypes                (b1's, b2's) dtype, None for a layer without bias"""
    return SimpleNamespace(scale=_spmm.dropout_scale(dropout_p), x_bound=None, z_bound=None, h_bound=None,
                           reassoc=False, keep_bits=None,
                           bias_dtypes=(b1.dtype if b1 is not None else None, b2.dtype if b2 is not None else None))


def _gcn2_forward(ctx, x, w1, b1, w2, b2, graph, dropout_p, seed, rs=None):
    """Forward pass of every one-node function: (tensor saved in place of x, h1, logp).  Leaves ctx.graph
    and the record ctx.fw (_forward_record).

    With `rs` (the row sets of the loss rows: GCN2RestrictedFunction) the pass is RESTRICTED to their
    receptive field — layer 2 on the rows R reads h1 on R2, layer 1 on R2 reads X everywhere; h1 is
    compact [n2, H], logp is [n_u, C] in the order of rs.rows_u — the same sums for the rows it keeps:

        reassociated layer 1     z_c = Â[R2,:]·X      h1_c = relu(z_c·W1 + b1)        GEMM on n2 rows
        other widths             sup1 = X·W1 [N, H]   h1_c = relu(Â[R2,:]·sup1 + b1)
        dropout_rows(h1_c, R2)   the keep bits of the full pass at rows R2 (in place)
        sup2_c = h1_c·W2         logp_u = log_softmax(Â[R,R2]·sup2_c + b2)

    The two passes differ in this and nothing else (some of it decides result bits under "h2"):

                                   full pass                               restricted pass
        layer-1 matrix `a1`, and   graph                                   Â[R2,:] = rs.restricted(graph)[0]
        its inf_norm() in z_bound
        / h_bound
        the cached Â·X hangs on    graph._input_product                    rs._input_product
        dropout                    in the store of the layer_gemm / SpMM   not in the launch: dropout_rows(h1,
                                   launch (`in_launch`)                    rs.rows2, p, seed) after it
        h_bound, reassociated      the maximum the GEMM reports, as it is  that maximum x 1.0001·scale (dropout
        path                                                               follows the launch)
        keep bits                  where gemm_keep_bits_usable and a       never (the mask is h1_c > 0)
                                   gradient is needed
        layer 2, matrix `a2`       the packed route where                  spmm_csr(Â[R,R2], h1·W2, log_softmax)
                                   packed_hidden_applies, else
                                   spmm_csr(graph, h1·W2, log_softmax)"""
    restricted = rs is not None
    a1, a2 = rs.restricted(graph) if restricted else (graph, graph)
    in_launch = {} if restricted else {"dropout_p": dropout_p, "seed": seed}
    _spmm.keep_graph(ctx, graph)
    fw = ctx.fw = _forward_record(dropout_p, b1, b2)
    # bounds of max|operand| for the scaled fp16 GEMMs (set_gemm_scheme("h2") only; the default
    # three-part bf16 GEMMs need none), without a pass over the data:
    # X is constant (cached), and |Â·B| <= ‖Â‖∞·max|B|
    bounded = x.dtype == torch.float32 and _gemm.gemm_needs_bounds()
    fw.x_bound = _gemm.absmax_cached(x) if bounded else None
    # Layer 1 REASSOCIATED when a GEMM kernel can carry the layer's epilogue (256 -> 256 fp32;
    # bf16 128 -> 128 / 256):
    #     h1 = dropout(relu((Â·X)·W1 + b1))        instead of   dropout(relu(Â·(X·W1) + b1))
    # — the same two kernels and the same bytes in the forward pass (an SpMM at the input's
    # width, a GEMM), but the product z = Â·X of THIS forward pass is then all the backward
    # pass needs for grad_W1 = zᵀ·grad_pre1: no second sparse product for layer 1 (12.7 ms at
    # C4, 35.5 ms at C5).
    fw.reassoc = bool(_gemm.layer_gemm_reassociable(x, w1, b1))
    h1 = h_bound = z = None
    if fw.reassoc:
        z = input_product(graph, x, rs)
        if bounded:
            fw.z_bound = a1.inf_norm() * fw.x_bound * 1.0001
            h_bound = torch.zeros(1, dtype=torch.float32, device=x.device)   # max|h1| of the launch, exact
        # `h1 > 0` — all the backward of ReLU / dropout asks of h1 — as one bit per element, written by the
        # same launch where it can: the masked grad_input GEMM then reads 32 bytes per row instead of 1 KiB
        if not restricted and _gemm.gemm_keep_bits_usable(z, None, dropout_p) and any(ctx.needs_input_grad):
            fw.keep_bits = torch.empty((z.shape[0], 8), dtype=torch.int32, device=z.device)
        h1 = _gemm.layer_gemm(z, w1, fw.z_bound, h_bound, bias=b1, relu=True, keep_bits_out=fw.keep_bits, **in_launch)
        if h1 is None:                     # (alignment the kernel cannot take)
            fw.reassoc, z, h_bound, fw.keep_bits = False, None, None, None
        elif bounded and restricted:
            h_bound = h_bound * (1.0001 * fw.scale)
    if h1 is None:
        s_max = torch.zeros(1, dtype=torch.float32, device=x.device) if bounded else None
        sup1 = _dense_forward(x, w1, fw.x_bound, s_max)
        h1 = spmm_csr(a1, sup1, bias=b1, relu=True, **in_launch)
        del sup1
        if bounded:   # |relu/dropout(Â·S + b)| <= (‖Â‖∞·max|S| + max|b|) / (1 - p)
            h_bound = a1.inf_norm() * s_max
            if b1 is not None:
                h_bound = h_bound + b1.detach().abs().max().float()
            h_bound = h_bound * (1.0001 * fw.scale)
    if restricted and dropout_p > 0.0:
        _spmm.dropout_rows(h1, rs.rows2, dropout_p, seed)
    fw.h_bound = h_bound
    logp = _layer2_packed(graph, h1, w2, b2) if (not restricted and packed_hidden_applies(h1, w2, b2, dropout_p)) \
        else None
    if logp is None:
        logp = spmm_csr(a2, _dense_forward(h1, w2, h_bound), bias=b2, log_softmax=True)
    return (z if fw.reassoc else x), h1, logp


def _loss_rows_stage(grad, logp, want_colsum, rs=None, round_first=False):
    """LOSS ROWS, the first stage of every one-node backward pass: log_softmax backward plus the
    last layer's bias sums.  `grad` — a dense [m, C] tensor or an NLLGrad — is the gradient that
    arrives for the log-probabilities `logp` [m, C]; `rs` (None at full height) says through
    has_duplicates / sorted_unique / inverse / n_u whether those m rows repeat or are out of order.
    One HIP pass where the shape allows (gcn_nll_log_softmax_backward_colsum for an NLLGrad,
    gcn_log_softmax_backward_colsum else: grad_pre and the column sums together), torch ops
    otherwise — class counts the kernels do not take, rows listed twice.
    Returns (grad_pre2 in logp's dtype, rows sorted and unique; column sums of grad_pre2 for the
    bias gradient — fp32, or already rounded to logp's dtype by the HIP pass — or None when not
    wanted).  `round_first`: the torch form sums the ROUNDED grad_pre2 (the one-node-per-layer
    route's order for bf16; the model-level routes sum before rounding)."""
    from .functional import NLLGrad
    dt = logp.dtype
    one_pass = None
    if isinstance(grad, NLLGrad):
        one_pass = _spmm.nll_log_softmax_backward(logp, grad.target, grad.coef)
        if one_pass is None:
            grad = grad.dense()
    if one_pass is None and rs is None:
        grad = grad.to(dt)          # (full height: another dtype is cast; with rows it takes the torch form)
    if one_pass is None and grad.dtype == dt and not (rs is not None and rs.has_duplicates):
        one_pass = _spmm.backward_with_colsum(grad.contiguous(), logp, log_softmax=True)
    if one_pass is not None:
        gp, colsum = one_pass[0], (one_pass[1] if want_colsum else None)
    else:
        g = grad.float()
        gp = g - logp.float().exp() * g.sum(1, keepdim=True)
        if round_first:
            gp = gp.to(dt)
        colsum = gp.float().sum(0) if want_colsum else None
    gp = gp.to(dt)
    if rs is not None and rs.has_duplicates:           # the same vertex listed twice: add up
        gp = torch.zeros((rs.n_u, gp.shape[1]), dtype=dt, device=gp.device).index_add_(0, rs.inverse, gp)
    elif rs is not None and not rs.sorted_unique:      # rows of R in sorted order (the block's columns)
        gp = torch.empty_like(gp).index_copy_(0, rs.inverse, gp)
    return gp, colsum


def _hidden_layer_stage(fw, h1, w2, grad_sup2, gs_bound, z, needs, rows=None, l1_follows_l2=False):
    """HIDDEN LAYER, the stage after the route's own layer-2 sparse product: from the forward pass's
    record `fw` (_gcn2_forward), grad_sup2 (and `gs_bound`, its bound for the scaled GEMMs, or None)

        grad_W2   = h1ᵀ · grad_sup2         gather-fused MFMA kernel (weight_grad_rows)
        grad_pre1 = mask(grad_sup2 · W2ᵀ)   MFMA GEMM with the ReLU / dropout mask (h1 > 0, or its
                                            one-bit form `keep_bits`) in its store
        grad_b1, grad_W1 = zᵀ · grad_pre1   ONE pass over grad_pre1 where that kernel exists, else a
                                            column-sum sweep and a second weight-gradient launch

    `rows` names the rows of h1 / z that grad_sup2's rows stand for: an object with rows2 (int64),
    rows2_i32, rows2_padded and n2 (RowSets, ShardedRowSets) — everything is then compact,
    [n2, ·], and h1 / z are read in place through the lists — or None = all rows, in order (the
    convention of weight_grad_rows' `rows_a` and gemm_xw256's `mask_rows`, which receive it as it
    is).  `z` = Â·X saved by a reassociated first layer, or None: grad_W1 is then the caller's.
    `needs` = (need_w1, need_b1, need_w2); grad_b1 comes in the bias's dtype, fw.bias_dtypes[0].
    Shapes a kernel declines fall through to the next form (each returns None before it allocates
    or launches).
    `l1_follows_l2`: the full-height and the sharded pass reach for layer 1's gather-fused fp32
    kernels only where layer 2's GEMMs were on theirs (256 classes too); the single-GPU row pass
    asks the kernels alone.  The routes differ there (256 -> 256 -> C < 256), and each keeps its
    launches.
    Returns (grad_pre1, its bound or None, grad_W2, grad_b1, grad_W1)."""
    dev, dt = h1.device, h1.dtype
    f32 = dt == torch.float32
    need_w1, need_b1, need_w2 = needs
    b1_dtype = fw.bias_dtypes[0] if need_b1 else None
    scale, h_bound, z_bound, keep_bits = fw.scale, fw.h_bound, fw.z_bound, fw.keep_bits
    rows2, rows2_i32, rows2_padded, n2 = (rows.rows2, rows.rows2_i32, rows.rows2_padded, rows.n2) \
        if rows is not None else (None,) * 4
    if n2 == 0:          # an empty list (a rank without labelled neighbourhood): every sum is empty
        def zeros(*shape, dtype=dt):
            return torch.zeros(shape, dtype=dtype, device=dev)
        return (zeros(0, h1.shape[1]), zeros(1, dtype=torch.float32) if f32 else None,
                zeros(h1.shape[1], grad_sup2.shape[1]) if need_w2 else None,
                zeros(h1.shape[1], dtype=b1_dtype) if b1_dtype is not None else None,
                zeros(z.shape[1], h1.shape[1]) if (z is not None and need_w1) else None)
    l2_fast = f32 and _gemm.gemm_handwritten() and grad_sup2.shape[1] == 256 and h1.shape[1] == 256
    l1_kernels = l2_fast or not f32 or not l1_follows_l2
    grad_w2 = grad_b1 = grad_w1 = h1c = None
    if need_w2:
        # (fp32 256 x 256, or bf16 128 x 128: rows of h1 read in place through the list)
        grad_w2 = _gemm.weight_grad_rows(h1, grad_sup2, rows2_padded, None, h_bound, gs_bound, n_list=n2)
        if grad_w2 is None:
            h1c = h1 if rows2 is None else h1.index_select(0, rows2)
            grad_w2 = _weight_grad(h1c, grad_sup2)
    gh_max = torch.zeros(1, dtype=torch.float32, device=dev) if f32 else None
    w2t = w2.t().contiguous()
    gpre1 = gemm_xw256(grad_sup2, w2t, gs_bound, gh_max, mask_src=h1, mask_rows=rows2_i32,
                       mask_bits=keep_bits, mask_scale=scale)
    if gpre1 is None:                                  # (C5: the bf16 GEMM carries the mask in its store too)
        gpre1 = _gemm.gemm_bf16(grad_sup2, w2t, mask_src=h1, mask_rows=rows2_i32, mask_scale=scale)
    if gpre1 is None:
        gh1 = _dense_forward(grad_sup2, w2t, gs_bound, gh_max)
        if rows2 is None:
            gpre1 = _spmm.relu_dropout_backward(gh1.contiguous(), h1, scale)
        else:
            h1c = h1.index_select(0, rows2) if h1c is None else h1c
            gpre1 = torch.where(h1c > 0, gh1 * scale if scale != 1.0 else gh1,
                                torch.zeros((), dtype=dt, device=dev))
        if gh_max is not None:
            gh_max = gh_max * scale
        del gh1
    del h1c
    if b1_dtype is not None and z is not None and need_w1 and l1_kernels:
        # grad_W1 and grad_b1 from ONE pass over grad_pre1: the weight-gradient kernel sums the rows it loads
        both = _gemm.weight_grad_rows(z, gpre1, rows2_padded, None, z_bound, gh_max, n_list=n2, colsum_g=True)
        if both is not None:
            grad_w1, grad_b1 = both[0], both[1].to(b1_dtype)
    if b1_dtype is not None and grad_b1 is None:
        sums = _spmm.backward_with_colsum(gpre1) if gpre1.is_contiguous() else None   # (one HIP pass)
        grad_b1 = (sums[1] if sums is not None else gpre1.float().sum(0)).to(b1_dtype)
    if z is not None and need_w1 and grad_w1 is None:
        if l1_kernels:
            grad_w1 = _gemm.weight_grad_rows(z, gpre1, rows2_padded, None, z_bound, gh_max, n_list=n2)
        if grad_w1 is None:
            grad_w1 = _weight_grad(z if rows2 is None else z.index_select(0, rows2), gpre1)
    return gpre1, gh_max, grad_w2, grad_b1, grad_w1


def _gcn2_backward(ctx, x, w1, w2, h1, logp, grad, needs, rs=None, restricted=False):
    """The backward pass of every single-GPU one-node function, in five steps: loss rows, early return,
    the layer-2 transpose product, hidden layer, layer-1 tail.  `grad` is the gradient that arrives for
    `logp` (for the routes with row sets `rs`: [|rows|, C] in the user's row order, `logp` = the
    log-probabilities at those rows); `x` is the z = Â·X the forward pass saved when ctx.fw.reassoc.
    Returns (grad_x, grad_w1, grad_b1, grad_w2, grad_b2).  The routes differ in this and nothing else:

                                   rows (rs)                 dense (no rs)            restricted (rs, restricted)
        h1 / z / x saved by        full height, read in      full height              COMPACT [n2, ·]: "all rows, in
        the forward pass           place through rs's lists                           order" of their own height
        loss stage                 rs                        no row sets              rs
        layer-2 operand            rs.at_block               CSR(Âᵀ)                  rs.at_block
        hidden stage `rows=`       rs                        None                     None (rs when R2 is empty:
                                                                                      the stage returns the zeros)
        `l1_follows_l2`            no                        yes                      no
        layer-1 matrix             CSR(Âᵀ)                   CSR(Âᵀ)                  Â[R2,:]ᵀ
        its operand                compact -> [N, ·] by      as it is                 as it is
                                   _operand_buffer, b_hint
        grad_W1 from a forward     yes (c_select; no grad_x  no                       no
        product on rows R2         and Fin <= 2·H)
        empty R2                   the hidden stage's zeros  —                        zero grad_x / grad_W1 here

    Nothing of size [N, ·] exists on the rows route before the layer-1 operand; the dense route is the
    minimum number of full-height sweeps, each stage handing the next what it needs; none synchronises
    with the host."""
    _spmm.graph_unedited(ctx)
    fw, graph = ctx.fw, ctx.graph
    need_x, need_w1, need_b1, need_w2, need_b2 = needs
    dev, dt = h1.device, h1.dtype
    f32 = dt == torch.float32
    listed = rs is not None and not restricted           # the rows route
    a1_t = None if restricted else graph.t()             # (restricted: Â[R2,:]ᵀ, built where the tail needs it)
    # ---- loss rows ([|R|, C] with row sets); for the mean-NLL gradient over all rows (NLLGrad,
    # pygcn_amd/functional.py) the loss gradient is never materialised
    gp, colsum = _loss_rows_stage(grad, logp, fw.bias_dtypes[1] is not None and need_b2, rs)
    grad_b2 = colsum.to(fw.bias_dtypes[1]) if colsum is not None else None
    grad_w1 = grad_w2 = grad_b1 = grad_x = None
    if not (need_x or need_w1 or need_b1 or need_w2):
        return grad_x, grad_w1, grad_b1, grad_w2, grad_b2
    # ---- layer 2: Âᵀ · grad_pre2.  With row sets only rows R of grad_pre2 are non-zero and only rows
    # R2 of the result can be: the product runs on that block of Âᵀ (RowSets.at_block), compact operand
    # [|R|, C] in, compact result [|R2|, C] out.
    # Bound of max|grad_sup2| for the scaled GEMMs: its EXACT maximum, reported by the product itself
    # (gcn_epilogue.c_absmax: one conditional atomic per wave) — ‖Âᵀ‖∞·max|grad_pre2| would overshoot
    # by the hub column sums, a separate reduction pass costs 0.5 ms at C4 (2 ms at full height)
    gs_max = torch.zeros(1, dtype=torch.float32, device=dev) if f32 else None
    grad_sup2 = spmm_csr(rs.at_block if rs is not None else a1_t, gp.contiguous(), tag="bwd_l2", c_absmax=gs_max)
    del gp
    gs_bound = gs_max * 1.0001 if f32 else None
    # ---- hidden layer
    gpre1, gpre_bound, grad_w2, grad_b1, grad_w1 = _hidden_layer_stage(
        fw, h1, w2, grad_sup2, gs_bound, x if fw.reassoc else None, (need_w1, need_b1, need_w2),
        rows=rs if (listed or (restricted and rs.n2 == 0)) else None, l1_follows_l2=rs is None)
    del grad_sup2
    # ---- layer 1 (reassociated: grad_W1 is done, and x is this step's Â·X)
    if restricted and rs.n2 == 0:                        # (no vertex feeds the loss rows: every sum is empty)
        if need_x:
            grad_x = torch.zeros((graph.shape[1], w1.shape[0]), dtype=dt, device=dev)
        if need_w1 and grad_w1 is None:
            grad_w1 = torch.zeros_like(w1)
    elif listed and not fw.reassoc and not need_x and x.shape[1] <= _spmm.REASSOC_MAX_WIDTH_RATIO * gpre1.shape[1]:
        if need_w1:
            # grad_W1 = (Â·X)[R2]ᵀ · grad_pre1[R2]: a forward product restricted to rows R2
            n = graph.shape[0]
            z = spmm_csr(graph, x, tag="bwd_l1", c_select=rs.hint2[0],
                         out=_spmm._maybe_poisoned((n, x.shape[1]), x.dtype, dev))
            if f32 and _gemm.gemm_handwritten() and x.shape[1] == 256 and gpre1.shape[1] == 256:
                z_bound = graph.inf_norm() * fw.x_bound * 1.0001 if fw.x_bound is not None else None
                grad_w1 = _gemm.weight_grad_rows(z, gpre1, rs.rows2_padded, None, z_bound,
                                                 gpre_bound, n_list=rs.n2)
            if grad_w1 is None:
                grad_w1 = _weight_grad(z.index_select(0, rs.rows2), gpre1)
    elif need_x or (need_w1 and not fw.reassoc):
        # ONE transpose product: of grad_pre1·W1ᵀ when layer 1 was reassociated (its result is grad_X),
        # else of grad_pre1 (grad_sup1, which grad_W1 = Xᵀ·grad_sup1 and grad_X = grad_sup1·W1ᵀ share)
        if restricted:
            a1_t = rs.restricted(graph)[0].t()
        g1 = _dense_forward(gpre1, w1.t().contiguous(), gpre_bound) if fw.reassoc else gpre1
        if listed:
            g1 = _operand_buffer(graph.shape[0], g1.shape[1], dt, dev, rs.rows2, g1, rs.n2)
        elif not fw.reassoc:
            g1 = g1.contiguous()
        g1 = spmm_csr(a1_t, g1, tag="bwd_l1", b_hint=rs.hint2 if listed else None)
        if fw.reassoc:
            grad_x = g1
        else:
            if need_w1:
                grad_w1 = _weight_grad(x, g1)
            if need_x:
                grad_x = _dense_forward(g1, w1.t().contiguous())
    return grad_x, grad_w1, grad_b1, grad_w2, grad_b2


def _gcn2_backward_rows(ctx, x, w1, w2, h1, out_rows, rs, grad_rows, needs):
    """The rows route of _gcn2_backward: a gradient that is non-zero on the loss rows only (module
    docstring), after a full-height forward pass."""
    return _gcn2_backward(ctx, x, w1, w2, h1, out_rows, grad_rows, needs, rs)


def _gcn2_backward_dense(ctx, x, w1, w2, h1, logp, grad, needs):
    """The dense route of _gcn2_backward: a gradient that is non-zero on EVERY row (a loss over all
    vertices — the fork's live case reduces over all nodes, reference pygcn/train.py:151-155)."""
    return _gcn2_backward(ctx, x, w1, w2, h1, logp, grad, needs)


class GCN2RowsFunction(torch.autograd.Function):
    """log_softmax(Â·dropout(relu(Â·X·W1 + b1))·W2 + b2)[rows] — models.py:47-71 (upstream form) —
    with the whole backward pass of the module docstring.  Outputs: (out_rows, full log-probability
    matrix or None); the second output is not differentiable."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, graph, rows, dropout_p, seed, keep_full):
        ctx.rs = row_sets(graph, rows)
        saved_x, h1, logp = _gcn2_forward(ctx, x, w1, b1, w2, b2, graph, dropout_p, seed)
        out_rows = logp.index_select(0, rows.to(torch.int64))
        ctx.save_for_backward(saved_x, w1, w2, h1, out_rows)
        if keep_full:
            ctx.mark_non_differentiable(logp)
            return out_rows, logp
        return out_rows, None

    @staticmethod
    def backward(ctx, grad_rows, _grad_full):
        x, w1, w2, h1, out_rows = ctx.saved_tensors          # (x is z = Â·X on the reassociated path)
        grads = _gcn2_backward_rows(ctx, x, w1, w2, h1, out_rows, ctx.rs, grad_rows,
                                    ctx.needs_input_grad[:5])
        return (*grads, None, None, None, None, None)


class GCN2Function(torch.autograd.Function):
    """`model(features, adj)` — the reference call, log-probabilities of EVERY vertex
    (models.py:47-71 upstream form) — as one autograd node.  What the backward pass does depends on
    the gradient that arrives:

      * a `RowGrad` (the caller selected `output[idx_train]`, pygcn/train.py:153 — pygcn_amd/rowgrad.py):
        the rows route, on the cached row sets of (graph, idx);
      * an `NLLGrad` (pygcn_amd.functional.nll_loss over all rows) or any dense tensor: the dense route.
    Neither synchronises with the host."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, graph, dropout_p, seed):
        saved_x, h1, logp = _gcn2_forward(ctx, x, w1, b1, w2, b2, graph, dropout_p, seed)
        ctx.save_for_backward(saved_x, w1, w2, h1, logp)
        return logp

    @staticmethod
    def backward(ctx, grad):
        from .rowgrad import RowGrad
        x, w1, w2, h1, logp = ctx.saved_tensors
        needs = ctx.needs_input_grad[:5]
        if isinstance(grad, RowGrad) and grad.rows.numel() and grad.values.dtype == logp.dtype:
            _spmm.graph_unedited(ctx)             # (before the row sets follow the values)
            rs = row_sets(ctx.graph, grad.rows)
            grads = _gcn2_backward_rows(ctx, x, w1, w2, h1, logp.index_select(0, rs.rows_user), rs,
                                        grad.values, needs)
        else:
            if isinstance(grad, RowGrad):
                grad = grad.dense()
            grads = _gcn2_backward_dense(ctx, x, w1, w2, h1, logp, grad, needs)
        return (*grads, None, None, None)


class GCN2RestrictedFunction(torch.autograd.Function):
    """GCN2RowsFunction's result — log_softmax(Â·dropout(relu(Â·X·W1 + b1))·W2 + b2)[rows] — with the
    FORWARD pass restricted to the receptive field of `rows` too (opt-in: `model(x, adj, rows=idx,
    restrict_forward=True)`): layer 2 runs on the rows R alone, layer 1 on R2 = the rows layer 2 reads,
    and every activation is compact.  The same sums as the full pass for the rows it keeps, the same
    dropout mask at the same seed (dropout_rows); the full log-probability matrix never exists."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, graph, rows, dropout_p, seed):
        rs = ctx.rs = row_sets(graph, rows)
        saved_x, h1, logp_u = _gcn2_forward(ctx, x, w1, b1, w2, b2, graph, dropout_p, seed, rs)
        out_rows = logp_u if rs.sorted_unique else logp_u.index_select(0, rs.inverse)
        ctx.save_for_backward(saved_x, w1, w2, h1, out_rows)
        return out_rows

    @staticmethod
    def backward(ctx, grad_rows):
        x, w1, w2, h1, out_rows = ctx.saved_tensors          # (x is z_c = Â[R2,:]·X on the reassociated path)
        grads = _gcn2_backward(ctx, x, w1, w2, h1, out_rows, grad_rows, ctx.needs_input_grad[:5], ctx.rs,
                               restricted=True)
        return (*grads, None, None, None, None)


def gcn2_rows_restricted(x, gc1, gc2, graph, rows, dropout_p, seed):
    """output[rows] of the 2-layer model with forward AND backward pass on the rows' receptive field."""
    return GCN2RestrictedFunction.apply(x, gc1.weight, gc1.bias, gc2.weight, gc2.bias, graph, rows,
                                        float(dropout_p), seed)


def gcn2_rows(x, gc1, gc2, graph, rows, dropout_p, seed, keep_full=False):
    """(output[rows], full output or None) of the 2-layer model through the one-node path."""
    return GCN2RowsFunction.apply(x, gc1.weight, gc1.bias, gc2.weight, gc2.bias, graph, rows,
                                  float(dropout_p), seed, bool(keep_full))


def gcn2_full(x, gc1, gc2, graph, dropout_p, seed):
    """Log-probabilities of every vertex through the one-node path (GCN2Function)."""
    return GCN2Function.apply(x, gc1.weight, gc1.bias, gc2.weight, gc2.bias, graph,
                              float(dropout_p), seed)
