"""The sparse x dense product of the GraphConvolution layer as a HIP custom op with autograd.

Replaces `torch.spmm(adj, support)` (reference pygcn/layers.py:34) and the product
`adj.t() @ grad_output` that autograd runs for it (pygcn/train.py:157), plus — optionally fused
into the kernel's store — `output + self.bias` (pygcn/layers.py:35-36) and the ReLU that follows
the layer in the model (upstream form, pygcn/models.py:48).

Every call goes through the C-ABI `gcn_spmm_csr` (include/gcn_spmm.h).  No CPU / PyTorch
fallback exists: non-HIP tensors or a missing library raise.
"""
import torch

from . import _native, tuning
from .gemm import (_dense_forward, _dense_grads, _seed_fields, _weight_grad, absmax_cached, absmax_now, gemm_bf16,
                   gemm_handwritten, gemm_needs_bounds, gemm_xw256, known_absmax, layer_gemm,
                   layer_gemm_reassociable, padded_row_list, remember_absmax, weight_grad_rows)
# (names of gemm.py that callers reach as pygcn_amd.spmm.<name>: bench.py and tests/conftest.py the scheme
#  switch, code written against the module before the dense side moved out the other three)
from .gemm import DenseMMFunction, gemm_keep_bits_usable, gemm_scheme, set_bound_check, set_gemm_scheme  # noqa: F401
from .graph import CSRGraph, _require_cuda, as_graph
from .tuning import MIN_ROWS, REASSOC_MAX_WIDTH_RATIO      # (dispatch thresholds: one table)

_DTYPES = {torch.float32: _native.GCN_DTYPE_F32, torch.bfloat16: _native.GCN_DTYPE_BF16}

# Optional launch timing for bench.py: when a list is installed here, every gcn_spmm_csr launch
# is bracketed by HIP events recorded on the launch stream and (tag, start, end, graph) appended.
_timing_records = None

# Test switch: tensors whose unflagged rows are deliberately left unwritten (skip_zero_rows,
# c_select) are pre-filled with NaN instead of being allocated empty, so a consumer that reads a
# row it must not read shows up as NaN in the gradients (tests/test_spmm_gpu.py).
_poison_unwritten = False


def _maybe_poisoned(shape, dtype, device):
    if _poison_unwritten:
        return torch.full(shape, float("nan"), dtype=dtype, device=device)
    return torch.empty(shape, dtype=dtype, device=device)


def set_timing_records(records):
    """Install (or remove, with None) the list that receives per-launch HIP event pairs."""
    global _timing_records
    _timing_records = records


class PackedRows:
    """A 256-wide fp32 matrix as fixed slots next to the matrix itself: `slots` int32 [m, slot_bytes / 4], `dense`,
    read by a gather only for the rows that did not fit their slot, and `slot_bytes`, the format (include/gcn_spmm.h):
    512 (rows_pack512) — per row four 128-byte sub-slots, one per column quarter (64-bit mask, count, 29 values in
    bit order); 384 (rows_pack384) — the four masks, a header of running quarter counts and ONE pool of 87 values.
    Without `slot_bytes` the format is read off the width of `slots`."""
    __slots__ = ("slots", "dense", "slot_bytes")

    def __init__(self, slots, dense, slot_bytes=None):
        self.slots, self.dense = slots, dense
        self.slot_bytes = 4 * slots.shape[1] if slot_bytes is None else int(slot_bytes)
        if self.slot_bytes not in _PACKED_ENTRY:
            raise RuntimeError(f"PackedRows: no slot format of {self.slot_bytes} bytes (512 or 384)")


PACK512_CAPACITY = 29      # values per sub-slot (GCN_PACK512_CAPACITY)
PACK384_CAPACITY = 87      # values per slot (GCN_PACK384_CAPACITY)
_PACKED_ENTRY = {512: "gcn_spmm_csr_packed", 384: "gcn_spmm_csr_packed384"}     # slot bytes -> the gather's entry point


def rows_pack512_usable(h):
    """Can rows_pack512 take `h` as it is (fp32 [m, 256], unit column stride, 16-byte aligned rows)?"""
    return (h.is_cuda and h.dim() == 2 and h.dtype == torch.float32 and h.shape[1] == 256 and h.stride(1) == 1
            and h.stride(0) % 4 == 0 and h.data_ptr() % 16 == 0)


def rows_pack512(h):
    """PackedRows of `h` (C-ABI gcn_rows_pack512: one streaming pass, 1 KiB read and at most 512 bytes written
    per row) — the operand form of spmm_csr(graph, packed=...) for a mostly-zero activation such as the
    ReLU + dropout output that layer 2 gathers."""
    _require_cuda(h, "h")
    if not rows_pack512_usable(h):
        raise RuntimeError(f"rows_pack512: {tuple(h.shape)} {h.dtype}: fp32 [m, 256] with 16-byte aligned rows")
    slots = torch.empty((h.shape[0], 128), dtype=torch.int32, device=h.device)
    if h.shape[0]:
        _native.launch("gcn_rows_pack512", h.device, h.data_ptr(), h.stride(0), h.shape[0], slots.data_ptr())
    return PackedRows(slots, h, 512)


def rows_pack384(h):
    """PackedRows of `h` in the pooled 384-byte format (C-ABI gcn_rows_pack384: one streaming pass, 1 KiB read and
    384 bytes written per row): three 128-byte lines per gathered row instead of four.  Takes what rows_pack512
    takes (rows_pack512_usable)."""
    _require_cuda(h, "h")
    if not rows_pack512_usable(h):
        raise RuntimeError(f"rows_pack384: {tuple(h.shape)} {h.dtype}: fp32 [m, 256] with 16-byte aligned rows")
    slots = torch.empty((h.shape[0], 96), dtype=torch.int32, device=h.device)
    if h.shape[0]:
        _native.launch("gcn_rows_pack384", h.device, h.data_ptr(), h.stride(0), h.shape[0], slots.data_ptr())
    return PackedRows(slots, h, 384)


def _spmm_csr_packed(graph, packed, out, tag):
    """spmm_csr's launch for a PackedRows operand (C-ABI gcn_spmm_csr_packed / gcn_spmm_csr_packed384 by the
    operand's format): plain product, bit-identical to the dense launch on packed.dense."""
    if not isinstance(graph, CSRGraph) or not isinstance(packed, PackedRows):
        raise RuntimeError("spmm_csr: graph must be a CSRGraph and packed a PackedRows")
    B, slots = packed.dense, packed.slots
    if B.shape[0] != graph.shape[1] or B.device != graph.device or not rows_pack512_usable(B) \
            or tuple(slots.shape) != (B.shape[0], packed.slot_bytes // 4) or not slots.is_contiguous():
        raise RuntimeError(f"size mismatch, adj {graph.shape} x packed {tuple(B.shape)}")
    n_rows = graph.shape[0]
    if out is None:
        out = torch.empty((n_rows, 256), dtype=torch.float32, device=B.device)
    elif out.shape != (n_rows, 256) or out.dtype != torch.float32 or out.stride(1) != 1:
        raise RuntimeError("spmm_csr: bad `out`")
    if n_rows == 0:
        return out
    L = _native.lib()
    plan = graph.plan(torch.float32)
    ws_bytes = L.gcn_spmm_workspace_bytes(plan, 256)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=B.device) if ws_bytes else None
    with torch.cuda.device(B.device):
        rec = _timing_records
        if rec is not None:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        _native.launch(_PACKED_ENTRY[packed.slot_bytes], B.device, plan, slots.data_ptr(), B.data_ptr(), B.stride(0),
                       out.data_ptr(), out.stride(0), ws.data_ptr() if ws is not None else None, ws_bytes)
        if rec is not None:
            ev1.record()
            rec.append((tag, ev0, ev1, graph))
    return out


def spmm_csr(graph, B=None, bias=None, relu=False, out=None, tag="fwd", dropout_p=0.0, seed=0,
             b_hint=None, B2=None, c_flags=None, log_softmax=False, c_select=None,
             skip_zero_rows=False, row_base=0, c_absmax=None, packed=None):
    """C = A · B (+ bias, ReLU, inverted dropout) on the current HIP stream; A is a CSRGraph,
    B dense [n_cols, F].  The epilogue order is that of the reference model: bias
    (layers.py:35-36), F.relu (models.py:48), F.dropout (models.py:50).  `b_hint` = (row bitmap
    int32 [ceil(n_cols/32)], nnz_rows int32 [1]) device tensors from backward_with_colsum (or
    row_bitmap()): rows of B whose bit is clear are not gathered (same result, less traffic).
    `B2`: optional second block of the dense operand — the operand is then [B; B2] stacked by rows
    without being materialised (the sharded path's own rows | halo rows).
    `c_flags`: optional uint8 [n_rows] tensor of ZEROS; the kernel sets c_flags[r] = 1 where the
    stored row r has a non-zero element (gcn_epilogue.c_row_nonzero).
    `log_softmax`: store log_softmax over each row of A·B + bias (`F.log_softmax(x, dim=1)`, the
    reference model's last line) — see log_softmax_fusable() for the shapes that allow it.
    `skip_zero_rows` (with c_flags): rows of the result that are entirely zero are not stored at
    all — only the flagged rows of the returned tensor are defined.
    `c_select`: optional int32 bitmap [ceil(n_rows/32)] over the OUTPUT rows: rows whose bit is
    clear are not wanted and may be left unwritten (gcn_epilogue.c_row_select).
    `seed` may be a 1-element int64 DEVICE tensor: the kernel then reads the seed when it executes
    (hipGraph replays draw a fresh mask if the graph updates the tensor, see dropout_seed_for).
    `row_base`: added to the row index in the dropout counter — a row-block shard passes the global
    index of its first row and draws the masks of the single-GPU run.
    `c_absmax`: optional DEVICE float32 [1], zeroed by the caller: receives max|stored value| of the
    launch (gcn_epilogue.c_absmax) — the bound a scaled GEMM consuming the result needs, without a
    reduction pass; non-finite if the result holds inf / NaN.
    `packed` (a PackedRows, INSTEAD of B): the operand's rows are gathered from their 512- or 384-byte slots — the same
    products in the same order, bit-identical to the launch on packed.dense; plain product only."""
    if packed is not None:
        if (B is not None or bias is not None or relu or dropout_p or b_hint is not None or B2 is not None
                or c_flags is not None or log_softmax or c_select is not None or c_absmax is not None):
            raise RuntimeError("spmm_csr: a packed operand takes the plain product only")
        return _spmm_csr_packed(graph, packed, out, tag)
    if not isinstance(graph, CSRGraph):
        raise RuntimeError("spmm_csr: graph must be a CSRGraph")
    _require_cuda(B, "dense operand")
    n_b = B.shape[0] + (B2.shape[0] if B2 is not None else 0)
    if B.dim() != 2 or n_b != graph.shape[1]:
        raise RuntimeError(f"size mismatch, adj {graph.shape} x dense {(n_b,) + tuple(B.shape[1:])}")
    if B2 is not None:
        if B2.dim() != 2 or B2.shape[1] != B.shape[1] or B2.dtype != B.dtype or B2.device != B.device:
            raise RuntimeError("B2 must match B in width, dtype and device")
        if B2.shape[1] > 0 and B2.stride(1) != 1:
            B2 = B2.contiguous()
    if B.dtype not in _DTYPES:
        raise RuntimeError(f"spmm_csr supports float32 and bfloat16, got {B.dtype}")
    if B.device != graph.device:
        raise RuntimeError(f"adj is on {graph.device} but dense operand on {B.device}")
    if B.shape[1] > 0 and B.stride(1) != 1:
        B = B.contiguous()
    n_rows, F = graph.shape[0], B.shape[1]
    if out is None:
        out = torch.empty((n_rows, F), dtype=B.dtype, device=B.device)
    elif out.shape != (n_rows, F) or out.dtype != B.dtype or out.stride(1) != 1:
        raise RuntimeError("spmm_csr: bad `out`")
    if c_flags is not None and (c_flags.dtype != torch.uint8 or c_flags.numel() != n_rows
                                or not c_flags.is_contiguous() or c_flags.device != B.device):
        raise RuntimeError("spmm_csr: c_flags must be a contiguous uint8 [n_rows] device tensor")
    if c_select is not None and (c_select.dtype != torch.int32 or c_select.device != B.device
                                 or c_select.numel() != (n_rows + 31) // 32
                                 or not c_select.is_contiguous()):
        raise RuntimeError("spmm_csr: c_select must be a contiguous int32 bitmap [ceil(n_rows/32)]")
    if c_absmax is not None and (c_absmax.dtype != torch.float32 or c_absmax.numel() != 1
                                 or c_absmax.device != B.device):
        raise RuntimeError("spmm_csr: c_absmax must be one float32 on the operand's device")
    if n_rows == 0 or F == 0:
        return out
    if bias is not None:
        _require_cuda(bias, "bias")
        bias = bias.detach().to(torch.float32).contiguous()
        if bias.numel() != F:
            raise RuntimeError("bias must have F entries")
    L = _native.lib()
    plan = graph.plan(B.dtype)
    ws_bytes = L.gcn_spmm_workspace_bytes(plan, F)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=B.device) if ws_bytes else None
    with torch.cuda.device(B.device):      # (the timing events belong on the operand's device)
        rec = _timing_records
        if rec is not None:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        seed, seed_dev = _seed_fields(seed, B.device, "spmm_csr")
        ep = _native.GcnEpilogue(bias.data_ptr() if bias is not None else None, int(bool(relu)),
                                 float(dropout_p), seed,
                                 b_hint[0].data_ptr() if b_hint is not None else None,
                                 b_hint[1].data_ptr() if b_hint is not None else None,
                                 B2.data_ptr() if B2 is not None and B2.numel() else None,
                                 B2.stride(0) if B2 is not None and B2.numel() else 0,
                                 B.shape[0] if B2 is not None else 0,
                                 c_flags.data_ptr() if c_flags is not None else None,
                                 int(bool(log_softmax)), seed_dev,
                                 c_select.data_ptr() if c_select is not None else None,
                                 int(bool(skip_zero_rows) and c_flags is not None), int(row_base),
                                 c_absmax.data_ptr() if c_absmax is not None else None)
        _native.launch("gcn_spmm_csr_ep", B.device, plan, _DTYPES[B.dtype], B.data_ptr(), B.stride(0) if F else 0,
                       out.data_ptr(), out.stride(0), F, ep, ws.data_ptr() if ws is not None else None, ws_bytes)
        if rec is not None:
            ev1.record()
            rec.append((tag, ev0, ev1, graph))
    return out


def sddmm_csr(graph, G, B):
    """values[e] = < G[row(e), :], B[col[e], :] > for every stored entry e of `graph` (fp32 [nnz]) —
    the gradient of the adjacency VALUES of C = A · B for the gradient G of C (C-ABI gcn_sddmm_csr;
    PyTorch's `mm` derivative for a sparse first operand, sampled on A's pattern).  The reference
    never needs it (adj is a constant, pygcn/train.py:80,123); SURVEY row f4 lists it as optional."""
    if not isinstance(graph, CSRGraph):
        raise RuntimeError("sddmm_csr: graph must be a CSRGraph")
    _require_cuda(G, "G")
    _require_cuda(B, "B")
    if (G.dim() != 2 or B.dim() != 2 or G.shape[0] != graph.shape[0] or B.shape[0] != graph.shape[1]
            or G.shape[1] != B.shape[1] or G.dtype != B.dtype or G.dtype not in _DTYPES
            or G.device != graph.device or B.device != graph.device):
        raise RuntimeError(f"sddmm_csr: adj {graph.shape}, G {tuple(G.shape)} {G.dtype}, B {tuple(B.shape)} {B.dtype}")
    if G.shape[1] > 0 and G.stride(1) != 1:
        G = G.contiguous()
    if B.shape[1] > 0 and B.stride(1) != 1:
        B = B.contiguous()
    out = torch.empty(graph.nnz, dtype=torch.float32, device=G.device)
    if graph.nnz == 0:
        return out
    _native.launch("gcn_sddmm_csr", G.device, graph.plan(), _DTYPES[G.dtype], G.data_ptr(), G.stride(0),
                   B.data_ptr(), B.stride(0), G.shape[1], out.data_ptr())
    return out


def rows_pack(src, rows=None):
    """Rows `rows` (int64 index tensor; None = all) of `src` [*, F] (fp32 / bf16, F a multiple of 32)
    as BITMASK + NON-ZERO VALUES (C-ABI gcn_rows_pack_count / gcn_rows_pack_values; wire format of
    the compressed halo exchange, pygcn_amd/sharded.py): -> (bits int32 [m, F/32], offsets int64
    [m + 1] (exclusive scan of the per-row counts), vals [offsets[-1]]).  Sizing `vals` reads the
    total count on the host (one synchronisation; the exchange needs the counts there anyway)."""
    _require_cuda(src, "src")
    if src.dim() != 2 or src.dtype not in _DTYPES or src.shape[1] % 32 != 0 or src.shape[1] == 0:
        raise RuntimeError(f"rows_pack: src {tuple(src.shape)} {src.dtype}: 2-D fp32 / bf16, width a multiple of 32")
    if src.stride(1) != 1 or src.stride(0) % 4 != 0:
        src = src.contiguous()
    F, dev = src.shape[1], src.device
    if rows is not None:
        if rows.dtype != torch.int64 or rows.device != dev or rows.dim() != 1:
            raise RuntimeError("rows_pack: rows must be a 1-D int64 tensor on the device of src")
        rows = rows.contiguous()
    m = src.shape[0] if rows is None else rows.numel()
    bits = torch.empty((m, F // 32), dtype=torch.int32, device=dev)
    counts = torch.empty(m, dtype=torch.int32, device=dev)
    offsets = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    source = (_DTYPES[src.dtype], src.data_ptr(), src.stride(0), rows.data_ptr() if rows is not None else None, m, F)
    _native.launch("gcn_rows_pack_count", dev, *source, bits.data_ptr(), counts.data_ptr())
    torch.cumsum(counts, 0, out=offsets[1:])
    vals = torch.empty(int(offsets[-1]), dtype=src.dtype, device=dev)
    _native.launch("gcn_rows_pack_values", dev, *source, offsets.data_ptr(), vals.data_ptr())
    return bits, offsets, vals


def rows_unpack(bits, vals, F):
    """Inverse of rows_pack on the receiving side: bits int32 [m, F/32] and the non-zero values in
    row-major order -> dense [m, F] of vals.dtype (C-ABI gcn_bits_row_counts + gcn_rows_unpack; the
    offsets are the receiver's own scan of the bit counts, no host synchronisation)."""
    _require_cuda(bits, "bits")
    _require_cuda(vals, "vals")
    if (bits.dim() != 2 or bits.dtype != torch.int32 or bits.shape[1] * 32 != F or vals.dim() != 1
            or vals.dtype not in _DTYPES or vals.device != bits.device):
        raise RuntimeError(f"rows_unpack: bits {tuple(bits.shape)} {bits.dtype}, vals {tuple(vals.shape)} {vals.dtype}, F {F}")
    bits, vals = bits.contiguous(), vals.contiguous()
    m, dev = bits.shape[0], bits.device
    counts = torch.empty(m, dtype=torch.int32, device=dev)
    offsets = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    out = torch.empty((m, F), dtype=vals.dtype, device=dev)
    _native.launch("gcn_bits_row_counts", dev, bits.data_ptr(), m, F // 32, counts.data_ptr())
    torch.cumsum(counts, 0, out=offsets[1:])
    _native.launch("gcn_rows_unpack", dev, _DTYPES[vals.dtype], bits.data_ptr(), offsets.data_ptr(), vals.data_ptr(),
                   m, F, out.data_ptr(), out.stride(0))
    return out


def log_softmax_fusable(F, dtype):
    """True when log_softmax over rows of width F can run inside the SpMM's store: the whole row
    must sit in one wavefront (F <= 64, or 16-byte lanes with F / lane width <= 64; a freshly
    allocated support tensor satisfies the kernel's 16-byte alignment rule)."""
    if dtype not in _DTYPES:
        return False
    v = 128 // torch.finfo(dtype).bits        # elements per 16-byte lane
    return F <= 64 or (F % v == 0 and F // v <= 64)


def relu_dropout_backward(grad_out, out, scale=1.0):
    """grad_pre = out > 0 ? grad_out * scale : 0 in one streaming HIP pass
    (C-ABI gcn_relu_dropout_backward): backward of the fused ReLU (+ dropout) epilogue."""
    _require_cuda(grad_out, "grad_out")
    if grad_out.dtype not in _DTYPES or out.dtype != grad_out.dtype or out.shape != grad_out.shape:
        raise RuntimeError("relu_dropout_backward: dtype/shape mismatch")
    grad_out, out = grad_out.contiguous(), out.contiguous()
    res = torch.empty_like(grad_out)
    _native.launch("gcn_relu_dropout_backward", grad_out.device, _DTYPES[grad_out.dtype], grad_out.data_ptr(),
                   out.data_ptr(), res.data_ptr(), grad_out.numel(), float(scale))
    return res


def backward_with_colsum(grad_out, out=None, scale=1.0, log_softmax=False, skip_zero_rows=False):
    """(grad_pre, column sums of grad_pre, row-sparsity hint) in ONE pass over fp32 / bf16 [N, F]
    tensors (C-ABI gcn_relu_dropout_backward_colsum); `out=None`: no masking, grad_pre is grad_out.
    `log_softmax=True`: `out` holds log-probabilities and grad_pre = grad_out - exp(out) *
    rowsum(grad_out) (C-ABI gcn_log_softmax_backward_colsum; rows need F / lane width <= 64).  The
    hint — (row bitmap int32 [ceil(N/32)], nnz_rows int32 [1]) or None when F > 256 — can be handed to
    spmm_csr(b_hint=...) when grad_pre is the dense operand of the following product.
    `skip_zero_rows=True` (needs `out` and a hint): rows of grad_pre that are entirely zero are
    NOT written — only the rows whose hint bit is set are defined; for consumers that read those
    rows only.
    Returns None when the shape/dtype is outside the kernel's envelope (caller falls back to
    relu_dropout_backward + torch's sum)."""
    _require_cuda(grad_out, "grad_out")
    L = _native.lib()
    if (grad_out.dtype not in _DTYPES or grad_out.dim() != 2
            or not grad_out.is_contiguous() or grad_out.shape[0] == 0
            or L.gcn_bwd_colsum_workspace_bytes(grad_out.shape[0], grad_out.shape[1],
                                                _DTYPES[grad_out.dtype]) == 0
            or (out is not None and (out.dtype != grad_out.dtype or not out.is_contiguous()
                                     or out.shape != grad_out.shape))
            or (log_softmax and (out is None
                                 or grad_out.shape[1] // (16 // grad_out.element_size()) > 64))):
        return None
    n, F = grad_out.shape
    grad_pre = _maybe_poisoned(grad_out.shape, grad_out.dtype, grad_out.device) if out is not None \
        else grad_out
    colsum = torch.empty(F, dtype=torch.float32, device=grad_out.device)
    hint = None
    if F <= (256 if grad_out.dtype == torch.float32 else 512):   # a row lives inside one wavefront
        hint = (torch.empty((n + 31) // 32, dtype=torch.int32, device=grad_out.device),   # bitmap
                torch.empty(1, dtype=torch.int32, device=grad_out.device))
    skip = int(bool(skip_zero_rows) and hint is not None and out is not None)
    ws_bytes = L.gcn_bwd_colsum_workspace_bytes(n, F, _DTYPES[grad_out.dtype])
    if log_softmax:
        _native.launch("gcn_log_softmax_backward_colsum", grad_out.device,
                       _DTYPES[grad_out.dtype], grad_out.data_ptr(), out.data_ptr(), grad_pre.data_ptr(),
                       colsum.data_ptr(), n, F, hint[0].data_ptr(), hint[1].data_ptr(), skip, workspace=ws_bytes)
    else:
        _native.launch("gcn_relu_dropout_backward_colsum", grad_out.device,
                       _DTYPES[grad_out.dtype], grad_out.data_ptr(), out.data_ptr() if out is not None else None,
                       grad_pre.data_ptr() if out is not None else None, colsum.data_ptr(), n, F, float(scale),
                       hint[0].data_ptr() if hint else None, hint[1].data_ptr() if hint else None, skip,
                       workspace=ws_bytes)
    return grad_pre, colsum.to(grad_out.dtype), hint


def nll_log_softmax_backward(logp, target, coef):
    """(grad_pre, column sums) for the gradient of a mean NLL loss over ALL rows of log-probabilities
    `logp` [n, F] (C-ABI gcn_nll_log_softmax_backward_colsum): grad_pre = coef·(onehot(target) −
    exp(logp)) and the bias gradient's column sums in ONE sweep that reads logp and the labels and
    writes grad_pre — the [n, F] loss gradient (one non-zero per row) is never materialised.
    `target` int64 [n] with entries in [0, F), `coef` DEVICE float32 [1].  None when the shape is
    outside the kernel's envelope (a row must sit in one wavefront)."""
    _require_cuda(logp, "logp")
    L = _native.lib()
    if (logp.dtype not in _DTYPES or logp.dim() != 2 or not logp.is_contiguous() or logp.shape[0] == 0
            or target.dtype != torch.int64 or target.numel() != logp.shape[0] or not target.is_contiguous()
            or target.device != logp.device or coef.dtype != torch.float32 or coef.numel() != 1
            or coef.device != logp.device
            or L.gcn_bwd_colsum_workspace_bytes(logp.shape[0], logp.shape[1], _DTYPES[logp.dtype]) == 0
            or logp.shape[1] // (16 // logp.element_size()) > 64):
        return None
    n, F = logp.shape
    grad_pre = torch.empty_like(logp)
    colsum = torch.empty(F, dtype=torch.float32, device=logp.device)
    _native.launch("gcn_nll_log_softmax_backward_colsum", logp.device,
                   _DTYPES[logp.dtype], target.data_ptr(), coef.data_ptr(), logp.data_ptr(),
                   grad_pre.data_ptr(), colsum.data_ptr(), n, F,
                   workspace=L.gcn_bwd_colsum_workspace_bytes(n, F, _DTYPES[logp.dtype]))
    return grad_pre, colsum.to(logp.dtype)


def pack_row_flags(nz):
    """bool [n] -> the operand hint (bitmap int32 [ceil(n/32)], count int32 [1]); torch ops."""
    n = nz.numel()
    pad = (-n) % 32
    if pad:
        nz = torch.cat([nz, torch.zeros(pad, dtype=torch.bool, device=nz.device)])
    w = (nz.view(-1, 32).to(torch.int64) << torch.arange(32, device=nz.device)).sum(1)
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    return w, nz.sum().to(torch.int32).reshape(1)


def unpack_row_flags(bits, n):
    """Inverse of pack_row_flags: bitmap int32 -> bool [n]."""
    sh = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits[:, None] >> sh) & 1).bool().reshape(-1)[:n]


def row_bitmap(B):
    """(bitmap, count) hint for a dense operand: bit r set iff row r of B has a non-zero element
    (torch ops; the backward pass gets the same thing for free from backward_with_colsum)."""
    return pack_row_flags((B != 0).any(1))


def _grad_pre_and_bias(grad_out, out, relu, scale, want_bias, log_softmax=False,
                       skip_zero_rows=False):
    """Shared by the single-GPU and sharded autograd functions: apply the fused-epilogue mask (or
    the log_softmax backward) and (optionally) produce the bias gradient, in one HIP pass when the
    shape allows.  Returns (grad_pre, grad_bias, row-sparsity hint or None).  With
    `skip_zero_rows` and a hint in the result, only the rows of grad_pre whose hint bit is set
    are defined (backward_with_colsum)."""
    grad_bias = None
    if want_bias or log_softmax:
        fused = backward_with_colsum(grad_out.contiguous(), out if (relu or log_softmax) else None,
                                     scale, log_softmax, skip_zero_rows and (relu or log_softmax))
        if fused is not None:
            return fused if want_bias else (fused[0], None, fused[2])
    if log_softmax:   # shapes outside the kernel's envelope (e.g. 7 classes): torch ops
        g32, o32 = grad_out.float(), out.float()
        grad_out = (g32 - o32.exp() * g32.sum(1, keepdim=True)).to(grad_out.dtype)
    if relu:
        grad_out = relu_dropout_backward(grad_out, out, scale)
    if want_bias:
        grad_bias = grad_out.sum(0)
    return grad_out, grad_bias, None


def dropout_scale(p):
    """1 / (keep probability) of the fused dropout at rate `p` — of the probability the kernels
    actually keep with: the threshold is 16 bits, T = clamp(round(p · 65536), 1, 65535), an element
    survives with probability (65536 − T) / 65536, and both the forward scale (C-ABI, struct
    gcn_epilogue) and the backward mask scale are 65536 / (65536 − T), so E[dropout(x)] = x
    exactly.  Equal to 1 / (1 − p) at p = 1/2 and within 2^-17 relative elsewhere."""
    if not p > 0.0:
        return 1.0
    import numpy as np
    t = int(np.float64(np.float32(p)) * 65536.0 + 0.5)
    thresh = min(65535, max(1, t))
    return float(np.float32(65536.0) / np.float32(65536 - thresh))


def next_dropout_seed(device=None):
    """64-bit seed of one fused-dropout launch, drawn the way `F.dropout` draws on a GPU in the
    reference model (pygcn/models.py:50 upstream): from the DEVICE's default generator — its seed
    (set by torch.manual_seed / torch.cuda.manual_seed) and its Philox offset, which is advanced —
    so it is reproducible under torch.manual_seed, needs no device synchronisation and leaves
    torch's CPU generator alone (a caller sharing that generator sees the stream the reference
    would give it).  CPU tensors (test stand-ins of the sharded path only) draw from the CPU
    generator, as F.dropout on CPU does."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
            else torch.device("cpu")
    if device.type != "cuda":
        return int(torch.empty((), dtype=torch.int64).random_().item())
    index = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[index]
    offset = gen.get_offset()
    gen.set_offset(offset + 4)          # one Philox counter step, like one dropout launch
    mixed = (gen.initial_seed() * 0x9E3779B97F4A7C15 + (offset // 4 + 1) * 0xD1B54A32D192ED03)
    return mixed & 0xFFFFFFFFFFFFFFFF


_device_seeds = {}


def dropout_seed_for(tensor):
    """Seed of one fused-dropout launch on `tensor`'s device.  Normally a host integer derived
    from the device generator's (seed, offset) (next_dropout_seed).  While the stream is being captured into a
    hipGraph a host seed would be frozen into the captured kernel arguments — the same mask on
    every replay — so the launch then reads a per-device int64 tensor that an op recorded in the
    same capture advances: every replay masks differently.  The tensor is created by the first
    eager dropout launch on the device (the warm-up steps torch requires before a capture)."""
    if not tensor.is_cuda:
        return next_dropout_seed(tensor.device)
    capturing = torch.cuda.is_current_stream_capturing()
    key = tensor.device.index if tensor.device.index is not None else torch.cuda.current_device()
    t = _device_seeds.get(key)
    if t is None:
        if capturing:
            raise RuntimeError("run one training step with dropout before capturing it into a "
                               "hipGraph (the device-resident dropout seed is created on first use)")
        # start value: the default generator's seed (torch.manual_seed), read without advancing
        # the generator — creating the tensor must not shift the stream of host seeds
        t = _device_seeds[key] = torch.full((1,), torch.initial_seed() & (2 ** 63 - 1),
                                            dtype=torch.int64, device=tensor.device)
    if not capturing:
        return next_dropout_seed(tensor.device)
    t.add_(0x9E3779B97F4A7C15 - (1 << 64))   # odd increment, wraps; recorded in the capture
    return t


def dropout_rows(h, rows, p, seed, row_base=0):
    """IN PLACE on the compact tensor h [m, F] (fp32 / bf16, unit column stride, any row pitch) whose
    row r stands for row rows[r] of a full-height tensor: h[r, f] = keep ? h[r, f] · s : 0 with the keep
    bit and the scale of the fused epilogues at (seed, rows[r] + row_base, f) — C-ABI gcn_dropout_rows.
    `spmm_csr(g, S, relu=True, dropout_p=p, seed=σ)[rows]` and `dropout_rows(spmm_csr(g, S,
    relu=True)[rows], rows, p, σ)` are the same bits.  `rows`: int64 device list, any order, repeats
    allowed, or None = 0 .. m-1; `seed` as in spmm_csr (a 1-element int64 device tensor is read when the
    kernel runs).  Returns h."""
    _require_cuda(h, "h")
    if h.dim() != 2 or h.dtype not in _DTYPES or (h.shape[1] > 0 and h.stride(1) != 1):
        raise RuntimeError("dropout_rows: h must be a 2-D float32 / bfloat16 tensor with unit column stride")
    m, F = h.shape
    if rows is not None:
        if (rows.dtype != torch.int64 or rows.device != h.device or rows.dim() != 1 or rows.numel() != m
                or not rows.is_contiguous()):
            raise RuntimeError("dropout_rows: rows must be a contiguous int64 device list, one entry per row of h")
    if m == 0 or F == 0:
        return h
    seed, seed_dev = _seed_fields(seed, h.device, "dropout_rows")
    _native.launch("gcn_dropout_rows", h.device, _DTYPES[h.dtype], h.data_ptr(), h.stride(0) if m > 1 else max(h.stride(0), F),
                   rows.data_ptr() if rows is not None else None, m, F, float(p), seed, seed_dev, int(row_base))
    return h


def check_fused_epilogue(relu, dropout_p, log_softmax=False):
    """The argument rules of the fused epilogues, for every layer function's forward."""
    if dropout_p > 0.0 and not relu:
        raise RuntimeError("fused dropout needs the fused ReLU (out > 0 encodes the mask)")
    if log_softmax and relu:
        raise RuntimeError("log_softmax cannot be combined with the fused ReLU / dropout")


def keep_graph(ctx, graph):
    """`ctx.graph` of an autograd node, with the version counter of the graph's values beside it: the graph is
    no saved tensor, so autograd's own check does not see an in-place edit of `graph.val` between the forward
    pass and its backward pass (graph_unedited does)."""
    ctx.graph = graph
    ctx.val_version = graph.val._version if isinstance(graph, CSRGraph) else None


def graph_unedited(ctx):
    """Raises, in a backward pass, when ctx.graph's values were edited in place since keep_graph(): the saved
    activations belong to the old matrix, the transpose and the row blocks would come from the new one."""
    graph = ctx.graph
    if ctx.val_version is not None and graph.val._version != ctx.val_version:
        raise RuntimeError(
            f"pygcn_amd: the values of {graph!r}, which this backward pass needs for gradient computation, have "
            f"been modified by an inplace operation: graph.val is at version {graph.val._version}; expected version "
            f"{ctx.val_version} instead. Edit the values (val.mul_, row_normalize_, sym_normalize_, an optimizer "
            "step) between steps, not between a forward pass and its backward pass.")


class SpMMFunction(torch.autograd.Function):
    """out = dropout(relu(A · B + bias)) with every stage optional and fused into the kernel's
    store;  grad_B = A^T · grad_pre;  grad_bias = column sums of grad_pre, where
    grad_pre = grad_out, masked and scaled through `out > 0` when ReLU (+ dropout) was fused.
    `adj` never receives a gradient (it is a loaded constant in the reference: train.py:80,123).
    Only the graph handle (and the output, for a fused ReLU) is kept for backward — not B and no
    dropout mask."""

    @staticmethod
    def forward(ctx, graph, B, bias, relu=False, dropout_p=0.0, seed=0):
        check_fused_epilogue(relu, dropout_p)
        keep_graph(ctx, graph)
        ctx.has_bias = bias is not None
        ctx.relu = bool(relu)
        ctx.scale = dropout_scale(dropout_p)
        out = spmm_csr(graph, B, bias=bias, relu=relu, dropout_p=dropout_p, seed=seed)
        if relu:
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        graph_unedited(ctx)
        grad_B = None
        out = ctx.saved_tensors[0] if ctx.relu else None
        grad_out, grad_bias, hint = _grad_pre_and_bias(grad_out, out, ctx.relu, ctx.scale,
                                                       ctx.has_bias and ctx.needs_input_grad[2])
        if ctx.needs_input_grad[1]:
            # gradients of a loss on few labelled rows are non-zero on few rows: the hint lets the
            # transpose product skip the all-zero rows of its dense operand
            grad_B = spmm_csr(ctx.graph.t(), grad_out.contiguous(), tag="bwd", b_hint=hint)
        return None, grad_B, grad_bias, None, None, None


_row_compaction = False


def set_row_compaction(enabled):
    """OPT-IN (default off since round 3): row compaction of the layer-by-layer path's gradient
    GEMMs reads two device counters on the host (two stream synchronisations per layer backward,
    only for graphs of >= MIN_ROWS vertices).  The model-level paths need none of it — a loss on
    selected rows reaches the layers as a structural RowGrad (pygcn_amd/rowgrad.py, fused.py) — so
    by default no backward pass synchronises with the host; a caller that composes bare layers
    under a row-sparse dense gradient can switch this on (never active during hipGraph capture)."""
    global _row_compaction
    _row_compaction = bool(enabled)


def _hint_will_be_used(n, F, element_size, aligned, nz_rows):
    """THE host mirror of the device-side rule (use_row_flags in gcn_spmm.hip): the product skips the
    flagged-zero rows of its dense operand [n, F] below 3/4 non-zero rows in the wide kernel (16-byte
    lanes, more than 32 of them per row; `aligned`: unit column stride, base and row pitch multiples
    of 16 bytes) and below 1/8 in the narrow one."""
    v = 16 // element_size
    wide = aligned and F % v == 0 and F // v > 32
    return tuning.below(nz_rows, n, tuning.HINT_WIDE_MAX_SHARE if wide else tuning.HINT_NARROW_MAX_SHARE)


class GraphConvFunction(torch.autograd.Function):
    """The whole layer — `torch.mm(input, weight)`, `torch.spmm(adj, support)`, `+ bias`
    (reference pygcn/layers.py:33-36) and the optional fused ReLU / dropout — as ONE autograd
    node, so that what the backward pass learns about the sparsity of its tensors can be used by
    the next stage instead of being re-discovered:

        grad_pre  = mask(grad_out)                 -> row bitmap + count   (one HIP pass)
        grad_sup  = Aᵀ · grad_pre   (skips zero rows of grad_pre) -> byte flags of ITS non-zero rows
        grad_W    = inputᵀ · grad_sup,  grad_input = grad_sup · Wᵀ   on the non-zero rows only

    With a loss on few labelled vertices (`nll_loss(output[idx_train], …)`, pygcn/train.py:153)
    grad_out of the last layer is non-zero on |idx_train| rows and grad_sup on their neighbourhood:
    5 % and 16 % of the rows at bench config C4."""

    @staticmethod
    def forward(ctx, input, weight, bias, graph, relu=False, dropout_p=0.0, seed=0,
                log_softmax=False):
        check_fused_epilogue(relu, dropout_p, log_softmax)
        keep_graph(ctx, graph)
        ctx.relu = bool(relu)
        ctx.log_softmax = bool(log_softmax)
        ctx.scale = dropout_scale(dropout_p)
        # (a layer input that needs no gradient is the constant feature matrix: its maximum is
        #  computed once and reused as the scaled GEMM's bound)
        # (bounds exist for the scaled fp16 scheme alone: the default three-part bf16 GEMMs need none)
        bounds = gemm_needs_bounds()
        x_bound = absmax_cached(input) if (bounds and input.dtype == torch.float32 and not input.requires_grad
                                           and input.is_cuda) else None
        const_input = not input.requires_grad and input.is_cuda
        if bounds and x_bound is None and input.dtype == torch.float32 and input.is_cuda:
            x_bound = known_absmax(input)       # (left by the layer that produced this tensor)
        # REASSOCIATED for a constant input on the shape the GEMM kernel carries the epilogue for
        # (256 -> 256 fp32): out = epilogue((A·input)·W + b).  Same two kernels and bytes in
        # forward; z = A·input of this forward pass is then all the backward pass needs for
        # grad_W = zᵀ·grad_pre — no sparse product in backward (pygcn_amd/fused.py does the same
        # inside the one-node path).
        ctx.reassoc = False
        if (const_input and not log_softmax and isinstance(graph, CSRGraph)
                and layer_gemm_reassociable(input, weight, bias)):
            z = spmm_csr(graph, input)
            ctx.z_bound = y_max = None
            if x_bound is not None:
                ctx.z_bound = graph.inf_norm() * x_bound * 1.0001
                y_max = torch.zeros(1, dtype=torch.float32, device=input.device)
            out = layer_gemm(z, weight, ctx.z_bound, y_max, bias=bias, relu=relu, dropout_p=dropout_p,
                             seed=seed)
            if out is not None:
                if y_max is not None:
                    remember_absmax(out, y_max)      # the next layer's GEMM scales by it
                ctx.reassoc = True
                ctx.save_for_backward(z, weight, *([out] if relu else []))
                return out
            del z
        ctx.x_bound = x_bound
        support = _dense_forward(input, weight, x_bound)
        out = spmm_csr(graph, support, bias=bias, relu=relu, dropout_p=dropout_p, seed=seed,
                       log_softmax=log_softmax)
        if relu or log_softmax:
            ctx.save_for_backward(input, weight, out)
        else:
            ctx.save_for_backward(input, weight)
        return out

    @staticmethod
    def _backward_rows(ctx, grad):
        """The backward pass for a row-sparse gradient (pygcn_amd/rowgrad.py): `grad.rows` are the only
        rows of grad_out that can be non-zero.  Returns the gradient tuple, or None where this
        route does not apply (the caller then continues with the dense tensor)."""
        from . import fused
        from .rowgrad import RowGrad
        input, weight = ctx.saved_tensors[:2]
        out = ctx.saved_tensors[2] if (ctx.relu or ctx.log_softmax) else None
        need_in, need_w, need_b = ctx.needs_input_grad[:3]
        graph, rows, vals = ctx.graph, grad.rows, grad.values
        if not isinstance(graph, CSRGraph) or rows.numel() == 0 or vals.dtype != input.dtype:
            return None
        dev, dt = vals.device, vals.dtype
        f32 = dt == torch.float32
        if ctx.log_softmax:
            # ---- last layer: log_softmax backward on the compact rows (the loss-rows stage of fused.py; this
            # route's torch form sums the bias gradient AFTER rounding to bf16), then Âᵀ on its block
            rs = fused.row_sets(graph, rows)
            out_rows = out.index_select(0, rs.rows_user)
            gp, colsum = fused._loss_rows_stage(vals, out_rows, need_b, rs, round_first=True)
            grad_bias = colsum.to(dt) if need_b else None
            if not (need_in or need_w):
                return None, None, grad_bias, None, None, None, None, None
            grad_sup = spmm_csr(rs.at_block, gp.contiguous(), tag="bwd")          # [|R2|, Fout], compact
            gs_bound = (graph.t().inf_norm() * absmax_now(gp) * 1.0001) \
                if f32 else None
            grad_w = grad_in = None
            if need_w:
                grad_w = weight_grad_rows(input, grad_sup, rs.rows2_padded, None, ctx.x_bound, gs_bound,
                                          n_list=rs.n2) if (f32 and gemm_handwritten() and
                                                            (ctx.x_bound is not None or not gemm_needs_bounds())) else None
                if grad_w is None:
                    grad_w = _weight_grad(input.index_select(0, rs.rows2), grad_sup)
            if need_in:
                wt = weight.t().contiguous()
                y_max = torch.zeros(1, dtype=torch.float32, device=dev) if f32 else None
                part = gemm_xw256(grad_sup, wt, gs_bound, y_max)
                if part is None:
                    part, y_max = gemm_bf16(grad_sup, wt), None
                if part is None:
                    part, y_max = torch.mm(grad_sup, wt), None
                grad_in = RowGrad(rs.rows2, part, input.shape[0],
                                  meta={"padded": rs.rows2_padded, "absmax": y_max})
            return grad_in, grad_w, grad_bias, None, None, None, None, None
        if ctx.reassoc and not need_in:
            # ---- a first layer evaluated as (A·x)·W: mask on the compact rows, grad_W from the saved z
            meta = grad.meta or {}
            if meta.get("padded") is None:        # (rows of unknown structure: sorted-unique lists only)
                return None
            g = vals
            bound = meta.get("absmax")
            if ctx.relu:
                g = relu_dropout_backward(vals.contiguous(), out.index_select(0, rows), ctx.scale)
                bound = bound * ctx.scale if bound is not None else None
            grad_bias = grad_w = None
            if need_b and need_w and f32 and g.is_contiguous():      # (both from ONE pass over g: weight_grad_rows)
                both = weight_grad_rows(input, g, meta["padded"], None, ctx.z_bound, bound, n_list=rows.numel(),
                                        colsum_g=True)
                if both is not None:
                    grad_w, grad_bias = both[0], both[1].to(dt)
            if need_b and grad_bias is None:
                sums = backward_with_colsum(g) if g.is_contiguous() else None
                grad_bias = sums[1] if sums is not None else g.float().sum(0).to(dt)
            if need_w and grad_w is None:
                grad_w = weight_grad_rows(input, g, meta["padded"], None, ctx.z_bound, bound,
                                          n_list=rows.numel()) if (f32 and (ctx.z_bound is not None or not gemm_needs_bounds())) else None
                if grad_w is None:
                    grad_w = _weight_grad(input.index_select(0, rows), g)
            return None, grad_w, grad_bias, None, None, None, None, None
        return None

    @staticmethod
    def backward(ctx, grad_out):
        from .rowgrad import RowGrad
        graph_unedited(ctx)
        if isinstance(grad_out, RowGrad):
            res = GraphConvFunction._backward_rows(ctx, grad_out)
            if res is not None:
                return res
            grad_out = grad_out.dense()
        input, weight = ctx.saved_tensors[:2]
        out = ctx.saved_tensors[2] if (ctx.relu or ctx.log_softmax) else None
        need_in, need_w, need_b = ctx.needs_input_grad[:3]
        graph_t = ctx.graph.t()
        n = graph_t.shape[0]
        # what follows reads the host-side count of non-zero gradient rows (a stream
        # synchronisation): large graphs only, never while capturing a hipGraph
        sync_ok = (_row_compaction and n >= MIN_ROWS and (need_in or need_w)
                   and not torch.cuda.is_current_stream_capturing())
        # ... and when it may, the fused backward pass does not even write the all-zero rows of
        # grad_pre: every consumer below reads the rows flagged in the bitmap only
        grad_pre, grad_bias, hint = _grad_pre_and_bias(grad_out, out, ctx.relu, ctx.scale, need_b,
                                                       ctx.log_softmax, skip_zero_rows=sync_ok)
        if not (need_in or need_w):
            return None, None, grad_bias, None, None, None, None, None
        if ctx.reassoc:          # (input is z = A·x here; x itself needs no gradient)
            z, grad_w = input, None
            if sync_ok and hint is not None:
                nz_rows = int(hint[1].item())
                if tuning.below(nz_rows, grad_pre.shape[0], tuning.SPARSE_GEMM_MAX_SHARE):   # the listed rows only
                    rows = torch.nonzero(unpack_row_flags(hint[0], grad_pre.shape[0])).squeeze(1)
                    lst = padded_row_list(rows)
                    grad_w = weight_grad_rows(z, grad_pre, lst, lst, ctx.z_bound, None, n_list=nz_rows)
                    if grad_w is None:
                        grad_w = _weight_grad(z.index_select(0, rows), grad_pre.index_select(0, rows))
                elif ctx.relu:       # rows of grad_pre whose bit is clear were not written
                    keep = unpack_row_flags(hint[0], grad_pre.shape[0])[:, None]
                    grad_pre = torch.where(keep, grad_pre, torch.zeros_like(grad_pre[:1]))
            if grad_w is None:
                grad_pre = grad_pre.contiguous()
                g_bound = None
                if ctx.z_bound is not None:      # |mask(grad_out)| <= scale * max|grad_out|
                    g_bound = known_absmax(grad_out)
                    g_bound = g_bound * ctx.scale if g_bound is not None else \
                        absmax_now(grad_pre)
                grad_w = _weight_grad(z, grad_pre, ctx.z_bound, g_bound)
            return None, grad_w, grad_bias, None, None, None, None, None
        c_flags = rows = None
        compact = sync_ok and hint is not None
        unwritten = compact and (ctx.relu or ctx.log_softmax)   # grad_pre: flagged rows only
        nz_rows = int(hint[1].item()) if compact else None
        if (compact and not need_in and tuning.below(nz_rows, grad_pre.shape[0], tuning.SPARSE_GEMM_MAX_SHARE)
                and input.shape[1] <= REASSOC_MAX_WIDTH_RATIO * grad_pre.shape[1]):
            # First layer (its input needs no gradient) under a row-sparse grad_pre:
            #     grad_W = inputᵀ · (Aᵀ · grad_pre) = (A · input)ᵀ · grad_pre,
            # and only the rows of A · input that meet a non-zero row of grad_pre take part: a
            # forward product restricted to those rows (c_select = the bitmap of grad_pre) and a
            # GEMM over them replace the transpose product and the full-height GEMM.  The
            # product here gathers rows of width Fin where the transpose product gathers width
            # Fout, and z is [n_rows, Fin]: it pays (and is bounded in memory) only while Fin is
            # not much wider than Fout — a 1433 -> 16 layer keeps the transpose product.
            z = spmm_csr(ctx.graph, input, tag="bwd", c_select=hint[0],
                         out=_maybe_poisoned((ctx.graph.shape[0], input.shape[1]), input.dtype,
                                             input.device))
            rows = torch.nonzero(unpack_row_flags(hint[0], grad_pre.shape[0])).squeeze(1)
            grad_w = _weight_grad(z.index_select(0, rows), grad_pre.index_select(0, rows))
            return None, grad_w, grad_bias, None, None, None, None, None
        es = grad_pre.element_size()
        aligned = grad_pre.stride(1) == 1 and grad_pre.data_ptr() % 16 == 0 and (grad_pre.stride(0) * es) % 16 == 0
        if unwritten and not _hint_will_be_used(*grad_pre.shape, es, aligned, nz_rows):
            # the product below would gather every row: give the unwritten ones their zeros
            keep = unpack_row_flags(hint[0], grad_pre.shape[0])[:, None]
            grad_pre = torch.where(keep, grad_pre, torch.zeros_like(grad_pre[:1]))
        if compact and tuning.below(nz_rows, grad_pre.shape[0], tuning.SPARSE_FLAGS_MAX_SHARE):
            c_flags = torch.zeros(n, dtype=torch.uint8, device=grad_pre.device)
        # with the flags requested, all-zero rows of the product are not even written: the GEMMs
        # below read the flagged rows only
        grad_sup = spmm_csr(graph_t, grad_pre.contiguous(), tag="bwd", b_hint=hint, c_flags=c_flags,
                            skip_zero_rows=c_flags is not None,
                            out=_maybe_poisoned((n, grad_pre.shape[1]), grad_pre.dtype, grad_pre.device)
                            if c_flags is not None else None)
        if c_flags is not None:
            rows = torch.nonzero(c_flags).squeeze(1)
            if not tuning.below(rows.numel(), n, tuning.SPARSE_GEMM_MAX_SHARE):     # too dense to pay: real zeros
                rows = None
                grad_sup = torch.where(c_flags.bool()[:, None], grad_sup, torch.zeros_like(grad_sup[:1]))
        grad_in, grad_w = _dense_grads(input, weight, grad_sup, need_in, need_w, rows)
        return grad_in, grad_w, grad_bias, None, None, None, None, None


def spmm(adj, dense, bias=None):
    """Drop-in for `torch.spmm(adj, dense)` (+ optional fused bias) with autograd: a thin caller
    of the registered operator `torch.ops.pygcn_amd.spmm_csr` (pygcn_amd/ops.py)."""
    from .ops import sparse_mm
    return sparse_mm(adj, dense, bias)
