"""The dense side of the GraphConvolution layer: `torch.mm(input, weight)` (reference
pygcn/layers.py:33) and its two gradient products through the hand-written MFMA GEMMs of the C-ABI
(include/gcn_spmm.h: gcn_gemm_xw256_*, gcn_gemm_xw_bf16, gcn_gemm_atg*), the switch between their
arithmetic schemes, and DenseMMFunction, the autograd node over them.  Where a kernel does not
carry a shape, the wrappers say so (None) and the callers use torch.mm; a missing library raises.
"""
import weakref

import torch

from . import _native
from .tuning import K_SPLIT, MIN_ROWS

_gemm_scheme = "bf16x3"
_bound_check = False


def gemm_scheme():
    """The current scheme of the fp32 256 -> 256 GEMMs (set_gemm_scheme)."""
    return _gemm_scheme


def gemm_handwritten():
    """Are the 256-wide fp32 GEMMs on the hand-written MFMA kernels (either decomposition)?"""
    return _gemm_scheme != "exact"


def gemm_needs_bounds():
    """Only the scaled two-part fp16 scheme needs an upper bound of max|operand|."""
    return _gemm_scheme == "h2"


def set_bound_check(enabled):
    """DEBUG switch: after every scaled GEMM that reports max|Y|, read it on the host (a stream
    synchronisation) and raise if it is not finite.  The kernels never hide an overflow — a bound
    that was too small makes y_absmax inf / NaN (its integer maximum keeps those patterns), and a
    consumer scaled by a non-finite bound stores NaN — so a wrong bound ends in a NaN loss, not in
    plausible numbers; this switch names the first launch that overflowed."""
    global _bound_check
    _bound_check = bool(enabled)


def set_gemm_scheme(name):
    """How the fp32 256 -> 256 GEMMs of the layers are evaluated:
    "bf16x3" (default since round 4): three bf16 parts per operand, six MFMAs per product — a 24-bit
        significand, the fp32-EQUIVALENT of the reference's `torch.mm` (pygcn/layers.py:33); no
        scaling, no bounds, fp32's range; forward (with the layer epilogue), grad_input (with the
        mask) and the gather-fused weight gradients;
    "h2": the scaled two-part fp16 MFMA kernels (22-bit significand, half the matrix work, 4e-7
        normwise vs fp64 on well-scaled data) wherever a bound of max|X| is known — opt-in;
    "exact": no hand-written fp32 GEMM at all — every dense product is `torch.mm` (hipBLASLt's exact
        fp32 MFMA path, the arithmetic of the reference's `torch.mm(input, self.weight)`,
        pygcn/layers.py:33) and the layers keep the reference's order Â·(X·W).  The SpMM kernels
        are the same in all three."""
    global _gemm_scheme
    if name not in ("h2", "bf16x3", "exact"):
        raise RuntimeError("gemm scheme must be 'h2', 'bf16x3' or 'exact'")
    _gemm_scheme = name


def _device_key(device):
    """Key of a per-device cache (a HIP tensor's device carries its index; None is the CPU of the
    sharded path's test stand-ins)."""
    return device.index if device.index is not None else -1


def _mfma_rows(t, dtype, width, pitch, align=16):
    """Rows the MFMA kernels can read: a 2-D `dtype` tensor of `width` columns (None: any) with unit
    column stride, a row pitch that is a multiple of `pitch` elements and a base address that is a
    multiple of `align` bytes."""
    return (t.dtype == dtype and t.dim() == 2 and (width is None or t.shape[1] == width)
            and t.stride(1) == 1 and t.stride(0) % pitch == 0 and t.data_ptr() % align == 0)


def _seed_fields(seed, device, who):
    """(seed, seed_dev) of an epilogue struct: a 1-element int64 DEVICE tensor is read by the kernel
    when it executes (hipGraph capture, spmm.dropout_seed_for); anything else is a host integer, cut
    to 64 bits."""
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or seed.numel() != 1 or seed.device != device:
            raise RuntimeError(f"{who}: a tensor seed must be one int64 on the operand's device")
        return 0, seed.data_ptr()
    return int(seed) & 0xFFFFFFFFFFFFFFFF, None


def gemm_keep_bits_usable(X, rows=None, dropout_p=0.0):
    """Does gemm_xw256 run this operand on the kernel that can write / read the ONE-BIT form of a ReLU /
    dropout result (C-ABI gcn_gemm_epilogue.keep_bits_out / mask_bits: contiguous rows, the three-part
    scheme, dropout_p in {0, 1/2})?"""
    return (_gemm_scheme == "bf16x3" and rows is None and X.dtype == torch.float32 and X.is_cuda and X.dim() == 2
            and X.shape[1] == 256 and X.stride(1) == 1 and X.stride(0) < (1 << 21) and dropout_p in (0.0, 0.5))


def gemm_xw256(X, W, x_bound=None, y_absmax=None, rows=None, mask_src=None, mask_scale=1.0,
               bias=None, relu=False, dropout_p=0.0, seed=0, mask_rows=None, row_base=0,
               keep_bits_out=None, mask_bits=None):
    """X[M,256] · W[256,256] through the hand-written MFMA kernels (fp32 in/out, fp32-level
    accuracy).  None if the operands do not fit the kernels' fixed shape / alignment (the caller
    then uses torch.mm — hipBLASLt).

    Default scheme "bf16x3": C-ABI gcn_gemm_xw256_f32_b3 — three bf16 parts per operand, six MFMAs
    per product: a 24-bit significand, the fp32-equivalent of the reference's `torch.mm`; no scaling,
    `x_bound` is ignored.  Scheme "h2" (set_gemm_scheme; 22-bit significand, half the matrix work):
    C-ABI gcn_gemm_xw256_f32_h2 — power-of-two scaling + two fp16 parts,
    three MFMAs per product.  `x_bound` (DEVICE float tensor [1]) is any upper bound of max|X|; if
    the caller has none, max|X| is computed here by one reduction pass.  `y_absmax` (DEVICE float
    tensor [1], zeroed by the caller) receives max|Y|, from which a layer derives the next bound
    without a pass over the data.  `rows` (int32 device list): output row r is the product of
    input row rows[r] — a gather fused into the kernel's loads.  `mask_src` ([*, 256] fp32, read
    at the same input rows, or — `mask_rows`, an int32 device list — at mask_rows[r] for output
    row r): the store becomes mask_src > 0 ? y * mask_scale : 0, the backward of a
    fused ReLU / dropout epilogue, in the GEMM's own store (None if it cannot be fused).
    `bias` / `relu` / `dropout_p` / `seed`: FORWARD epilogue in the store, y = dropout(relu(acc +
    bias)) with the same Philox keep function as the SpMM epilogue — for a layer evaluated as
    (Â·X)·W + b, whose last stage is the GEMM (None if it cannot be fused).
    `keep_bits_out` (int32 [M, 8], with relu; only where gemm_keep_bits_usable()): the launch also writes
    `out > 0` as one bit per element; `mask_bits` (such a tensor, given NEXT TO mask_src): the backward mask
    is read from the bits (32 bytes per row instead of 1 KiB) where the launch can, from mask_src where not.
    Both schemes carry every option; "bf16x3" keeps full accuracy for 1e-30 <= |x| <= 3e38 (below
    that its low-order parts underflow — tests/test_gemm_gpu.py)."""
    if (_gemm_scheme == "exact" or not X.is_cuda or not _mfma_rows(X, torch.float32, 256, 4)
            or W.dtype != torch.float32 or tuple(W.shape) != (256, 256) or X.shape[0] == 0 or W.stride(1) != 1):
        return None
    L = _native.lib()
    has_fwd_ep = bias is not None or relu or dropout_p > 0.0
    if has_fwd_ep and (mask_src is not None
                       or (bias is not None and (bias.dtype != torch.float32 or bias.numel() != 256
                                                 or not bias.is_contiguous() or bias.data_ptr() % 16))):
        return None
    if mask_src is not None and (not _mfma_rows(mask_src, torch.float32, 256, 4) or mask_src.device != X.device):
        return None
    if mask_rows is not None and (mask_rows.dtype != torch.int32 or not mask_rows.is_contiguous()
                                  or mask_rows.device != X.device
                                  or mask_rows.numel() < (rows.numel() if rows is not None else X.shape[0])):
        raise RuntimeError("gemm_xw256: mask_rows must be a contiguous int32 device list, one entry per output row")
    if rows is not None:
        if rows.dtype != torch.int32 or not rows.is_contiguous() or rows.device != X.device:
            raise RuntimeError("gemm_xw256: rows must be a contiguous int32 device tensor")
    m_out = rows.numel() if rows is not None else X.shape[0]
    Y = torch.empty((m_out, 256), dtype=torch.float32, device=X.device)
    if m_out == 0:
        return Y
    for t, name in ((keep_bits_out, "keep_bits_out"), (mask_bits, "mask_bits")):
        if t is not None and (t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != 8 or not t.is_contiguous()
                              or t.device != X.device):
            raise RuntimeError(f"gemm_xw256: {name} must be a contiguous int32 [rows, 8] device tensor")
    if keep_bits_out is not None and not (relu and keep_bits_out.shape[0] >= m_out
                                          and gemm_keep_bits_usable(X, rows, dropout_p)
                                          and Y.stride(0) < (1 << 21)):
        raise RuntimeError("gemm_xw256: keep_bits_out needs relu, contiguous rows, the bf16x3 scheme and "
                           "dropout_p in {0, 1/2} (gemm_keep_bits_usable)")
    if mask_bits is not None and (mask_src is None or not gemm_keep_bits_usable(X, rows)):
        mask_bits = None                      # (this launch reads the mask itself)
    if x_bound is None and _gemm_scheme == "h2":
        # no bound known: one reduction pass over X (1.4 ms at M = 10^7) and the 5.4 ms kernel
        # still beat the 7.5 ms three-part kernel — and keep full accuracy for tiny operands,
        # where the third bf16 part would fall into the denormals
        x_bound = absmax_now(X)
    ep = None
    if has_fwd_ep or mask_src is not None:
        by_bits = mask_bits is not None
        seed, seed_dev = _seed_fields(seed, X.device, "gemm_xw256")   # (a tensor: hipGraph capture)
        ep = _native.GcnGemmEpilogue(
            bias.detach().data_ptr() if bias is not None else None, int(bool(relu)),
            float(dropout_p), seed, seed_dev,
            mask_src.data_ptr() if (mask_src is not None and not by_bits) else None,
            mask_src.stride(0) if (mask_src is not None and not by_bits) else 0, float(mask_scale),
            mask_rows.data_ptr() if (mask_rows is not None and mask_src is not None) else None,
            int(row_base),
            keep_bits_out.data_ptr() if keep_bits_out is not None else None,
            mask_bits.data_ptr() if by_bits else None)
    # one launch: the scaled scheme's entry point takes the bound of max|X| in front of y_absmax
    h2 = _gemm_scheme == "h2"
    if h2 and (x_bound.dtype != torch.float32 or x_bound.numel() != 1 or x_bound.device != X.device):
        raise RuntimeError("gemm_xw256: x_bound must be one float32 on the operand's device")
    ws_bytes = L.gcn_gemm_xw256_h2_workspace_bytes() if h2 else L.gcn_gemm_xw256_b3_workspace_bytes()
    _native.launch("gcn_gemm_xw256_f32_h2" if h2 else "gcn_gemm_xw256_f32_b3", X.device,
                   X.data_ptr(), X.stride(0), rows.data_ptr() if rows is not None else None,
                   W.data_ptr(), W.stride(0), Y.data_ptr(), Y.stride(0), m_out,
                   *((x_bound.data_ptr(),) if h2 else ()),
                   y_absmax.data_ptr() if y_absmax is not None else None, ep, workspace=ws_bytes)
    if h2 and _bound_check and y_absmax is not None and not bool(torch.isfinite(y_absmax).all()):
        raise RuntimeError("gemm_xw256: non-finite output — x_bound was smaller than max|X| (the "
                           "fp16 parts overflowed) or the operands hold inf / NaN")
    return Y


def gemm_xw256_log_softmax(X, W, bias=None):
    """log_softmax(X[M,256] · W[256,256] + bias, dim=1) in ONE launch of the contiguous-row three-part kernel
    (C-ABI gcn_gemm_xw256_f32_b3_logsoftmax: the finished tile is normalised in registers before it is stored) —
    the end of a last layer evaluated as (Â·h)·W + b.  None where the kernel does not apply (another scheme,
    shape, pitch or alignment): the caller then takes another route."""
    if (_gemm_scheme != "bf16x3" or not X.is_cuda or not _mfma_rows(X, torch.float32, 256, 4)
            or X.stride(0) >= (1 << 21) or W.dtype != torch.float32 or tuple(W.shape) != (256, 256)
            or W.stride(1) != 1 or W.device != X.device):
        return None
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != 256 or not bias.is_contiguous()
                             or bias.data_ptr() % 16 or bias.device != X.device):
        return None
    Y = torch.empty((X.shape[0], 256), dtype=torch.float32, device=X.device)
    if X.shape[0] == 0:
        return Y
    _native.launch("gcn_gemm_xw256_f32_b3_logsoftmax", X.device, X.data_ptr(), X.stride(0), W.data_ptr(),
                   W.stride(0), bias.detach().data_ptr() if bias is not None else None, Y.data_ptr(), Y.stride(0),
                   X.shape[0], workspace=_native.lib().gcn_gemm_xw256_b3_workspace_bytes())
    return Y


def gemm_bf16(X, W, bias=None, relu=False, dropout_p=0.0, seed=0, row_base=0, mask_src=None,
              mask_rows=None, mask_scale=1.0):
    """X[M,K] · W[K,N] for bf16 storage through the streaming MFMA kernel (C-ABI gcn_gemm_xw_bf16;
    (K, N) in {(128,128), (128,256), (256,128)} — config C5's layers are 128 -> 128).
    `bias` / `relu` / `dropout_p` / `seed`: the layer's FORWARD epilogue on the fp32 accumulators
    before the rounding to bf16 (same Philox keep function as the SpMM epilogue) — for a layer
    evaluated as (Â·X)·W + b.  `mask_src` (bf16 [*, N], read at row mask_rows[r] — an int32 device
    list — or r for output row r): the store becomes mask_src > 0 ? y * mask_scale : 0, the backward
    of a fused ReLU / dropout epilogue in the grad_input GEMM's own store (excludes the forward
    epilogue).  None if the operands do not fit (the caller then uses torch.mm)."""
    if (not X.is_cuda or not _mfma_rows(X, torch.bfloat16, None, 8) or W.dtype != torch.bfloat16
            or W.dim() != 2 or X.shape[1] != W.shape[0] or X.shape[0] == 0 or W.stride(1) != 1):
        return None
    L = _native.lib()
    K, N = W.shape
    ws_bytes = L.gcn_gemm_bf16_workspace_bytes(K, N)
    if ws_bytes == 0:
        return None
    ep = bias32 = None
    if mask_src is not None:
        if (bias is not None or relu or dropout_p > 0.0 or not _mfma_rows(mask_src, torch.bfloat16, N, 8)
                or mask_src.device != X.device):
            return None
        if mask_rows is not None and (mask_rows.dtype != torch.int32 or not mask_rows.is_contiguous()
                                      or mask_rows.device != X.device or mask_rows.numel() < X.shape[0]):
            raise RuntimeError("gemm_bf16: mask_rows must be a contiguous int32 device list, one entry per output row")
        ep = _native.GcnGemmEpilogue(None, 0, 0.0, 0, None, mask_src.data_ptr(), mask_src.stride(0),
                                     float(mask_scale), mask_rows.data_ptr() if mask_rows is not None else None, 0)
    elif bias is not None or relu or dropout_p > 0.0:
        if bias is not None:
            if bias.numel() != N or bias.device != X.device:
                return None
            bias32 = bias.detach().to(torch.float32).contiguous()     # (kept alive past the launch)
        seed, seed_dev = _seed_fields(seed, X.device, "gemm_bf16")   # (a tensor: hipGraph capture)
        ep = _native.GcnGemmEpilogue(bias32.data_ptr() if bias32 is not None else None, int(bool(relu)),
                                     float(dropout_p), seed, seed_dev, None, 0, 1.0, None, int(row_base))
    Y = torch.empty((X.shape[0], N), dtype=torch.bfloat16, device=X.device)
    _native.launch("gcn_gemm_xw_bf16", X.device, X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0),
                   Y.data_ptr(), Y.stride(0), X.shape[0], K, N, ep, workspace=ws_bytes)
    return Y


def layer_gemm_reassociable(x, weight, bias):
    """Can `epilogue((A·x)·W + b)` run with the epilogue in a hand-written GEMM's store?  fp32
    256 -> 256 (gcn_gemm_xw256_f32_h2) or bf16 storage at the streaming kernel's shapes with
    Fin <= Fout (the product A·x then is no wider than A·(x·W))."""
    if x.dim() != 2 or not x.is_cuda or x.stride(1) != 1 or weight.dim() != 2 or x.dtype != weight.dtype:
        return False
    if x.dtype == torch.float32:
        return (_gemm_scheme != "exact" and tuple(weight.shape) == (256, 256) and x.shape[1] == 256
                and (bias is None or (bias.dtype == torch.float32 and bias.is_contiguous())))
    if x.dtype == torch.bfloat16:
        return (tuple(weight.shape) in ((128, 128), (128, 256)) and x.shape[1] == weight.shape[0]
                and weight.stride(1) == 1)
    return False


def layer_gemm(z, weight, z_bound=None, y_absmax=None, bias=None, relu=False, dropout_p=0.0, seed=0,
               row_base=0, keep_bits_out=None):
    """epilogue(z·W + b) through the kernel layer_gemm_reassociable() promised (None if it declines)."""
    if z.dtype == torch.float32:
        return gemm_xw256(z, weight, z_bound, y_absmax, bias=bias, relu=relu, dropout_p=dropout_p,
                          seed=seed, row_base=row_base, keep_bits_out=keep_bits_out)
    return gemm_bf16(z, weight, bias=bias, relu=relu, dropout_p=dropout_p, seed=seed, row_base=row_base)


_identity_lists = {}


def padded_row_list(rows):
    """int32 copy of a row-index list, padded to a multiple of 16 entries by repeating its last
    entry (what gcn_gemm_atg256_f32 expects: the 16 indices of a step are one scalar load)."""
    r = rows.to(torch.int32)
    pad = (-r.numel()) % 16
    if pad and r.numel():
        r = torch.cat([r, r[-1:].expand(pad)])
    return r.contiguous()


def _identity_list(n, device):
    """0, 1, …, n-1 (padded) — cached per device, grown on demand."""
    key = _device_key(device)
    have = _identity_lists.get(key)
    need = (n + 15) // 16 * 16
    if have is None or have.numel() < need:
        have = _identity_lists[key] = torch.arange(need, dtype=torch.int32, device=device).clamp_(max=max(n - 1, 0))
        have._n = n
    if getattr(have, "_n", None) != n:       # the clamp of the padding depends on n
        have = torch.arange(need, dtype=torch.int32, device=device).clamp_(max=max(n - 1, 0))
        have._n = n
        _identity_lists[key] = have
    return have


def weight_grad_rows(A, G, rows_a=None, rows_g=None, a_bound=None, g_bound=None, n_list=None, colsum_g=False):
    """Σ_r A[rows_a[r]]ᵀ ⊗ G[rows_g[r]] through the gather-fused MFMA kernels: the weight gradient
    `inputᵀ · grad_support` over a LIST of rows, without compacting either operand first.
    fp32 [*, 256] x [*, 256] (C-ABI gcn_gemm_atg256_f32_b3: three bf16 parts, fp32-equivalent — or
    gcn_gemm_atg256_f32, the scaled two-part fp16 scheme, under set_gemm_scheme("h2")) or bf16
    storage [*, 128] x [*, 128] (C-ABI gcn_gemm_atg_bf16: fp32 accumulation, result rounded once
    to bf16).  rows_*: int32 device index lists or None (= all rows, in order).  A list may be
    longer than `n_list` (padding to a multiple of 16, padded_row_list()); unpadded lists are
    padded here.  *_bound (fp32 only): DEVICE float [1] upper bounds of max|A|, max|G| (computed
    here by a reduction pass over the listed rows when missing).  None if the operands do not fit
    a kernel.
    colsum_g=True (fp32, default scheme): returns (grad_w, Σ_r G[rows_g[r]] as fp32 [256]) — the layer's bias
    gradient from the rows the kernel loads anyway (C-ABI gcn_gemm_atg256_f32_b3_colsum); None where that
    form does not exist (the caller then sums G itself)."""
    bf16 = A.dtype == torch.bfloat16 and G.dtype == torch.bfloat16
    if colsum_g and (bf16 or _gemm_scheme != "bf16x3"):
        return None
    if bf16:
        if (not A.is_cuda or not _mfma_rows(A, torch.bfloat16, None, 2, 4)
                or not _mfma_rows(G, torch.bfloat16, None, 2, 4)
                or _native.lib().gcn_gemm_atg_bf16_workspace_bytes(16, A.shape[1], G.shape[1]) == 0):
            return None
    elif (_gemm_scheme == "exact" or not A.is_cuda or not _mfma_rows(A, torch.float32, 256, 4)
            or not _mfma_rows(G, torch.float32, 256, 4)):
        return None
    if n_list is None:
        n_a = rows_a.numel() if rows_a is not None else A.shape[0]
        n_g = rows_g.numel() if rows_g is not None else G.shape[0]
        if n_a != n_g:
            raise RuntimeError("weight_grad_rows: the two operands list different numbers of rows")
        n_list = n_a
    if n_list == 0:
        zero = torch.zeros((A.shape[1], G.shape[1]), dtype=A.dtype, device=A.device)
        return (zero, torch.zeros(G.shape[1], dtype=torch.float32, device=A.device)) if colsum_g else zero
    lists = []
    for r, t in ((rows_a, A), (rows_g, G)):
        if r is None:
            if t.shape[0] < n_list:
                raise RuntimeError("weight_grad_rows: operand has fewer rows than n_list")
            r = _identity_list(n_list, A.device)
        elif r.dtype != torch.int32 or not r.is_contiguous() or r.device != A.device:
            raise RuntimeError("weight_grad_rows: row lists must be contiguous int32 device tensors")
        elif r.numel() < (n_list + 15) // 16 * 16:
            r = padded_row_list(r[:n_list])
        lists.append(r)
    L = _native.lib()
    if bf16:
        K, N = A.shape[1], G.shape[1]
        out = torch.empty((K, N), dtype=torch.float32, device=A.device)
        _native.launch("gcn_gemm_atg_bf16", A.device, A.data_ptr(), A.stride(0), lists[0].data_ptr(),
                       G.data_ptr(), G.stride(0), lists[1].data_ptr(), n_list, K, N, out.data_ptr(), out.stride(0),
                       workspace=L.gcn_gemm_atg_bf16_workspace_bytes(n_list, K, N))
        return out.to(torch.bfloat16)
    # one launch: the three entry points differ by what stands in front of the output (the scaled
    # scheme's two bounds) and behind it (the column sums)
    out = torch.empty((256, 256), dtype=torch.float32, device=A.device)
    name, bounds, sums = "gcn_gemm_atg256_f32_b3", (), ()       # three bf16 parts: no bounds
    if colsum_g:
        cs = torch.empty(256, dtype=torch.float32, device=A.device)
        name, sums = "gcn_gemm_atg256_f32_b3_colsum", (cs.data_ptr(),)
    elif _gemm_scheme == "h2":
        # (no bound supplied: a reduction pass — over the LISTED rows only, the others may hold anything)
        if a_bound is None:
            src = A.detach()[:n_list] if rows_a is None else A.detach().index_select(0, rows_a[:n_list].long())
            a_bound = absmax_now(src)
        if g_bound is None:
            src = G.detach()[:n_list] if rows_g is None else G.detach().index_select(0, rows_g[:n_list].long())
            g_bound = absmax_now(src)
        name, bounds = "gcn_gemm_atg256_f32", (a_bound.data_ptr(), g_bound.data_ptr())
    _native.launch(name, A.device, A.data_ptr(), A.stride(0), lists[0].data_ptr(), G.data_ptr(), G.stride(0),
                   lists[1].data_ptr(), n_list, *bounds, out.data_ptr(), out.stride(0), *sums,
                   workspace=L.gcn_gemm_atg256_workspace_bytes(n_list))
    return (out, cs) if colsum_g else out




_absmax = {}        # (kind of entry, device key) -> the last four (weak reference, version, DEVICE float [1])


def _absmax_get(kind, t):
    for ref, version, val in _absmax.get((kind, _device_key(t.device)), ()):
        if ref() is t and version == t._version:
            return val
    return None


def _absmax_put(kind, t, val):
    key = (kind, _device_key(t.device))
    live = [e for e in _absmax.get(key, ()) if e[0]() is not None]
    _absmax[key] = live[-3:] + [(weakref.ref(t), t._version, val)]


def _absmax_staged(t):
    """max|t| as a DEVICE float [1] — the value of torch.linalg.vector_norm(t, inf), a maximum being exact in any
    order — by reductions of at most a row each: per row of t, then over groups of 128 until one group is left.
    For a launch recorded in a hipGraph: torch's one-output reduction of a large tensor splits the output over
    blocks that meet through a zeroed counter, and replayed from a graph that begins with it, after any kernel on
    the launching stream, it left its result unwritten (profiles/capture_coverage.md, finding 4); a reduction whose
    every output belongs to one block has no such counter."""
    v = t.detach()
    if v.dim() >= 2 and v.shape[-1] <= 4096:
        v = torch.linalg.vector_norm(v.reshape(-1, v.shape[-1]), ord=float("inf"), dim=1)
    else:
        v = v.reshape(-1).abs()
    while v.numel() > 128:
        pad = (-v.numel()) % 128
        if pad:
            v = torch.nn.functional.pad(v, (0, pad))
        v = v.view(-1, 128).amax(dim=1)
    return v.amax().float().reshape(1)


def absmax_now(t):
    """max|t| as a DEVICE float [1] by one reduction pass, for every bound formed where none is known: torch's
    vector_norm, and _absmax_staged (the same bits) while the stream is being captured into a hipGraph."""
    if t.is_cuda and torch.cuda.is_current_stream_capturing():
        return _absmax_staged(t)
    return torch.linalg.vector_norm(t.detach(), ord=float("inf")).reshape(1)


def absmax_cached(t):
    """max|t| as a DEVICE float tensor [1], computed once per (tensor object, version): for operands
    that stay constant across steps (the feature matrix).  A few entries per device (an eval-mode
    forward pass sees every layer's input as "constant": they must not evict each other), each
    holding a weak reference to the tensor OBJECT — a new tensor that happens to reuse the storage
    address of a freed one can never inherit its bound (a bound that is too small would overflow
    the fp16 parts).  While the stream is being captured into a hipGraph the cache is neither consulted
    nor filled: a replay follows in-place refills of t, which a bound computed before the capture would
    not, so the reduction is recorded in the graph."""
    if t.is_cuda and torch.cuda.is_current_stream_capturing():
        return _absmax_staged(t)
    val = _absmax_get("computed", t)
    if val is None:
        val = torch.linalg.vector_norm(t.detach(), ord=float("inf")).float().reshape(1)
        _absmax_put("computed", t, val)
    return val


def remember_absmax(t, value):
    """Record max|t| (a DEVICE float [1] a kernel produced as a side result, e.g. the GEMM's
    y_absmax) for the tensor OBJECT t at its current version, so that the next layer's GEMM needs
    no reduction pass over t.  A few entries per device; weak references, like absmax_cached
    (whose entries these never evict, nor the other way round)."""
    _absmax_put("recorded", t, value)


def known_absmax(t):
    """The bound remember_absmax() recorded for this tensor object and version, or None."""
    return _absmax_get("recorded", t)


def _dense_forward(input, weight, x_bound=None, y_absmax=None):
    out = gemm_xw256(input, weight, x_bound, y_absmax)
    if out is None and y_absmax is None:
        out = gemm_bf16(input, weight)
    if out is None:
        out = torch.mm(input, weight)
        if y_absmax is not None:
            y_absmax.copy_(out.detach().abs().max())
    return out


def _weight_grad(input, grad, a_bound=None, g_bound=None):
    """inputᵀ · grad: the hand-written MFMA kernel for 256-wide fp32 layers — always under the
    three-part bf16 scheme; under "h2" when the caller knows bounds of both operands' maxima (the
    scaling needs them; two reduction passes over [N, 256] tensors would cost what the kernel saves)
    — otherwise hipBLASLt with the reduction over the graph's vertices cut into K_SPLIT slabs."""
    if (_gemm_scheme == "bf16x3" and input.dtype == torch.float32) or \
            (a_bound is not None and g_bound is not None and _gemm_scheme == "h2") or \
            (input.dtype == torch.bfloat16 and grad.dtype == torch.bfloat16 and input.is_cuda):
        out = weight_grad_rows(input, grad, a_bound=a_bound, g_bound=g_bound)
        if out is not None:
            return out
    n, b = input.shape[0], K_SPLIT
    if n >= MIN_ROWS and input.is_contiguous() and grad.is_contiguous():
        m = n // b * b
        grad_w = torch.bmm(input[:m].view(b, m // b, -1).transpose(1, 2),
                           grad[:m].view(b, m // b, -1)).sum(0)
        if m < n:
            grad_w = grad_w + torch.mm(input[m:].t(), grad[m:])
        return grad_w
    return torch.mm(input.t(), grad)


def _dense_grads(input, weight, grad, need_in, need_w, rows=None):
    """(grad_input, grad_weight) of `input @ weight`.  `rows` (int64 indices, sorted) names the
    only rows of `grad` that are non-zero: both GEMMs then run on those rows alone — zero rows
    add nothing to inputᵀ·grad and give zero rows of grad·weightᵀ."""
    grad_in = grad_w = None
    if rows is not None:
        grad = grad.index_select(0, rows)
        if need_w:
            grad_w = _weight_grad(input.index_select(0, rows), grad)
        if need_in:
            part = gemm_xw256(grad, weight.t().contiguous())
            if part is None:
                part = gemm_bf16(grad, weight.t().contiguous())
            if part is None:
                part = torch.mm(grad, weight.t())
            grad_in = torch.zeros((input.shape[0], weight.shape[0]), dtype=part.dtype,
                                  device=part.device)
            grad_in.index_copy_(0, rows, part)
        return grad_in, grad_w
    if need_in:
        y_max = torch.zeros(1, dtype=torch.float32, device=grad.device) \
            if (grad.is_cuda and grad.dtype == torch.float32) else None
        grad_in = gemm_xw256(grad, weight.t().contiguous(), None, y_max)
        if grad_in is not None and y_max is not None and _gemm_scheme != "exact":
            remember_absmax(grad_in, y_max)      # (the layer below bounds its masked gradient by it)
        if grad_in is None:
            grad_in = gemm_bf16(grad, weight.t().contiguous())
        if grad_in is None:
            grad_in = torch.mm(grad, weight.t())
    if need_w:
        grad_w = _weight_grad(input, grad)
    return grad_in, grad_w


class DenseMMFunction(torch.autograd.Function):
    """`torch.mm(input, weight)` (reference pygcn/layers.py:33) with a K-split weight gradient.

    grad_W = inputᵀ · grad is a [Fin, N]·[N, Fout] GEMM whose reduction runs over the N graph
    vertices (10⁷ at config C4).  hipBLASLt answers that shape with a stream-K kernel at 21.5 ms;
    cutting N into 128 slabs, one batched GEMM over the slabs and a sum of the 128 small partial
    products takes 8.7 ms on MI355X (tools/gemm_probe.py) and is at least as accurate (shorter
    fp32 accumulation chains).

    Forward and grad_input use the hand-written MFMA kernels when the layer is 256 -> 256 fp32
    (gemm_xw256: 5.2 ms vs hipBLASLt 9.95 ms at N = 10⁷) or one of the bf16 shapes of gemm_bf16,
    torch.mm otherwise.  (The one-node training path, pygcn_amd/fused.py, forms the weight
    gradient with the gather-fused kernel weight_grad_rows instead.)"""

    K_SPLIT = K_SPLIT
    MIN_ROWS = MIN_ROWS

    @staticmethod
    def forward(ctx, input, weight):
        ctx.save_for_backward(input, weight)
        bound = known_absmax(input) if (input.is_cuda and input.dtype == torch.float32) else None
        return _dense_forward(input, weight, bound)

    @staticmethod
    def backward(ctx, grad):
        input, weight = ctx.saved_tensors
        return _dense_grads(input, weight, grad, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
