"""Float64 reference products for the full-size tests, in plain torch ops (no pygcn_amd kernel, no
hipSPARSE): the arbiter at heights where the CPU oracle cannot run the whole problem.

  spmm64(rowptr, col, val, B)              Â·B
  spmm64_t(rowptr, col, val, G, n_cols)    Âᵀ·G, from the ORIGINAL arrays with row and column swapped
                                           (not from a transposed graph the project built)
  mm64(A, W)                               A·W
  tn64(A, G)                               Aᵀ·G (a weight gradient), optionally over row lists

The sparse products expand the row ids with repeat_interleave and index_add_ the float64 products
of a chunk of edges at a time; the dense ones work in row chunks, so no full-height float64
temporary exists twice."""
import torch

EDGE_CHUNK = 1 << 22          # 2²² edges x 256 features x 8 B: ~8.6 GB gathered per chunk
ROW_CHUNK = 1 << 20


def _row_ids(rowptr):
    n = rowptr.numel() - 1
    lens = (rowptr[1:] - rowptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(n, device=rowptr.device), lens)


def _scatter64(dst_ids, src_ids, val, B, n_out, chunk, skip_chunk):
    out = torch.zeros((n_out, B.shape[1]), dtype=torch.float64, device=B.device)
    nnz = val.numel()
    for k, s in enumerate(range(0, nnz, chunk)):
        if k == skip_chunk:               # (sensitivity demonstrations only: leave one chunk out)
            continue
        e = min(s + chunk, nnz)
        part = B.index_select(0, src_ids[s:e].long()).double()
        part.mul_(val[s:e].double().unsqueeze(1))
        out.index_add_(0, dst_ids[s:e].long(), part)
        del part
    return out


def spmm64(rowptr, col, val, B, chunk=EDGE_CHUNK, skip_chunk=None):
    """Â·B in float64 for CSR (rowptr, col, val); B of any float dtype, [n_cols, F]."""
    return _scatter64(_row_ids(rowptr), col, val, B, rowptr.numel() - 1, chunk, skip_chunk)


def spmm64_t(rowptr, col, val, G, n_cols, chunk=EDGE_CHUNK, skip_chunk=None):
    """Âᵀ·G in float64: the entries (r, c, v) of Â scattered as (c, r, v); G [n_rows, F]."""
    return _scatter64(col, _row_ids(rowptr), val, G, n_cols, chunk, skip_chunk)


def mm64(A, W, chunk=ROW_CHUNK, out=None):
    """A·W in float64, A [M, K] of any float dtype, W [K, N]; `out` (float64 [M, N]) may be given."""
    W64 = W.double()
    if out is None:
        out = torch.empty((A.shape[0], W.shape[1]), dtype=torch.float64, device=A.device)
    for s in range(0, A.shape[0], chunk):
        torch.mm(A[s:s + chunk].double(), W64, out=out[s:s + chunk])
    return out


def tn64(A, G, rows_a=None, rows_g=None, chunk=ROW_CHUNK, absolute=False):
    """Σ_r A[rows_a[r]]ᵀ ⊗ G[rows_g[r]] in float64 (rows_* None: all rows in order).  With
    `absolute=True` also returns Σ_r |A[.]|ᵀ ⊗ |G[.]| — the size of the summands, the yardstick of
    a reduction that may cancel."""
    m = rows_a.numel() if rows_a is not None else A.shape[0]
    if (rows_g.numel() if rows_g is not None else G.shape[0]) != m:
        raise ValueError("tn64: the two operands list different numbers of rows")
    acc = torch.zeros((A.shape[1], G.shape[1]), dtype=torch.float64, device=A.device)
    acc_abs = torch.zeros_like(acc) if absolute else None
    for s in range(0, m, chunk):
        e = min(s + chunk, m)
        a = (A[s:e] if rows_a is None else A.index_select(0, rows_a[s:e].long())).double()
        g = (G[s:e] if rows_g is None else G.index_select(0, rows_g[s:e].long())).double()
        acc.addmm_(a.t(), g)
        if absolute:
            acc_abs.addmm_(a.abs().t(), g.abs())     # (not in place: a float64 operand is a view)
    return (acc, acc_abs) if absolute else acc


def colsum64(G, chunk=ROW_CHUNK):
    """(Σ_r G[r], Σ_r |G[r]|) in float64."""
    s = torch.zeros(G.shape[1], dtype=torch.float64, device=G.device)
    a = torch.zeros_like(s)
    for r in range(0, G.shape[0], chunk):
        g = G[r:r + chunk].double()
        s += g.sum(0)
        a += g.abs().sum(0)
    return s, a
