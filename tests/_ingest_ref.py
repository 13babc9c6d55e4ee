"""Plain host references for the device ingest kernels (pygcn_amd/csrc/gcn_ingest.hip), numpy and
scipy only: the arbiter of tests/test_ingest_scale_gpu.py, itself pinned by
tests/test_ingest_ref_cpu.py.  Nothing here imports pygcn_amd.graph, the native library or the
oracle; `pygcn_amd/utils.py` (the project's copy of the reference's `normalize`, pure scipy) is
loaded as a stand-alone file so that the package and its kernels stay out of the reference.

  coo_reduce_reference(rows, cols, vals, n_rows, n_cols, reduce)   COO -> CSR, duplicates reduced
                                                                  sequentially in storage order, fp32
  adjacency_recipe_reference(edges, n, ...)                        the reference's adjacency recipe
  transpose_reference(rowptr, col, val, n_cols)                    CSR(A) -> CSR(A^T), stable
  row_normalize_bound(vals_of_row) / row_normalize_bounds(...)     derived tolerance of D^-1 · A
"""
import importlib.util
import os

import numpy as np
import scipy.sparse as sp

_UTILS = None


def product_utils():
    """pygcn_amd/utils.py as a stand-alone module (it imports numpy, scipy and torch only)."""
    global _UTILS
    if _UTILS is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "pygcn_amd", "utils.py")
        spec = importlib.util.spec_from_file_location("_ingest_ref_product_utils", path)
        _UTILS = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_UTILS)
    return _UTILS


def coo_reduce_reference(rows, cols, vals, n_rows, n_cols, reduce="sum"):
    """(rowptr int64, col int32, val float32) of the COO triplets: stable sort by
    row * n_cols + col, then every run of equal keys reduced SEQUENTIALLY, in storage order, in
    float32 — ((v0 + v1) + v2) + ... for "sum", fmax(fmax(v0, v1), v2) ... for "max" (fmax: a NaN
    member is ignored unless the whole run is NaN, the behaviour gcn_coo_to_csr_device documents).
    No Python loop per run: pass k folds the k-th member into every run still longer than k, so
    the passes are as many as the longest run and their index sets shrink."""
    if reduce not in ("sum", "max"):
        raise ValueError(reduce)
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    vals = np.asarray(vals, np.float32)
    key = rows * np.int64(n_cols) + cols
    order = np.argsort(key, kind="stable")
    ks, vs = key[order], vals[order]
    if ks.size == 0:
        return np.zeros(n_rows + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
    head = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    length = np.diff(np.concatenate([head, [ks.size]]))
    acc = vs[head].copy()
    live = np.flatnonzero(length > 1)
    k = 1
    with np.errstate(invalid="ignore", over="ignore"):
        while live.size:
            nxt = vs[head[live] + k]
            acc[live] = (acc[live] + nxt) if reduce == "sum" else np.fmax(acc[live], nxt)
            k += 1
            live = live[length[live] > k]
    assert acc.dtype == np.float32
    uk = ks[head]
    rowptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(uk // n_cols, minlength=n_rows), out=rowptr[1:])
    return rowptr, (uk % n_cols).astype(np.int32), acc


def adjacency_recipe_reference(edges, n, symmetrize=True, self_loops=True, normalize=True):
    """The reference's adjacency recipe (pygcn/utils.py:360-368) with scipy, in float64:
    COO of ones with duplicates summed, max(adj, adj.T) (what the three-term symmetrization
    formula amounts to), + I, D^-1 · adj by the project's copy of `normalize`.
    Returns (rowptr int64, col int32, val float64), columns sorted inside every row."""
    edges = np.asarray(edges, np.int64)
    adj = sp.coo_matrix((np.ones(edges.shape[0], np.float64), (edges[:, 0], edges[:, 1])),
                        shape=(n, n)).tocsr()
    adj.sum_duplicates()
    if symmetrize:
        adj = adj.maximum(adj.T)
    if self_loops:
        adj = adj + sp.eye(n, dtype=np.float64, format="csr")
    adj = sp.csr_matrix(adj)
    if normalize:
        adj = sp.csr_matrix(product_utils().normalize(adj))
    adj.sum_duplicates()
    adj.sort_indices()
    return adj.indptr.astype(np.int64), adj.indices.astype(np.int32), adj.data.astype(np.float64)


def transpose_reference(rowptr, col, val, n_cols):
    """CSR(A) -> CSR(A^T) by a stable sort of the stored entries by column: inside every row of
    A^T the entries keep their storage order, i.e. increasing source row (and, for duplicate
    columns inside one source row, the order they were stored in).  Values are moved, not
    touched; rowptr comes back as int64, col as int32, val with the dtype it came in."""
    rowptr, col, val = np.asarray(rowptr, np.int64), np.asarray(col), np.asarray(val)
    src = np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))
    order = np.argsort(col, kind="stable")
    rowptr_t = np.zeros(n_cols + 1, np.int64)
    np.cumsum(np.bincount(col, minlength=n_cols), out=rowptr_t[1:])
    return rowptr_t, src[order].astype(np.int32), val[order]


U32 = 2.0 ** -24          # unit roundoff of float32


def row_normalize_bound(vals_of_row):
    """Relative tolerance of one row of D^-1 · A computed the way gcn_row_normalize_device does:
    |got - ref| <= bound * |ref| with bound = (ceil(L/64) + 8) · 2^-24 · (Σ|v| / |Σv|).
    64 lanes each sum ceil(L/64) entries of the row, six butterfly steps join them (the float32
    sum: at most ceil(L/64) + 6 roundings on the path of any entry, each relative to a partial sum
    bounded by Σ|v|, hence the condition number Σ|v|/|Σv| of the sum), then one reciprocal and one
    product.  inf for a row whose float64 sum is 0 (no relative bound exists)."""
    v = np.asarray(vals_of_row, np.float64)
    s = abs(v.sum())
    if s == 0:
        return np.inf
    return (-(-v.size // 64) + 8) * U32 * (np.abs(v).sum() / s)


def row_normalize_bounds(rowptr, val):
    """row_normalize_bound for every row of a CSR matrix at once (float64 sums by reduceat);
    returns (bound per row, Σv per row in float64).  Empty rows: bound inf, sum 0."""
    rowptr = np.asarray(rowptr, np.int64)
    v = np.asarray(val, np.float64)
    length = np.diff(rowptr)
    s, a = np.zeros(length.size), np.zeros(length.size)
    full = np.flatnonzero(length > 0)
    if full.size:
        # (reduceat over the starts of the non-empty rows only: consecutive starts then delimit
        #  exactly one row each, the last one running to the end of the array)
        s[full] = np.add.reduceat(v, rowptr[full])
        a[full] = np.add.reduceat(np.abs(v), rowptr[full])
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = np.where(s != 0, (-(-length // 64) + 8) * U32 * (a / np.abs(s)), np.inf)
    return bound, s
