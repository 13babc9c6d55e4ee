"""Numpy restatement of the dense adjacency ingest (include/gcn_spmm.h, "Dense adjacency ingest";
CSRGraph.from_dense): what tests/test_dense_ingest_cpu.py pins and tests/test_dense_ingest_gpu.py holds the HIP
sweeps against, exactly.  The selection order, the k-th largest and the index rule are those of tests/_select_ref.py.
Nothing here imports the native library.

  kept_mask(A, rule, bound, keep)      bool [n_rows, n_cols]: the entries the conversion keeps
  dense_to_csr(A, rule, bound, keep)   (rowptr int64, col int32, val float32) in np.nonzero's (row-major) order
  symmetrized(rowptr, col, val, n)     the union with the transpose, a mirrored pair keeping the larger value
  dense_of(rowptr, col, val, shape)    the float32 matrix of a CSR triple
  row_normalized64(A)                  float64 D^-1 A, an empty row staying 0
  edge_matrix / special_rows / tall_matrix / covisit_matrix     the fixtures of the tests
"""
import numpy as np

import _select_ref as S

NONZERO, GREATER = 0, 1          # GCN_DENSE_NONZERO, GCN_DENSE_GREATER


def kept_mask(A, rule=NONZERO, bound=0.0, keep=None):
    A = np.ascontiguousarray(A, dtype=np.float32)
    assert A.ndim == 2 and rule in (NONZERO, GREATER)
    with np.errstate(invalid="ignore"):
        ok = ~(A == 0) if rule == NONZERO else A > np.float32(bound)       # (NaN == 0 is False: kept; NaN > t: dropped)
    if keep is not None and keep < A.shape[1] and A.shape[0]:
        assert keep >= 1
        chosen = np.zeros(A.shape, dtype=bool)
        np.put_along_axis(chosen, S.topk_indices(A, keep), True, axis=1)
        ok &= chosen
    return ok


def dense_to_csr(A, rule=NONZERO, bound=0.0, keep=None):
    A = np.ascontiguousarray(A, dtype=np.float32)
    ok = kept_mask(A, rule, bound, keep)
    rowptr = np.zeros(A.shape[0] + 1, np.int64)
    rowptr[1:] = np.cumsum(ok.sum(1))
    return rowptr, np.nonzero(ok)[1].astype(np.int32), A[ok]


def rows_of(rowptr):
    return np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))


def symmetrized(rowptr, col, val, n):
    """The entries (i, j) with (i, j) or (j, i) stored, each holding the larger of the stored values."""
    row = rows_of(rowptr)
    r = np.concatenate([row, col.astype(np.int64)])
    c = np.concatenate([col.astype(np.int64), row])
    v = np.concatenate([val, val])
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    first = np.ones(r.size, dtype=bool)
    first[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    start = np.flatnonzero(first)
    out_v = np.maximum.reduceat(v, start) if r.size else v
    out_rowptr = np.zeros(n + 1, np.int64)
    out_rowptr[1:] = np.cumsum(np.bincount(r[first], minlength=n))
    return out_rowptr, c[first].astype(np.int32), out_v.astype(np.float32)


def dense_of(rowptr, col, val, shape):
    out = np.zeros(shape, np.float32)
    out[rows_of(rowptr), col] = val
    return out


def row_normalized64(A):
    A = np.asarray(A, np.float64)
    d = A.sum(1, keepdims=True)
    return np.divide(A, d, out=np.zeros_like(A), where=d != 0)


# ------------------------------------------------------------------------------------------------ fixtures
LEVELS = np.arange(1, 9, dtype=np.float32) / 8           # eight values: ties at every threshold


def edge_matrix(n_cols, seed, n_rows=7):
    """Density about 1/2, values of LEVELS with one in ten negative; row 2 is empty and row 4 full."""
    rng = np.random.default_rng(seed)
    A = rng.choice(LEVELS, size=(n_rows, n_cols)).astype(np.float32)
    A *= np.where(rng.random((n_rows, n_cols)) < 0.1, -1, 1).astype(np.float32)
    A[rng.random((n_rows, n_cols)) < 0.5] = 0
    A[2] = 0
    A[4] = np.where(A[4] == 0, np.float32(0.5), A[4])
    return A


NAN_A, NAN_B = 0x7FC00001, 0xFFA5A5A5                  # two NaN payloads, the second with its sign bit set


def special_rows():
    """[4, 16]: -0, +0, two NaNs, both infinities, subnormals, negatives and ties; a row of equal entries; a row of
    zeros of both signs; a row of NaNs only."""
    bits = np.array([0x80000000, 0x00000000, NAN_A, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF,
                     0x3F800000, 0xBF800000, NAN_B, 0x3F800000, 0x80000000, 0x40000000, 0x3F800000, 0xC0000000],
                    dtype=np.uint32)
    A = np.empty((4, 16), np.float32)
    A[0] = bits.view(np.float32)
    A[1] = 0.75
    A[2] = np.where(np.arange(16) % 2 == 0, np.float32(-0.0), np.float32(0.0))
    A[3] = np.array([NAN_A, NAN_B] * 8, dtype=np.uint32).view(np.float32)
    return A


def tall_matrix(n_rows, seed, n_cols=8):
    rng = np.random.default_rng(seed)
    A = rng.choice(LEVELS[:4], size=(n_rows, n_cols)).astype(np.float32)
    A[rng.random((n_rows, n_cols)) < 0.4] = 0
    A[-1] = LEVELS[:n_cols][::-1]                      # the last row: full and strictly decreasing
    A[-2] = 0
    return A


def covisit_matrix(n=300, visits=40, density=0.08, seed=7):
    """A = BᵀB for a 0/1 visit matrix B [visits, n]: symmetric, small non-negative integers, its own diagonal."""
    rng = np.random.default_rng(seed)
    B = (rng.random((visits, n)) < density).astype(np.float32)
    return (B.T @ B).astype(np.float32)
