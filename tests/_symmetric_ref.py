"""Plain numpy float64 restatements of what pygcn_amd/csrc/gcn_symmetric.hip computes (no pygcn_amd code):

  sym_normalize_ref(rowptr, col, val)   w / sqrt(d_i · d_j) for every stored entry (i, j), d = the float64 row sums;
                                        a product of 0 gives 0, NaN and negative products give NaN
  mirror_ref(rowptr, col, val)          for every stored entry (i, j) the storage position of (j, i) — the lower bound
                                        of i among the columns of row j, if that position holds i — or -1, and the
                                        four counts of `gcn_csr_mirror_device`
  within_one_ulp(got, ref64)            |got - fl32(ref64)| <= 2^-23 · |fl32(ref64)|, NaN where the reference is NaN

The lower bound is written out (not np.searchsorted) because on a row whose columns are NOT sorted its answer is
whatever this probe sequence finds, and the device counts are compared with these on such a row too.
"""
import numpy as np


def row_ids(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))


def sym_normalize_ref(rowptr, col, val):
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    w = np.asarray(val, np.float64)
    row = row_ids(rowptr)
    d = np.bincount(row, weights=w, minlength=rowptr.size - 1)
    prod = d[row] * d[col]
    with np.errstate(all="ignore"):
        out = w / np.sqrt(prod)
    out[prod == 0] = 0.0
    return out


def within_one_ulp(got, ref64):
    """Boolean per entry: `got` (float32) is within one float32 ulp (relative 2^-23) of the float64 reference
    rounded to float32; where the reference is NaN, `got` must be NaN."""
    got = np.asarray(got)
    assert got.dtype == np.float32
    with np.errstate(all="ignore"):
        ref32 = np.asarray(ref64, np.float64).astype(np.float32).astype(np.float64)
    g = got.astype(np.float64)
    nan = np.isnan(ref32)
    with np.errstate(invalid="ignore"):
        ok = np.abs(g - ref32) <= 2.0 ** -23 * np.abs(ref32)
    ok[nan] = np.isnan(g[nan])
    inf = np.isinf(ref32)
    ok[inf] = g[inf] == ref32[inf]
    return ok


def mirror_ref(rowptr, col, val):
    """-> (mirror int64 [nnz], (no_mirror, mirror_of_mirror_differs, not_increasing, value_differs))."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    bits = np.ascontiguousarray(np.asarray(val, np.float32)).view(np.int32)
    n, nnz = rowptr.size - 1, col.size
    row = row_ids(rowptr)
    inside = (col >= 0) & (col < n)
    j = np.where(inside, col, 0)
    lo, end = rowptr[j].copy(), rowptr[j + 1]
    hi = end.copy()
    while True:
        live = lo < hi
        if not live.any():
            break
        mid = (lo + hi) >> 1
        less = np.zeros(nnz, bool)
        less[live] = col[mid[live]] < row[live]
        lo = np.where(live & less, mid + 1, lo)
        hi = np.where(live & ~less, mid, hi)
    hit = inside & (lo < end)
    hit[hit] = col[lo[hit]] == row[hit]
    mirror = np.where(hit, lo, -1)
    has = mirror >= 0
    twice = int((mirror[mirror[has]] != np.flatnonzero(has)).sum())
    differs = int((bits[mirror[has]] != bits[has]).sum())
    e = np.arange(nnz)
    not_first = e > rowptr[row]
    unsorted = int((col[e[not_first] - 1] >= col[not_first]).sum())
    return mirror, (int((~has).sum()), twice, unsorted, differs)
