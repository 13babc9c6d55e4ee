"""Seeded synthetic inputs shared by the golden-vector generator and the tests.

Everything here is plain numpy with explicit seeds so that the generator
(`make_golden.py`, run once in the build container where /root/reference is
mounted) and the tests (run anywhere, including the GPU box where the reference
does not exist) see bit-identical inputs.  Nothing here imports the reference,
the oracle or the product.
"""
import numpy as np

CORA_N = 2708
CORA_NFEAT = 1433
CORA_NCLASS = 7
CORA_NHID = 16


def cora_features(seed=42, n=CORA_N, nfeat=CORA_NFEAT, p=0.0127):
    """Synthetic stand-in for cora.content (absent from the reference tree):
    Bernoulli(p) bag-of-words rows, row-normalized the way utils.normalize does
    (reference pygcn/utils.py:390-397; empty rows -> 0)."""
    rng = np.random.default_rng(seed)
    x = (rng.random((n, nfeat)) < p).astype(np.float32)
    rowsum = x.sum(1, dtype=np.float64)
    with np.errstate(divide="ignore"):
        rinv = np.where(rowsum > 0, 1.0 / rowsum, 0.0)
    return (x * rinv[:, None]).astype(np.float32)


def cora_labels(seed=42, n=CORA_N, nclass=CORA_NCLASS):
    rng = np.random.default_rng(seed + 1)
    return rng.integers(0, nclass, size=n).astype(np.int64)


def cora_splits():
    # reference pygcn/utils.py:370-372
    return np.arange(140), np.arange(200, 500), np.arange(500, 1500)


def random_coo(n_rows, n_cols, nnz, seed, empty_rows=(), hub_row=None, hub_deg=0,
               duplicates=0):
    """Random COO (unsorted, possibly with duplicates) with fp32 values in (0,1]."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_rows, size=nnz)
    cols = rng.integers(0, n_cols, size=nnz)
    if hub_row is not None:
        rows = np.concatenate([rows, np.full(hub_deg, hub_row)])
        cols = np.concatenate([cols, rng.integers(0, n_cols, size=hub_deg)])
    if duplicates:
        pick = rng.integers(0, len(rows), size=duplicates)
        rows = np.concatenate([rows, rows[pick]])
        cols = np.concatenate([cols, cols[pick]])
    if len(empty_rows):
        keep = ~np.isin(rows, np.asarray(empty_rows))
        rows, cols = rows[keep], cols[keep]
    vals = (1.0 - rng.random(len(rows))).astype(np.float32)
    perm = rng.permutation(len(rows))
    return rows[perm].astype(np.int64), cols[perm].astype(np.int64), vals[perm]


def dense(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


# the rows of a matrix on which `normalize` (reference pygcn/utils.py:390-397) does not simply
# divide: name -> stored float32 values.  Expected: zeros for the first four (the reciprocal of
# the float32 row sum is infinite, or the sum itself is), NaN for the last.
NORMALIZE_SPECIAL_ROWS = {
    "cancels": [1.0, -1.0, 2.0, -2.0],          # small integers: 0 in every summation order
    "stored_zeros": [0.0, 0.0, 0.0],
    "subnormal_sum": [1e-40, 2e-40],            # 1 / 3e-40 overflows float32
    "overflowing_sum": [3e38, 3e38],            # the sum is +inf, its reciprocal 0
    "nan": [0.5, float("nan"), 0.25],
}


def normalize_matrix(lengths, n_cols, seed, special=None, max_condition=50.0):
    """CSR (rowptr int64, col int32, val float32) with the given row lengths for row-normalisation
    checks.  Ordinary rows: magnitudes in (0, 1], the sign of about one entry in ten flipped; a row
    whose sum would be ill-conditioned (Σ|v| / |Σv| > max_condition) gets all its signs cleared, so
    every ordinary row has a condition number <= max_condition.  `special`: {row: name in
    NORMALIZE_SPECIAL_ROWS}; those rows hold exactly the listed values.  Columns: a run of
    consecutive indices per row at a random offset (sorted, distinct)."""
    rng = np.random.default_rng(seed)
    lengths = np.array(lengths, np.int64)
    special = dict(special or {})
    for r, name in special.items():
        lengths[r] = len(NORMALIZE_SPECIAL_ROWS[name])
    assert lengths.max() <= n_cols
    rowptr = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(lengths, out=rowptr[1:])
    nnz = int(rowptr[-1])
    val = 1.0 - rng.random(nnz)
    val[rng.random(nnz) < 0.1] *= -1.0
    val = val.astype(np.float32)
    full = np.flatnonzero(lengths > 0)
    s = np.add.reduceat(val.astype(np.float64), rowptr[full])
    a = np.add.reduceat(np.abs(val.astype(np.float64)), rowptr[full])
    for r in full[a > max_condition * np.abs(s)]:
        val[rowptr[r]:rowptr[r + 1]] = np.abs(val[rowptr[r]:rowptr[r + 1]])
    for r, name in special.items():
        val[rowptr[r]:rowptr[r + 1]] = np.asarray(NORMALIZE_SPECIAL_ROWS[name], np.float32)
    offset = np.floor(rng.random(lengths.size) * (n_cols - lengths + 1)).astype(np.int64)
    col = np.repeat(offset, lengths) + (np.arange(nnz) - np.repeat(rowptr[:-1], lengths))
    return rowptr, col.astype(np.int32), val


G6_SPECIAL = {3: "cancels", 40: "stored_zeros", 77: "subnormal_sum", 500: "overflowing_sum",
              1200: "nan", 1999: "subnormal_sum"}
G6_LONG_ROW = 900


def g6_normalize_input():
    """The 2000 x 2000 float32 matrix of fixture g6_normalize.npz: ~16 000 entries, the special
    rows above (the last row among them), empty rows and one row of 300 entries."""
    n = 2000
    lengths = np.random.default_rng(600).poisson(8, n)
    lengths[[0, 41, 1998]] = 0
    lengths[G6_LONG_ROW] = 300
    rowptr, col, val = normalize_matrix(lengths, n, seed=601, special=G6_SPECIAL)
    return rowptr, col, val, (n, n)
