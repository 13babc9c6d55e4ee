"""Numpy restatement of neighbour sampling (include/gcn_spmm.h, "Neighbour sampling"): the random word of an entry,
the three keys, the selection with its tie rule, the diagonal and the rescale — what tests/test_neighbor_sampling_cpu.py
pins and tests/test_neighbor_sampling_gpu.py holds `gcn_csr_sample_rows` against, bit for bit.  The generator and the
selection order are those of tests/_select_ref.py.  Nothing here imports the native library.

  random_words(e, seed, stream)    uint32 [len(e)]: w(e) = Philox((e >> 2, stream, 2), seed)[e & 3]
  entry_keys(val, by, seed, stream)  uint32 [nnz]: the key of every stored entry
  sample_neighbors(rowptr, col, val, n_cols, fanout, ...)   (rowptr_out int64, col_out int32, val_out fp32)
  take_rows(rowptr, col, val, rows)                         the rows `rows`, as CSRGraph.take_rows cuts them

The two double sums of rescale="sum" are taken in stored order (np.cumsum); the device adds the same numbers in
another fixed order, so the two agree bit for bit wherever the sums are exact — which the GPU tests arrange."""
import numpy as np

from _select_ref import order_key, philox4x32_10

MODES = ("uniform", "weight", "strongest")


def random_words(e, seed, stream):
    e = np.asarray(e, dtype=np.int64)
    q = e >> 2
    counter = np.empty((e.size, 4), np.uint64)
    counter[:, 0] = q & 0xFFFFFFFF
    counter[:, 1] = q >> 32
    counter[:, 2] = int(stream)
    counter[:, 3] = 2
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(counter, (seed & 0xFFFFFFFF, seed >> 32))
    return w[np.arange(e.size), e & 3]


def entry_keys(val, by, seed=0, stream=0, first=0):
    """The keys of the entries first .. first + len(val) - 1 of the source arrays."""
    val = np.asarray(val, dtype=np.float32)
    if by == "strongest":
        return order_key(val)
    w = random_words(first + np.arange(val.size, dtype=np.int64), seed, stream)
    if by == "uniform":
        return w
    assert by == "weight", by
    u = (w.astype(np.float64) + 0.5) * 2.0 ** -32
    with np.errstate(divide="ignore", invalid="ignore"):
        return order_key((val.astype(np.float64) / -np.log(u)).astype(np.float32))


def kept_positions(keys, cols, s, K, keep_diagonal):
    """Which of a row's d > K entries stay (ascending positions in the row): the first entry of column s ahead of
    the order when keep_diagonal, then the largest keys, the earlier entry on equal keys."""
    d = keys.size
    forced = np.flatnonzero(cols == s)[:1] if keep_diagonal else np.zeros(0, np.int64)
    cand = np.delete(np.arange(d), forced)
    order = np.argsort(-keys[cand].astype(np.int64), kind="stable")[:K - forced.size]
    return np.sort(np.concatenate([forced, cand[order]]))


def sample_neighbors(rowptr, col, val, n_cols, fanout, by="uniform", seed=0, stream=0, rows=None,
                     keep_diagonal=None, rescale=None):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col, val = np.asarray(col, dtype=np.int32), np.asarray(val, dtype=np.float32)
    n_rows, K = rowptr.size - 1, int(fanout)
    assert K >= 1 and by in MODES and rescale in (None, "sum")
    if keep_diagonal is None:
        keep_diagonal = n_rows == n_cols
    assert not (keep_diagonal and n_rows != n_cols)
    keys = entry_keys(val, by, seed, stream)
    source = np.arange(n_rows) if rows is None else np.asarray(rows, dtype=np.int64)
    cols_out, vals_out, lens = [], [], []
    for s in source.tolist():
        s0, s1 = int(rowptr[s]), int(rowptr[s + 1])
        c, v = col[s0:s1], val[s0:s1]
        if s1 - s0 > K:
            keep = kept_positions(keys[s0:s1], c, s, K, keep_diagonal)
            c, kept = c[keep], v[keep]
            if rescale == "sum":
                S, Sp = np.cumsum(v.astype(np.float64))[-1], np.cumsum(kept.astype(np.float64))[-1]
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    ratio = np.float32(S / Sp)
                if np.isfinite(ratio):
                    kept = kept * ratio                      # (fp32 * fp32, rounded once)
            v = kept
        cols_out.append(c)
        vals_out.append(v.astype(np.float32))
        lens.append(c.size)
    rowptr_out = np.zeros(source.size + 1, np.int64)
    np.cumsum(lens, out=rowptr_out[1:])
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)  # noqa: E731
    return rowptr_out, cat(cols_out, np.int32), cat(vals_out, np.float32)


def take_rows(rowptr, col, val, rows):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    lens = rowptr[rows + 1] - rowptr[rows]
    out = np.zeros(rows.size + 1, np.int64)
    np.cumsum(lens, out=out[1:])
    idx = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows.tolist()]) if rows.size else \
        np.zeros(0, np.int64)
    return out, np.asarray(col)[idx.astype(np.int64)], np.asarray(val)[idx.astype(np.int64)]


def assert_same(got, want, what=""):
    """(rowptr, col, val) bit for bit: values as bit patterns, so NaN payloads and the sign of zero count."""
    for name, g, w in zip(("rowptr", "col", "val"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, expected {w.shape}"
        if name == "val":
            g, w = g.astype(np.float32).view(np.uint32), w.astype(np.float32).view(np.uint32)
        else:
            g, w = g.astype(np.int64), w.astype(np.int64)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {name} differs at {bad.size} places, first at {bad[:5].tolist()}"
