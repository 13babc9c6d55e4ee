"""Device graph ingest (pygcn_amd/csrc/gcn_ingest.hip) past one grid sweep and
at its edge cases, every entry compared with the plain host references of tests/_ingest_ref.py:

  COO -> CSR      6 000 011 unsorted triplets on 2 500 003 x 2 400 001 (three sweeps of the entry
                  loops, two of the row-pointer loop, 43-bit keys), sum and max, bitwise; with
                  32-bit and 64-bit row pointers; through the torch sparse COO entry point
  the recipe      from_edge_list on 10^7 R-MAT pairs (multiplicities up to 127, self-loops) against
                  scipy, with each switch off in turn, and on a hand-written multigraph
  normalisation   200 000 rows (four sweeps), rows of 0 ... 100 000 entries, the rows on which
                  the reference's `normalize` does not simply divide, and fixture g6_normalize.npz
  transpose       entry for entry (order inside every row) on the rectangular matrix and the
                  R-MAT adjacency, and back again
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _ingest_ref as R
import inputs as gin
from conftest import assert_normwise, load_golden

pytestmark = pytest.mark.gpu

SWEEP = 8192 * 256            # entries (or rows) one sweep of the COO kernels' grid covers
NORM_SWEEP = 16384 * 4        # rows one sweep of the row normalisation covers (one wave per row)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pygcn_amd import _native
    _native.lib()
    return torch.device("cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    if want.dtype != np.float32:
        got, want = got.astype(np.int64), want.astype(np.int64)
    else:
        assert got.dtype == np.float32
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: " \
                          f"{got[bad[0]]!r} vs {want[bad[0]]!r}"


# ---------------------------------------------------------------- the large COO input
N_ROWS, N_COLS, N_TRIPLETS = 2_500_003, 2_400_001, 6_000_011
N_DUP, HOT, N_EMPTY, STRADDLE_EXTRA = 1_500_000, 5_000, 1_200, 8


class _BigCoo:
    """Unsorted COO: ~1.5 M duplicated pairs anywhere, one key stored 5 000 times all over the
    array, a run of duplicates across position SWEEP of the SORTED order, 1 200 empty rows (the
    first and the last among them), entries in the last column.  Standard normal values."""

    def __init__(self):
        rng = np.random.default_rng(2024)
        empty = np.unique(np.concatenate([[0, N_ROWS - 1], rng.integers(0, N_ROWS, N_EMPTY - 2)]))
        allowed = np.setdiff1d(np.arange(N_ROWS), empty)
        n_base = N_TRIPLETS - N_DUP - HOT - STRADDLE_EXTRA
        rows = allowed[rng.integers(0, allowed.size, n_base)]
        cols = rng.integers(0, N_COLS, n_base)
        cols[rng.integers(0, n_base, 3000)] = N_COLS - 1
        rows[-1], cols[-1] = allowed[-1], N_COLS - 1             # the largest key there can be
        pick = rng.integers(0, n_base, N_DUP)
        hot_r, hot_c = allowed[allowed.size // 3], N_COLS // 2 + 1
        rows = np.concatenate([rows, rows[pick], np.full(HOT, hot_r)])
        cols = np.concatenate([cols, cols[pick], np.full(HOT, hot_c)])
        # the key at position SWEEP - 1 of the sorted order, stored a few more times: its run
        # then has members on both sides of the place where the sorted entry loop wraps
        ks = np.sort(rows * N_COLS + cols)
        k = ks[SWEEP - 1]
        rows = np.concatenate([rows, np.full(STRADDLE_EXTRA, k // N_COLS)])
        cols = np.concatenate([cols, np.full(STRADDLE_EXTRA, k % N_COLS)])
        perm = rng.permutation(rows.size)
        self.rows, self.cols = rows[perm].astype(np.int64), cols[perm].astype(np.int64)
        self.vals = rng.standard_normal(rows.size).astype(np.float32)
        self.empty, self.hot_key, self.straddle_key = empty, hot_r * N_COLS + hot_c, int(k)
        self.shape, self.last_row = (N_ROWS, N_COLS), int(allowed[-1])
        self._ref = {}

    def reference(self, reduce):
        if reduce not in self._ref:
            self._ref[reduce] = R.coo_reduce_reference(self.rows, self.cols, self.vals, N_ROWS, N_COLS, reduce)
        return self._ref[reduce]

    def check_construction(self):
        key = self.rows * N_COLS + self.cols
        assert key.size == N_TRIPLETS and key.size > 2 * SWEEP and N_ROWS > SWEEP
        assert int(key.max()) == self.last_row * N_COLS + N_COLS - 1 >= 2 ** 42
        assert math.ceil(math.log2(N_ROWS * N_COLS)) == 43
        ks = np.sort(key)
        assert ks[SWEEP - 1] == ks[SWEEP] == self.straddle_key                # the run straddles
        where = np.flatnonzero(key == self.hot_key)
        assert where.size >= HOT and where[0] < key.size // 50 and where[-1] > key.size - key.size // 50
        assert np.diff(where).max() < key.size // 100                        # spread, not clustered
        uniq, count = np.unique(key, return_counts=True)
        assert (count > 1).sum() > 1_000_000 and key.size - uniq.size > 1_400_000
        rowptr = self.reference("sum")[0]
        deg = np.diff(rowptr)
        assert (deg[self.empty] == 0).all() and self.empty.size >= 1000
        assert deg[0] == 0 and deg[-1] == 0
        assert (self.reference("sum")[1] == N_COLS - 1).sum() > 2000
        return uniq.size


@pytest.fixture(scope="module")
def big():
    b = _BigCoo()
    b.n_distinct = b.check_construction()
    return b


def _from_coo(big, dev, reduce):
    from pygcn_amd import CSRGraph
    return CSRGraph.from_coo(torch.from_numpy(big.rows), torch.from_numpy(big.cols),
                             torch.from_numpy(big.vals), big.shape, device=dev, reduce=reduce)


# ---------------------------------------------------------------- (a) COO -> CSR past one sweep
@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_coo_to_csr_past_one_sweep_is_bitwise_the_sequential_reduction(dev, big, reduce):
    """rowptr, col, val and nnz of the device conversion equal the host reference bit for bit —
    every entry, both reductions — and a second run gives the same bits."""
    rowptr, col, val = big.reference(reduce)
    g = _from_coo(big, dev, reduce)
    assert g.nnz == big.n_distinct == col.size and g.shape == big.shape
    assert g.rowptr.dtype == torch.int32
    _same(g.rowptr, rowptr, "rowptr")
    _same(g.col, col, "col")
    _same(g.val, val, "val")
    again = _from_coo(big, dev, reduce)
    assert torch.equal(again.rowptr, g.rowptr) and torch.equal(again.col, g.col)
    assert torch.equal(again.val.view(torch.int32), g.val.view(torch.int32))


# ---------------------------------------------------------------- (b) 64-bit row pointers
def _coo_to_csr_raw(big, dev, reduce, is64):
    """gcn_coo_to_csr_device called directly (Python asks for 64-bit row pointers only at
    nnz >= 2^31 - 1)."""
    from pygcn_amd import _native
    L = _native.lib()
    row, col, val = (torch.from_numpy(a).to(dev) for a in (big.rows, big.cols, big.vals))
    nnz = row.numel()
    rowptr = torch.full((N_ROWS + 1,), -1, dtype=torch.int64 if is64 else torch.int32, device=dev)
    col_out = torch.full((nnz,), -1, dtype=torch.int32, device=dev)
    val_out = torch.zeros(nnz, dtype=torch.float32, device=dev)
    nnz_out = torch.zeros(1, dtype=torch.int64, device=dev)
    ws_bytes = L.gcn_coo_to_csr_workspace_bytes(N_ROWS, N_COLS, nnz)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.gcn_coo_to_csr_device(row.data_ptr(), col.data_ptr(), val.data_ptr(), nnz, N_ROWS, N_COLS,
                                     {"sum": _native.GCN_REDUCE_SUM, "max": _native.GCN_REDUCE_MAX}[reduce],
                                     rowptr.data_ptr(), int(is64), col_out.data_ptr(), val_out.data_ptr(),
                                     nnz_out.data_ptr(), ws.data_ptr(), ws_bytes,
                                     torch.cuda.current_stream().cuda_stream)
    _native.check(rc, "gcn_coo_to_csr_device")
    torch.cuda.synchronize()
    k = int(nnz_out.item())
    return rowptr, col_out[:k], val_out[:k], k


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_coo_to_csr_with_64_bit_row_pointers(dev, big, reduce):
    rowptr, col, val = big.reference(reduce)
    rp64, c64, v64, k64 = _coo_to_csr_raw(big, dev, reduce, True)
    rp32, c32, v32, k32 = _coo_to_csr_raw(big, dev, reduce, False)
    assert rp64.dtype == torch.int64 and rp32.dtype == torch.int32 and k64 == k32 == col.size
    assert torch.equal(rp64, rp32.to(torch.int64))
    assert torch.equal(c64, c32) and torch.equal(v64.view(torch.int32), v32.view(torch.int32))
    _same(rp64, rowptr, "int64 rowptr")
    _same(c64, col, "col")
    _same(v64, val, "val")


def test_row_normalize_and_transpose_with_64_bit_row_pointers(dev, big):
    """The int64_t instantiations of the normalisation and of pack / unpack give the bits of the
    int32_t ones (and the transposed row pointer comes back 64 bits wide)."""
    from pygcn_amd import CSRGraph
    rowptr, col, val = big.reference("sum")
    t = lambda a: torch.from_numpy(a).to(dev)                             # noqa: E731
    g32 = CSRGraph(t(rowptr.astype(np.int32)), t(col), t(val), big.shape)
    g64 = CSRGraph(t(rowptr), t(col), t(val), big.shape)
    assert g64.rowptr.dtype == torch.int64
    t32, t64 = g32.t(), g64.t()
    assert t64.rowptr.dtype == torch.int64 and t32.rowptr.dtype == torch.int32
    assert torch.equal(t64.rowptr, t32.rowptr.to(torch.int64)) and torch.equal(t64.col, t32.col)
    assert torch.equal(t64.val.view(torch.int32), t32.val.view(torch.int32))
    rp_t, col_t, val_t = R.transpose_reference(rowptr, col, val, N_COLS)
    _same(t64.rowptr, rp_t, "int64 rowptr of the transpose")
    _same(t64.col, col_t, "col of the transpose")
    _same(t64.val, val_t, "val of the transpose")
    g32.row_normalize_()
    g64.row_normalize_()
    assert torch.equal(g64.val.view(torch.int32), g32.val.view(torch.int32))
    assert not torch.equal(g64.val, t(val))
    # (standard normal rows: the sums cancel, so only the well-conditioned rows are gated here;
    #  the accuracy of the normalisation is the subject of the tests further down)
    got = g64.val.cpu().numpy().astype(np.float64)
    bound, s = R.row_normalize_bounds(rowptr, val)
    row = np.repeat(np.arange(N_ROWS), np.diff(rowptr))
    well = (bound <= 100 * 9 * R.U32)[row]                  # (no row here has more than 64 entries)
    assert np.diff(rowptr).max() <= 64 and well.mean() > 0.9
    ref = val.astype(np.float64)[well] / s[row[well]]
    assert (np.abs(got[well] - ref) <= bound[row[well]] * np.abs(ref)).all()


# ---------------------------------------------------------------- (c) the recipe at C3 scale
RMAT_N, RMAT_E, RMAT_SEED = 1_000_000, 10_000_000, 5


@pytest.fixture(scope="module")
def rmat_pairs():
    """10^7 R-MAT pairs over 10^6 vertices WITHOUT the vertex permutation: repeated pairs
    (multiplicities up to 127), both directions with different multiplicities, self-loops, a
    largest symmetrized row of tens of thousands of entries, isolated vertices."""
    from pygcn_amd.utils import rmat_edges
    src, dst = rmat_edges(RMAT_N, RMAT_E, seed=RMAT_SEED)
    edges = torch.stack([src, dst], 1).numpy()
    key = edges[:, 0] * RMAT_N + edges[:, 1]
    uniq, count = np.unique(key, return_counts=True)
    assert uniq.size == 9_709_918 and count.max() == 127
    assert int((uniq // RMAT_N == uniq % RMAT_N).sum()) == 291
    return edges


_RECIPE = {}


def _recipe_reference(edges, **kw):
    k = tuple(sorted(kw.items()))
    if k not in _RECIPE:
        _RECIPE[k] = R.adjacency_recipe_reference(edges, RMAT_N, **kw)
    return _RECIPE[k]


def _check_recipe(dev, edges, n, what, exact=False, reference=None, **kw):
    """from_edge_list against the scipy recipe: structure equal; values within rtol 2e-7 of the
    float64 result rounded to float32, and the worst relative error printed next to the gate.
    Derivation of the gate: every stored value and every row sum before the normalisation is an
    integer below 2^24, so the float32 row sum is exact in any order; what remains is 1/s
    (correctly rounded: 2^-24 relative), v · (1/s) (2^-24) and the rounding of the float64 reference
    to float32 (2^-24): 3 · 2^-24 = 1.8e-7.  Without `normalize` nothing is rounded at all: bitwise.
    Measured on the MI355X: 1.19e-7 in every normalized case."""
    from pygcn_amd import CSRGraph
    rowptr, col, val = reference or R.adjacency_recipe_reference(edges, n, **kw)
    g = CSRGraph.from_edge_list(edges, n, device=dev, **kw)
    assert g.nnz == col.size
    _same(g.rowptr, rowptr, what + ": rowptr")
    _same(g.col, col, what + ": col")
    got, want = g.val.cpu().numpy(), val.astype(np.float32)
    if exact:
        assert (val == np.round(val)).all() and val.max() < 2 ** 24
        _same(got, want, what + ": val")
        return g, 0.0
    worst = float(np.abs(got.astype(np.float64) / want.astype(np.float64) - 1).max())
    print(f"[ingest] {what}: worst relative error of val {worst:.3e} (gate 2e-7), nnz {g.nnz}")
    np.testing.assert_allclose(got, want, rtol=2e-7, atol=0, err_msg=what)
    return g, worst


def test_recipe_on_rmat_pairs_with_repeats_and_self_loops(dev, rmat_pairs):
    ref = _recipe_reference(rmat_pairs)
    deg = np.diff(ref[0])
    assert deg.max() > 40_000 and (deg == 1).sum() > 1000          # a huge row; isolated vertices (+I only)
    g, _ = _check_recipe(dev, rmat_pairs, RMAT_N, "recipe", reference=ref)
    # the normalized rows sum to 1 (summed in float64): every entry within 2 roundings of v / s
    sums = torch.zeros(RMAT_N, dtype=torch.float64, device=dev).index_add_(0, g.coo()[0], g.val.double())
    assert float((sums - 1).abs().max()) <= 2.0 ** -23 * 1.001


def test_recipe_without_symmetrization(dev, rmat_pairs):
    ref = _recipe_reference(rmat_pairs, symmetrize=False)
    g, _ = _check_recipe(dev, rmat_pairs, RMAT_N, "symmetrize=False", reference=ref, symmetrize=False)
    # it really is not symmetric: the transposed pattern differs
    t = g.t()
    assert not (torch.equal(t.rowptr, g.rowptr) and torch.equal(t.col, g.col))


def test_recipe_without_self_loops(dev, rmat_pairs):
    """Besides the gate against float64: the values are BITWISE fl(v · fl(1/s)) — the row sums are
    exact integers, the reciprocal is a correctly rounded division and the product one rounding, so
    numpy's float32 arithmetic states the same two operations."""
    ref = _recipe_reference(rmat_pairs, self_loops=False)
    assert (np.diff(ref[0]) == 0).sum() > 1000                     # isolated vertices: empty rows
    g, _ = _check_recipe(dev, rmat_pairs, RMAT_N, "self_loops=False", reference=ref, self_loops=False)
    raw = _recipe_reference(rmat_pairs, self_loops=False, normalize=False)
    assert np.array_equal(raw[0], ref[0]) and np.array_equal(raw[1], ref[1])
    s = np.add.reduceat(raw[2], raw[0][:-1][np.diff(raw[0]) > 0])
    assert s.max() < 2 ** 24
    inv = np.zeros(RMAT_N, np.float32)
    inv[np.diff(raw[0]) > 0] = np.float32(1) / s.astype(np.float32)
    want = raw[2].astype(np.float32) * np.repeat(inv, np.diff(raw[0]))
    assert want.dtype == np.float32
    _same(g.val, want, "self_loops=False: val against fl(v · fl(1/s))")


def test_recipe_without_normalisation_is_exact(dev, rmat_pairs):
    ref = _recipe_reference(rmat_pairs, normalize=False)
    assert ref[2].max() == 128                 # the pair stored 127 times is a self-loop: + I makes 128
    g, _ = _check_recipe(dev, rmat_pairs, RMAT_N, "normalize=False", exact=True, reference=ref,
                         normalize=False)
    t = g.t()                                                      # max(A, A^T) + I is symmetric
    assert torch.equal(t.rowptr, g.rowptr) and torch.equal(t.col, g.col) and torch.equal(t.val, g.val)


def test_recipe_on_a_hand_written_multigraph(dev):
    """11 vertices, compared as dense matrices: 0 -> 1 three times and 1 -> 0 once, a self-loop in
    the list (twice), vertex 9 isolated, vertex 10 with in-edges only, repeated pairs."""
    from pygcn_amd import CSRGraph
    n = 11
    edges = np.array([[0, 1], [1, 0], [0, 1], [0, 1], [2, 2], [2, 2], [2, 3], [3, 2], [4, 5], [4, 5],
                      [5, 6], [6, 4], [7, 10], [8, 10], [8, 10], [3, 10], [1, 7], [7, 1], [7, 1]])
    a = np.zeros((n, n))
    for s, d in edges:
        a[s, d] += 1
    assert a[0, 1] == 3 and a[1, 0] == 1 and a[2, 2] == 2 and not a[9].any() and not a[:, 9].any()
    assert not a[10].any() and a[:, 10].sum() == 4

    def dense(**kw):
        g = CSRGraph.from_edge_list(edges, n, device=dev, **kw)
        m = sp.csr_matrix((g.val.cpu().numpy(), g.col.cpu().numpy(), g.rowptr.cpu().numpy()), shape=(n, n))
        assert m.has_sorted_indices or np.all(np.diff(m.indices) != 0)
        return m.toarray(), g
    got, g = dense(symmetrize=False, self_loops=False, normalize=False)
    assert got.dtype == np.float32 and np.array_equal(got, a) and g.nnz == np.count_nonzero(a)
    sym = np.maximum(a, a.T)
    got, g = dense(self_loops=False, normalize=False)
    assert np.array_equal(got, sym), f"\n{got}\n{sym}"
    assert g.rowptr[9].item() == g.rowptr[10].item()                       # the isolated vertex: empty row
    got, g = dense(normalize=False)
    assert np.array_equal(got, sym + np.eye(n)), f"\n{got}\n{sym + np.eye(n)}"
    assert got[2, 2] == 3 and got[9, 9] == 1                               # the listed self-loop counts
    full = sym + np.eye(n)
    want = full / full.sum(1, keepdims=True)
    got, g = dense()
    np.testing.assert_allclose(got, want.astype(np.float32), rtol=2e-7, atol=0)
    got, _ = dense(symmetrize=False)
    dir_ = a + np.eye(n)
    np.testing.assert_allclose(got, (dir_ / dir_.sum(1, keepdims=True)).astype(np.float32), rtol=2e-7, atol=0)
    got, _ = dense(self_loops=False)
    with np.errstate(invalid="ignore"):
        want = np.nan_to_num(sym / sym.sum(1, keepdims=True))
    np.testing.assert_allclose(got, want.astype(np.float32), rtol=2e-7, atol=0)
    assert not got[9].any()
    rp, c, v = R.adjacency_recipe_reference(edges, n)
    assert np.allclose(sp.csr_matrix((v, c, rp), shape=(n, n)).toarray(), full / full.sum(1, keepdims=True))


# ---------------------------------------------------------------- (d) row normalisation
NORM_ROWS = 200_000
NORM_SPECIAL = {5: "cancels", 6: "stored_zeros", 7: "subnormal_sum", 8: "overflowing_sum", 9: "nan",
                70_001: "subnormal_sum", 70_002: "nan", 131_073: "cancels", 131_074: "overflowing_sum",
                199_998: "stored_zeros", 199_999: "subnormal_sum"}
NORM_LENGTHS = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 65_536: 4097, 65_537: 0, 150_000: 100_000,
                199_997: 65, 199_996: 0}


def _check_row_normalize(dev, rowptr, col, val, shape, special, what, idx64=False):
    """The kernel on (rowptr, col, val) against float64 row sums and division.  Ordinary rows: every
    entry within row_normalize_bound of its row; the condition number of every ordinary row is
    asserted <= 100 here, so no row is excused.  Special rows: exactly what the project's
    `normalize` gives on the float32 matrix (zeros or NaN)."""
    from pygcn_amd import CSRGraph
    from pygcn_amd.utils import normalize
    n_rows = shape[0]
    length = np.diff(rowptr)
    row = np.repeat(np.arange(n_rows), length)
    is_special = np.zeros(n_rows, bool)
    is_special[list(special)] = True
    bound, s = R.row_normalize_bounds(rowptr, val)
    ordinary = ~is_special & (length > 0)
    units = (-(-length // 64) + 8) * R.U32
    assert (bound[ordinary] <= 100 * units[ordinary]).all(), "an ordinary row is ill-conditioned"
    assert (s[ordinary] < 0).sum() > 0 or n_rows < 10_000           # negative sums are ordinary rows
    g = CSRGraph(torch.from_numpy(rowptr.astype(np.int64 if idx64 else np.int32)).to(dev),
                 torch.from_numpy(col).to(dev), torch.from_numpy(val).to(dev), shape)
    assert g.row_normalize_() is g
    got = g.val.cpu().numpy()
    e_ord = ordinary[row]
    ref = val[e_ord].astype(np.float64) / s[row[e_ord]]
    err = np.abs(got[e_ord].astype(np.float64) - ref)
    gate = bound[row[e_ord]] * np.abs(ref)
    worst = float((err / gate).max())
    at = row[e_ord][int((err / gate).argmax())]
    print(f"[ingest] {what}: worst error / gate {worst:.3f} (row {at}, {length[at]} entries, gate "
          f"{bound[at] / R.U32:.1f} · 2^-24), worst relative error {float((err / np.abs(ref)).max()):.3e}")
    assert (err <= gate).all(), f"{what}: {int((err > gate).sum())} entries miss the gate, worst x{worst:.2f}"
    # special rows, exactly as the reference semantics on the float32 matrix
    rows_s = np.array(sorted(special))
    for r in rows_s:                                   # (first row by row, so that a failure names it)
        stored = got[rowptr[r]:rowptr[r + 1]]
        if special[r] == "nan":
            assert np.isnan(stored).all(), f"{what}: row {r} ({special[r]}) became {stored}"
        else:
            assert (stored == 0).all(), f"{what}: row {r} ({special[r]}) became {stored}"
    with np.errstate(all="ignore"):
        want = sp.csr_matrix(normalize(sp.csr_matrix((val, col, rowptr), shape=shape)))[rows_s].toarray()
    got_m = sp.csr_matrix((got, col, rowptr), shape=shape)[rows_s].toarray()
    np.testing.assert_array_equal(got_m, want, err_msg=what + ": special rows")
    assert np.isfinite(got[~is_special[row]]).all()                # NaN / inf stay in their own rows
    return got, worst


def test_row_normalize_past_one_sweep_and_on_the_rows_that_do_not_divide(dev):
    """200 000 rows (more than three sweeps of 65 536 waves), lengths 0 ... 100 000, mixed signs.
    Measured on the MI355X: worst error 0.38 of the gate (a 14-entry row), worst relative error
    1.9e-6 (on an ill-conditioned row, inside its gate)."""
    rng = np.random.default_rng(77)
    lengths = rng.integers(0, 21, NORM_ROWS)
    for r, n in NORM_LENGTHS.items():
        lengths[r] = n
    n_cols = 200_000
    rowptr, col, val = gin.normalize_matrix(lengths, n_cols, seed=78, special=NORM_SPECIAL)
    assert NORM_ROWS > 3 * NORM_SWEEP and all(np.diff(rowptr)[r] == n for r, n in NORM_LENGTHS.items())
    assert (val < 0).mean() > 0.05
    _check_row_normalize(dev, rowptr, col, val, (NORM_ROWS, n_cols), NORM_SPECIAL, "row_normalize 200k")
    _check_row_normalize(dev, rowptr, col, val, (NORM_ROWS, n_cols), NORM_SPECIAL,
                         "row_normalize 200k, int64 rowptr", idx64=True)


def test_row_normalize_against_the_captured_reference_output(dev):
    """The kernel against fixture g6_normalize.npz (the reference's own `normalize` on the seeded
    matrix of inputs.g6_normalize_input, captured through its live code): the special rows exactly,
    every other entry at the gate of the test above."""
    z = load_golden("g6_normalize.npz")
    rowptr, col, val, shape = gin.g6_normalize_input()
    got, _ = _check_row_normalize(dev, rowptr, col, val, shape, gin.G6_SPECIAL, "row_normalize g6")
    fixture = sp.coo_matrix((z["coo_val"], (z["coo_row"], z["coo_col"])), shape=shape).toarray()
    row = np.repeat(np.arange(shape[0]), np.diff(rowptr))
    want = fixture[row, col]                        # (the reference's product drops the zeros it makes)
    special = np.isin(row, list(gin.G6_SPECIAL))
    np.testing.assert_array_equal(got[special], want[special])
    assert np.isnan(got[special]).sum() == 3 and (got[special] == 0).sum() == special.sum() - 3
    bound, _ = R.row_normalize_bounds(rowptr, val)
    err = np.abs(got[~special].astype(np.float64) - want[~special])
    gate = bound[row[~special]] * np.abs(want[~special].astype(np.float64))
    print(f"[ingest] row_normalize g6 against the fixture: worst error / gate {float((err / gate).max()):.3f}")
    assert (err <= gate).all()


# ---------------------------------------------------------------- (e) transpose, entry for entry
def _check_transpose(dev, rowptr, col, val, shape, what):
    from pygcn_amd import CSRGraph
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    g = CSRGraph(t(rowptr.astype(np.int32)), t(col), t(val), shape)
    gt = g.t()
    rp_t, col_t, val_t = R.transpose_reference(rowptr, col, val, shape[1])
    assert gt.shape == (shape[1], shape[0]) and gt.nnz == g.nnz
    _same(gt.rowptr, rp_t, what + ": rowptr of the transpose")
    _same(gt.col, col_t, what + ": col of the transpose")           # order inside every row
    _same(gt.val, val_t, what + ": val of the transpose")
    fresh = CSRGraph(gt.rowptr.clone(), gt.col.clone(), gt.val.clone(), gt.shape)
    back = fresh.t()
    assert back is not g
    _same(back.rowptr, rowptr, what + ": rowptr after two transposes")
    _same(back.col, col, what + ": col after two transposes")
    _same(back.val, val, what + ": val after two transposes")


def test_transpose_entry_for_entry_on_the_rectangular_matrix(dev, big):
    rowptr, col, val = big.reference("sum")
    assert col.size > 2 * SWEEP and N_COLS + 1 > SWEEP and N_ROWS != N_COLS
    _check_transpose(dev, rowptr, col, val, big.shape, "rectangular")


def test_transpose_entry_for_entry_on_the_rmat_adjacency(dev, rmat_pairs):
    rowptr, col, val = _recipe_reference(rmat_pairs)
    assert col.size > 8 * SWEEP
    _check_transpose(dev, rowptr, col, val.astype(np.float32), (RMAT_N, RMAT_N), "R-MAT adjacency")


# ---------------------------------------------------------------- (f) the compat entry point
def test_uncoalesced_sparse_coo_tensor_through_as_graph(dev, big, monkeypatch):
    """`model(features, adj)` with the reference's layout: an UNCOALESCED sparse COO tensor of the
    6 000 011 triplets -> as_graph -> from_torch -> from_coo -> the device conversion; the product
    against a float64 index_add_ over the raw triplets (which sums the duplicates itself)."""
    from pygcn_amd import CSRGraph, as_graph, spmm_csr
    F = 16
    idx = torch.from_numpy(np.stack([big.rows, big.cols])).to(dev)
    vals = torch.from_numpy(big.vals).to(dev)
    adj = torch.sparse_coo_tensor(idx, vals, big.shape)
    assert not adj.is_coalesced() and adj._nnz() == N_TRIPLETS
    B = torch.from_numpy(gin.dense((N_COLS, F), 31)).to(dev)
    g = as_graph(adj)
    assert g.nnz == big.n_distinct and g.shape == big.shape
    out = spmm_csr(g, B)
    ref = torch.zeros((N_ROWS, F), dtype=torch.float64, device=dev)
    for s in range(0, N_TRIPLETS, SWEEP):
        e = min(s + SWEEP, N_TRIPLETS)
        ref.index_add_(0, idx[0, s:e], B.index_select(0, idx[1, s:e]).double() * vals[s:e].double().unsqueeze(1))
    assert_normwise(out.cpu().numpy(), ref.cpu().numpy(), 1e-5, "A·B from the uncoalesced COO tensor")
    # the handle is cached on the tensor: a second call converts nothing
    def boom(*a, **k):
        raise AssertionError("as_graph converted a tensor it had already prepared")
    monkeypatch.setattr(CSRGraph, "from_torch", classmethod(boom))
    monkeypatch.setattr(CSRGraph, "from_coo", classmethod(boom))
    assert as_graph(adj) is g


# ---------------------------------------------------------------- (g) non-finite duplicates
def test_non_finite_values_in_duplicates_stay_in_their_entry(dev):
    """What the header of gcn_coo_to_csr_device states: under sum a run [1, inf, 2] gives inf and
    [1, nan] gives NaN, in that entry only; max is fmaxf — a NaN member is ignored, the entry is
    NaN only if its whole run is."""
    from pygcn_amd import CSRGraph
    inf, nan = float("inf"), float("nan")
    rows = np.array([0, 1, 0, 1, 0, 2, 2, 1, 3, 3, 0, 3])
    cols = np.array([1, 2, 1, 2, 1, 0, 0, 0, 3, 3, 0, 2])
    vals = np.array([1, 1, inf, nan, 2, -inf, inf, 7, nan, nan, 5, -4], np.float32)
    want = {"sum": [5, inf, 7, nan, nan, -4, nan], "max": [5, inf, 7, 1, inf, -4, nan]}
    for reduce in ("sum", "max"):
        g = CSRGraph.from_coo(torch.from_numpy(rows), torch.from_numpy(cols), torch.from_numpy(vals),
                              (4, 4), device=dev, reduce=reduce)
        rowptr, col, val = R.coo_reduce_reference(rows, cols, vals, 4, 4, reduce)
        assert g.rowptr.tolist() == rowptr.tolist() == [0, 2, 4, 5, 7]
        assert g.col.tolist() == col.tolist() == [0, 1, 0, 2, 0, 2, 3]
        np.testing.assert_array_equal(val, np.array(want[reduce], np.float32))
        np.testing.assert_array_equal(g.val.cpu().numpy(), np.array(want[reduce], np.float32))
