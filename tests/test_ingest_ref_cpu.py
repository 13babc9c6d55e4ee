"""The host references of the ingest tests (tests/_ingest_ref.py) pinned against independent
statements of the same operations — a naive Python loop, scipy, numpy's reduceat, the CPU oracle,
the golden fixtures — so the arbiter of tests/test_ingest_scale_gpu.py is itself under test.
No GPU."""
import sys

import numpy as np
import scipy.sparse as sp

import _ingest_ref as R
import inputs as gin
from conftest import load_golden


def _runs_1_to_40(seed=11, n_rows=37, n_cols=29):
    """Unsorted COO in which the k-th distinct pair is stored k times, k = 1...40, its copies
    spread over the whole array; standard normal values."""
    rng = np.random.default_rng(seed)
    pairs = rng.choice(n_rows * n_cols, size=40, replace=False)
    key = np.repeat(pairs, np.arange(1, 41))
    perm = rng.permutation(key.size)
    key = key[perm]
    vals = rng.standard_normal(key.size).astype(np.float32)
    return key // n_cols, key % n_cols, vals, n_rows, n_cols


def _naive(rows, cols, vals, n_rows, n_cols, reduce):
    """One Python loop per run, one float32 operation per member."""
    key = rows * n_cols + cols
    order = np.argsort(key, kind="stable")
    out = {}
    for k, v in zip(key[order], vals[order]):
        if k not in out:
            out[k] = np.float32(v)
        elif reduce == "sum":
            out[k] = np.float32(out[k] + np.float32(v))
        else:
            out[k] = max(out[k], np.float32(v))
    uk = np.array(sorted(out))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(uk // n_cols, minlength=n_rows))])
    return rowptr, (uk % n_cols).astype(np.int32), np.array([out[k] for k in uk], np.float32)


def test_sequential_reduction_equals_a_naive_loop():
    rows, cols, vals, n_rows, n_cols = _runs_1_to_40()
    for reduce in ("sum", "max"):
        rowptr, col, val = R.coo_reduce_reference(rows, cols, vals, n_rows, n_cols, reduce)
        n_rowptr, n_col, n_val = _naive(rows, cols, vals, n_rows, n_cols, reduce)
        assert rowptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.float32
        assert np.array_equal(rowptr, n_rowptr) and np.array_equal(col, n_col)
        assert np.array_equal(val.view(np.int32), n_val.view(np.int32)), reduce        # bitwise
    # the order matters (otherwise "bitwise" would pin nothing): summing the runs backwards
    # gives other bits somewhere
    back = R.coo_reduce_reference(rows[::-1], cols[::-1], vals[::-1], n_rows, n_cols, "sum")[2]
    fwd = R.coo_reduce_reference(rows, cols, vals, n_rows, n_cols, "sum")[2]
    assert not np.array_equal(back, fwd)
    np.testing.assert_allclose(back, fwd, rtol=0, atol=1e-3)     # (<= 2·39 roundings of Σ|v| <= 200)


def test_sequential_reduction_against_scipy_and_reduceat():
    rows, cols, vals = gin.random_coo(300, 211, 6000, seed=5, duplicates=3000, hub_row=9, hub_deg=400,
                                      empty_rows=(0, 150, 299))
    vals = np.random.default_rng(6).standard_normal(vals.size).astype(np.float32)
    rowptr, col, val = R.coo_reduce_reference(rows, cols, vals, 300, 211, "sum")
    m = sp.coo_matrix((vals.astype(np.float64), (rows, cols)), shape=(300, 211)).tocsr()
    m.sum_duplicates()
    m.sort_indices()
    assert np.array_equal(rowptr, m.indptr) and np.array_equal(col, m.indices)       # structure: exact
    assert rowptr[0] == rowptr[1] == 0 and rowptr[-1] == rowptr[-2] == col.size     # the empty ends
    # value: the float32 running sum of a run of L members is within (L - 1) roundings of Σ|v|
    key = rows * 211 + cols
    order = np.argsort(key, kind="stable")
    heads = np.flatnonzero(np.concatenate([[True], np.diff(key[order]) != 0]))
    length = np.diff(np.concatenate([heads, [key.size]]))
    mag = np.add.reduceat(np.abs(vals[order].astype(np.float64)), heads)
    assert length.max() >= 3
    assert (np.abs(val - m.data) <= (length - 1) * 2.0 ** -24 * mag * 1.01 + 1e-300).all()
    assert np.array_equal(val[length == 1], vals[order][heads[length == 1]])
    # max: order-free, so numpy's reduceat over the sorted values is the same statement
    val_max = R.coo_reduce_reference(rows, cols, vals, 300, 211, "max")[2]
    assert np.array_equal(val_max, np.maximum.reduceat(vals[order], heads))


def test_reduction_of_non_finite_members():
    """sum propagates inf / NaN inside the run only; max is fmax: NaN members are ignored."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    rows = np.array([0, 1, 0, 1, 0, 2, 2, 1, 3, 3])
    cols = np.array([1, 2, 1, 2, 1, 0, 0, 0, 3, 3])
    vals = np.array([1, 1, inf, nan, 2, -inf, inf, 7, nan, nan], np.float32)
    rowptr, col, s = R.coo_reduce_reference(rows, cols, vals, 4, 4, "sum")
    assert rowptr.tolist() == [0, 1, 3, 4, 5] and col.tolist() == [1, 0, 2, 0, 3]
    np.testing.assert_array_equal(s, np.array([inf, 7, nan, nan, nan], np.float32))
    m = R.coo_reduce_reference(rows, cols, vals, 4, 4, "max")[2]
    np.testing.assert_array_equal(m, np.array([inf, 7, 1, inf, nan], np.float32))


def test_transpose_reference_against_the_oracle_and_scipy(oracle):
    rng = np.random.default_rng(8)
    n_rows, n_cols = 421, 333
    deg = rng.poisson(5, n_rows)
    deg[::13] = 0
    deg[7] = 600                                       # a hub row with duplicate columns
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = rng.integers(0, n_cols - 3, rowptr[-1]).astype(np.int32)      # last 3 columns empty
    val = rng.standard_normal(rowptr[-1]).astype(np.float32)
    got = R.transpose_reference(rowptr, col, val, n_cols)
    want = oracle.csr_transpose(rowptr, col, val, n_cols)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32
    for g, w in zip(got, want):
        assert np.array_equal(g, w)                    # entry for entry, order inside rows included
    # scipy (which sums the duplicates): the same matrix
    a = sp.csr_matrix((val.astype(np.float64), col, rowptr), shape=(n_rows, n_cols))
    t = sp.csr_matrix((got[2].astype(np.float64), got[1], got[0]), shape=(n_cols, n_rows))
    assert abs(t - a.T.tocsr()).max() <= 1e-12
    # and on a matrix without duplicates scipy agrees array for array
    u = sp.random(n_rows, n_cols, density=0.02, random_state=3, format="csr", dtype=np.float32)
    u.sort_indices()
    ut = u.T.tocsr()
    ut.sort_indices()
    got = R.transpose_reference(u.indptr, u.indices, u.data, n_cols)
    assert np.array_equal(got[0], ut.indptr) and np.array_equal(got[1], ut.indices)
    assert np.array_equal(got[2], ut.data)


def test_recipe_reference_reproduces_the_cora_fixture():
    z = load_golden("cora_graph.npz")
    rowptr, col, val = R.adjacency_recipe_reference(z["edges"], int(z["n"]))
    assert val.dtype == np.float64
    assert np.array_equal(rowptr, z["csr_rowptr"]) and np.array_equal(col, z["csr_col"])
    np.testing.assert_allclose(val, z["csr_val"].astype(np.float64), rtol=2.0 ** -23)   # fp32 fixture
    # the switches, on a multigraph small enough to state by hand
    edges = np.array([[0, 1], [0, 1], [1, 0], [2, 2], [3, 0]])
    raw = np.array([[0, 2, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]], np.float64)

    def dense(**kw):
        rp, c, v = R.adjacency_recipe_reference(edges, 4, **kw)
        return sp.csr_matrix((v, c, rp), shape=(4, 4)).toarray()
    assert np.array_equal(dense(symmetrize=False, self_loops=False, normalize=False), raw)
    sym = np.maximum(raw, raw.T)
    assert np.array_equal(dense(self_loops=False, normalize=False), sym)
    assert np.array_equal(dense(normalize=False), sym + np.eye(4))
    full = sym + np.eye(4)
    np.testing.assert_allclose(dense(), full / full.sum(1, keepdims=True), rtol=1e-15)


def test_row_normalize_bound():
    assert R.row_normalize_bound([0.5]) == 9 * 2.0 ** -24
    assert R.row_normalize_bound(np.ones(64)) == 9 * 2.0 ** -24
    assert R.row_normalize_bound(np.ones(65)) == 10 * 2.0 ** -24
    assert R.row_normalize_bound([3.0, -1.0]) == 9 * 2.0 ** -24 * 2
    assert R.row_normalize_bound([1.0, -1.0]) == np.inf
    rowptr, col, val, _ = gin.g6_normalize_input()
    bound, s = R.row_normalize_bounds(rowptr, val)
    for r in (0, 1, 2, 5, gin.G6_LONG_ROW, 1997, 1998):
        v = val[rowptr[r]:rowptr[r + 1]]
        assert s[r] == v.astype(np.float64).sum() or np.isclose(s[r], v.astype(np.float64).sum(), rtol=1e-14)
        if v.size:
            np.testing.assert_allclose(bound[r], R.row_normalize_bound(v), rtol=1e-13)
        else:
            assert bound[r] == np.inf and s[r] == 0
    ordinary = np.setdiff1d(np.flatnonzero(np.diff(rowptr) > 0), list(gin.G6_SPECIAL))
    length = np.diff(rowptr)[ordinary]
    assert (bound[ordinary] <= (-(-length // 64) + 8) * 2.0 ** -24 * 100).all()    # condition <= 100


def test_references_stay_clear_of_the_product():
    """The arbiter shares no code with what it judges: no pygcn_amd.graph, no native library, no
    oracle (the project's `normalize`, pure scipy, is loaded as a stand-alone file)."""
    import subprocess
    code = ("import sys; sys.path[:0] = %r; import _ingest_ref as R; R.product_utils(); "
            "bad = [m for m in sys.modules if m.startswith('pygcn_amd') or m == 'gcn_oracle']; "
            "assert not bad, bad" % [p for p in sys.path if p.endswith(("tests", "golden"))])
    subprocess.check_call([sys.executable, "-c", code])


def test_project_normalize_equals_the_captured_reference_output():
    """pygcn_amd.utils.normalize / sparse_mx_to_torch_sparse_tensor on the seeded matrix of
    fixture g6 (rows that cancel, hold zeros only, sum to a subnormal, overflow, hold a NaN):
    exactly what the reference's own helpers returned."""
    from pygcn_amd.utils import normalize, sparse_mx_to_torch_sparse_tensor
    z = load_golden("g6_normalize.npz")
    rowptr, col, val, shape = gin.g6_normalize_input()
    with np.errstate(all="ignore"):
        mx = sp.csr_matrix(normalize(sp.csr_matrix((val, col, rowptr), shape=shape)))
    assert mx.dtype == np.float32
    assert np.array_equal(mx.indptr, z["indptr"])
    assert np.array_equal(mx.data.view(np.int32), z["val"].view(np.int32))          # bitwise, NaN too
    t = sparse_mx_to_torch_sparse_tensor(mx)
    assert np.array_equal(t._indices()[0].numpy(), z["coo_row"])
    assert np.array_equal(t._indices()[1].numpy(), z["coo_col"])
    assert np.array_equal(t._values().numpy().view(np.int32), z["coo_val"].view(np.int32))
    # what the fixture says about the special rows
    dense = sp.coo_matrix((z["coo_val"], (z["coo_row"], z["coo_col"])), shape=shape).toarray()
    for r, name in gin.G6_SPECIAL.items():
        stored = dense[r, col[rowptr[r]:rowptr[r + 1]]]
        assert np.isnan(stored).all() if name == "nan" else (stored == 0).all(), (r, name, stored)
        assert np.isfinite(dense[[r - 1, (r + 1) % shape[0]]]).all()
