"""The float64 reference of the full-size tests (tests/_f64.py) against the CPU oracle on a small
skewed graph: a hub row, a hub column, empty rows and columns, duplicate entries — so the arbiter
of the large-height checks is itself under test.  No GPU."""
import numpy as np
import torch

import _f64


def _skewed(rng, n_rows, n_cols, per_row):
    deg = rng.poisson(per_row, n_rows)
    deg[::17] = 0                                    # empty rows
    deg[3] = n_cols * 2                              # a hub row (with duplicate columns)
    rows = np.repeat(np.arange(n_rows), deg)
    cols = rng.integers(0, n_cols - 5, rows.size)    # the last 5 columns stay empty
    cols[rng.random(rows.size) < 0.2] = 7            # a hub column
    val = rng.standard_normal(rows.size).astype(np.float32)
    rowptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    return rowptr, cols.astype(np.int32), val


def test_f64_reference_against_the_oracle(oracle):
    rng = np.random.default_rng(5)
    n_rows, n_cols, F = 601, 397, 24
    rowptr, col, val = _skewed(rng, n_rows, n_cols, 6)
    a = oracle.CSR(rowptr, col, val, (n_rows, n_cols))
    B = rng.standard_normal((n_cols, F)).astype(np.float32)
    G = rng.standard_normal((n_rows, F)).astype(np.float32)
    t = lambda x: torch.from_numpy(x)                                   # noqa: E731
    # small chunks: every product crosses many chunk boundaries, one chunk ends mid-row
    got = _f64.spmm64(t(rowptr), t(col), t(val), t(B), chunk=97)
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), oracle.spmm_csr_f64acc(rowptr, col, val, B), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got.numpy(), a.matmul(B), rtol=0, atol=1e-5 * np.abs(got.numpy()).max())
    got_t = _f64.spmm64_t(t(rowptr), t(col), t(val), t(G), n_cols, chunk=101)
    ref_t = a.t_matmul(G)
    np.testing.assert_allclose(got_t.numpy(), ref_t, rtol=0, atol=1e-5 * np.abs(ref_t).max())
    dense = np.zeros((n_rows, n_cols))
    np.add.at(dense, (np.repeat(np.arange(n_rows), np.diff(rowptr)), col), val.astype(np.float64))
    np.testing.assert_allclose(got_t.numpy(), dense.T @ G.astype(np.float64), rtol=1e-12, atol=1e-12)
    assert not got_t[-5:].any() and not got[::17].any()
    # leaving one chunk out must show
    assert not np.allclose(_f64.spmm64(t(rowptr), t(col), t(val), t(B), chunk=97, skip_chunk=2).numpy(),
                           got.numpy())


def test_f64_dense_products():
    gen = torch.Generator().manual_seed(3)
    A = torch.randn(1000, 48, generator=gen)
    W = torch.randn(48, 32, generator=gen)
    G = torch.randn(1500, 32, generator=gen).bfloat16()
    ref = A.double() @ W.double()
    assert torch.allclose(_f64.mm64(A, W, chunk=77), ref, rtol=1e-13, atol=1e-13)
    ra = torch.randint(0, 1000, (555,), generator=gen, dtype=torch.int32)
    rg = torch.randperm(1500, generator=gen)[:555].to(torch.int32)
    got, summ = _f64.tn64(A, G, ra, rg, chunk=64, absolute=True)
    want = A[ra.long()].double().t() @ G[rg.long()].double()
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(summ, A[ra.long()].double().abs().t() @ G[rg.long()].double().abs(), rtol=1e-12)
    s, sa = _f64.colsum64(G, chunk=100)
    assert torch.allclose(s, G.double().sum(0), rtol=1e-12, atol=1e-12)
    assert torch.allclose(sa, G.double().abs().sum(0), rtol=1e-12)
    # float64 operands are read through views: the helpers must leave them as they were
    A64, G64 = A.double() - 0.5, G.double() - 0.5
    a0, g0 = A64.clone(), G64.clone()
    _f64.tn64(A64, G64[:1000], absolute=True)
    _f64.colsum64(G64)
    _f64.spmm64_t(torch.tensor([0, 2, 3]), torch.tensor([1, 0, 1], dtype=torch.int32), torch.ones(3), G64[:2], 2)
    assert torch.equal(A64, a0) and torch.equal(G64, g0)
