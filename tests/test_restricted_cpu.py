"""What the restricted forward pass (pygcn_amd/fused.py, GCN2RestrictedFunction) rests on that needs no GPU: the
two new C-ABI symbols, the algebra of the restricted step in float64, and GCN.forward's refusals."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import inputs as gin
from conftest import ROOT
from pygcn_amd import _native

NEW = ("gcn_dropout_rows", "gcn_csr_take_rows")


def test_header_tables_and_library_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert int(re.search(r"#define GCN_ABI_VERSION\s+(\d+)", hdr).group(1)) == _native.GCN_ABI_VERSION == 26
    L = _native.lib()
    assert L.gcn_abi_version() == 26
    for name in NEW:
        assert name in _native.SIGNATURES and name in _native.EXPORTS
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl and len(decl.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name
        assert getattr(L, name).argtypes == _native.SIGNATURES[name][1]
    assert len(_native.SIGNATURES["gcn_dropout_rows"][1]) == 11 and len(_native.SIGNATURES["gcn_csr_take_rows"][1]) == 13


def test_argument_errors_are_reported_before_any_launch():
    """p outside [0, 1), m < 0, F < 1, ld < F: GCN_E_BADARG — checked on the host, so no device is needed."""
    L = _native.lib()
    h = 4096         # (never dereferenced: every call below is refused first, or has nothing to do)
    for dtype, ld, m, F, p in ((0, 8, 4, 8, 1.0), (0, 8, 4, 8, -0.25), (0, 8, 4, 8, float("nan")), (0, 8, -1, 8, 0.5),
                               (0, 8, 4, 0, 0.5), (1, 7, 4, 8, 0.5), (2, 8, 4, 8, 0.5)):
        assert L.gcn_dropout_rows(dtype, h, ld, None, m, F, p, 1, None, 0, None) == -1, (dtype, ld, m, F, p)
        assert b"gcn_dropout_rows" in L.gcn_last_error()
    assert L.gcn_dropout_rows(0, h, 8, None, 0, 8, 0.5, 1, None, 0, None) == 0       # m = 0: nothing to do
    assert L.gcn_dropout_rows(0, h, 8, None, 4, 8, 0.0, 1, None, 0, None) == 0       # p = 0: dropout off
    assert L.gcn_csr_take_rows(h, 0, h, h, h, -1, None, h, 0, h, h, None, None) == -1
    assert L.gcn_csr_take_rows(h, 0, h, h, h, 0, None, h, 0, h, h, None, None) == 0


def _log_softmax(z):
    z = z - z.max(1, keepdims=True)
    return z - np.log(np.exp(z).sum(1, keepdims=True))


def _step(A_l1, A_l2, X, W1, b1, W2, b2, keep, scale, labels, pick, reassoc):
    """One training step in float64 on whatever row blocks it is handed: layer 1 through A_l1 (reassociated or
    not), dropout mask `keep`, layer 2 through A_l2; the loss reads the rows `pick` of layer 2's output.
    Returns (picked log-probabilities, grad_W1, grad_b1, grad_W2, grad_b2)."""
    pre1 = ((A_l1 @ X) @ W1 if reassoc else A_l1 @ (X @ W1)) + b1
    h1 = np.where(keep, np.maximum(pre1, 0) * scale, 0.0)
    logp = _log_softmax(A_l2 @ (h1 @ W2) + b2)
    g = np.zeros_like(logp)
    np.add.at(g, (pick, labels), -1.0 / len(pick))
    gpre2 = g - np.exp(logp) * g.sum(1, keepdims=True)
    gsup2 = A_l2.T.tocsr() @ gpre2
    gpre1 = np.where(keep & (pre1 > 0), (gsup2 @ W2.T) * scale, 0.0)
    gW1 = X.T @ (A_l1.T.tocsr() @ gpre1)
    return logp[pick], gW1, gpre1.sum(0), h1.T @ gsup2, gpre2.sum(0)


@pytest.mark.parametrize("reassoc", [False, True])
def test_restricted_step_equals_the_full_step_on_the_loss_rows(oracle, reassoc):
    """The algebra the GPU tests rely on, on the Cora graph in float64: with R the loss rows (here unsorted, one
    listed twice), R2 the columns of Â[R,:], the step through Â[R2,:] and Â[R,R2] — dropout keyed by R2 — gives
    the rows and the four parameter gradients of the step through Â."""
    g = np.load(gin.__file__.replace("inputs.py", "cora_graph.npz"))
    a = oracle.cora_adjacency(g["edges"], int(g["n"]))
    n = a.shape[0]
    A = sp.csr_matrix((a.val.astype(np.float64), a.col, a.rowptr), shape=a.shape)
    X = gin.cora_features().astype(np.float64)
    rng = np.random.default_rng(0)
    W1, b1 = rng.normal(size=(1433, 16)), rng.normal(size=16) * 0.1
    W2, b2 = rng.normal(size=(16, 7)), rng.normal(size=7) * 0.1
    idx = np.concatenate([rng.permutation(n)[:140], [5, 5]])
    labels = rng.integers(0, 7, len(idx))
    seed, p = 0x1234567887654321, 0.5
    scale = float(oracle.dropout_scale(p))
    full = _step(A, A, X, W1, b1, W2, b2, oracle.dropout_keep(seed, np.arange(n), 16, p), scale, labels, idx, reassoc)
    R, inverse = np.unique(idx, return_inverse=True)
    R2 = np.unique(A[R].indices)
    assert 0 < len(R2) < n
    a_rows2, a_block = A[R2], A[R][:, R2]
    assert a_block.nnz == A[R].nnz                       # every column of the rows R lies in R2: nothing is cut off
    part = _step(a_rows2, a_block, X, W1, b1, W2, b2, oracle.dropout_keep(seed, R2, 16, p), scale, labels, inverse,
                 reassoc)
    for got, want, what in zip(part, full, ("rows", "grad_W1", "grad_b1", "grad_W2", "grad_b2")):
        assert got.shape == want.shape, what
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), what
    # and the mask is the point: keyed by the COMPACT row numbers it is another mask
    assert (oracle.dropout_keep(seed, np.arange(len(R2)), 16, p) != oracle.dropout_keep(seed, R2, 16, p)).any()


def test_refusals_that_need_no_device():
    from pygcn_amd import GCN
    from pygcn_amd.sharded import ShardedGraph
    model = GCN(8, 8, 3, dropout=0.5)
    x, idx = torch.randn(6, 8), torch.arange(3)
    dense = torch.eye(6)
    for adj, kw, word in ((dense, dict(rows=None), "rows"), (dense, dict(rows=idx, keep_full=True), "keep_full"),
                          (dense, dict(rows=idx), "CSRGraph"), (dense.to_sparse(), dict(rows=idx), "CSRGraph"),
                          (object.__new__(ShardedGraph), dict(rows=idx), "ShardedGraph")):
        with pytest.raises(RuntimeError, match=word):
            model(x, adj, restrict_forward=True, **kw)
