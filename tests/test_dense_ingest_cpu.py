"""CPU side of the dense adjacency ingest (pygcn_amd/csrc/gcn_dense.hip, CSRGraph.from_dense): the header, the
binding table and the library; every argument check of the two entry points, which run before any launch; the numpy
restatement of tests/_dense_ref.py against torch's own dense -> CSR conversion and on hand-written rows; and the error
of a conversion asked for without a device.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _dense_ref as R
from conftest import ROOT

NAMES = ("gcn_dense_to_csr_count", "gcn_dense_to_csr_fill")
COUNTS = (11, 14)
BADARG, ALIGN = -1, -2


def test_header_table_and_library():
    from pygcn_amd import _native, build
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert re.search(r"#define GCN_ABI_VERSION\s+26\b", hdr) and _native.GCN_ABI_VERSION == 26
    assert _native.lib().gcn_abi_version() == 26                    # additive: the number did not move
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name, count in zip(NAMES, COUNTS):
        assert name in _native.SIGNATURES and name in _native.EXPORTS
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", code)
        assert decl and len(decl.group(1).split(",")) == count == len(_native.SIGNATURES[name][1]), name
        assert hasattr(raw, name) and getattr(_native.lib(), name).argtypes == _native.SIGNATURES[name][1]
        assert _native.SIGNATURES[name][0] is ctypes.c_int
    for name, value in (("GCN_DENSE_NONZERO", 0), ("GCN_DENSE_GREATER", 1)):
        assert int(re.search(rf"#define {name}\s+(\d+)", code).group(1)) == value == getattr(_native, name)
        assert getattr(R, name[len("GCN_DENSE_"):]) == value
    sweep = int(re.search(r"#define GCN_DENSE_SWEEP_ROWS\s+(\d+)", code).group(1))
    assert sweep == _native.GCN_DENSE_SWEEP_ROWS and 1 <= sweep < 70_000
    assert any(src.endswith("gcn_dense.hip") for src in build.SRCS)


# ------------------------------------------------------------------------------------------------ argument checks
P = 0x10000          # a "device address": aligned, never dereferenced — every call below fails its checks or has no rows


def _calls(**over):
    """The two entry points on one set of arguments (valid but for `over`): {name: thunk}."""
    from pygcn_amd import _native
    L = _native.lib()
    a = dict(A=P, lda=12, n_rows=5, n_cols=10, rule=0, bound=0.0, thr=None, count_gt=None, keep=0,
             row_count=P, rowptr=P, is64=0, col=P, val=P)
    a.update(over)
    head = (a["A"], a["lda"], a["n_rows"], a["n_cols"], a["rule"], a["bound"], a["thr"], a["count_gt"], a["keep"])
    return {NAMES[0]: lambda: L.gcn_dense_to_csr_count(*head, a["row_count"], None),
            NAMES[1]: lambda: L.gcn_dense_to_csr_fill(*head, a["rowptr"], a["is64"], a["col"], a["val"], None)}


def _expect(calls, code, only=NAMES):
    from pygcn_amd import _native
    for name in only:
        assert calls[name]() == code, name
        assert _native.lib().gcn_last_error().decode().startswith(name + ":"), _native.lib().gcn_last_error()


@pytest.mark.parametrize("bad", [
    dict(n_rows=-1), dict(n_cols=0), dict(n_cols=-3), dict(n_cols=2 ** 31, lda=2 ** 31), dict(lda=9), dict(rule=2),
    dict(rule=-1), dict(thr=P), dict(thr=P, count_gt=P, keep=0), dict(thr=P, count_gt=P, keep=11),
    dict(thr=P, count_gt=P, keep=-2), dict(A=None)])
def test_bad_arguments_are_refused_before_any_launch(bad):
    _expect(_calls(**bad), BADARG)


def test_null_and_misaligned_arrays():
    _expect(_calls(row_count=None), BADARG, NAMES[:1])
    for name in ("rowptr", "col", "val"):
        _expect(_calls(**{name: None}), BADARG, NAMES[1:])
    for name in ("A", "thr", "count_gt"):
        _expect(_calls(**{"thr": P, "count_gt": P, "keep": 3, name: P + 2}), ALIGN)
    _expect(_calls(row_count=P + 1), ALIGN, NAMES[:1])
    for name in ("rowptr", "col", "val"):
        _expect(_calls(**{name: P + 2}), ALIGN, NAMES[1:])
    _expect(_calls(rowptr=P + 4, is64=1), ALIGN, NAMES[1:])            # an int64 row pointer: 8 bytes
    # the argument rules come first, the pointers after them: a bad size with a bad pointer is a bad size
    _expect(_calls(n_cols=0, A=P + 2), BADARG)


def test_no_rows_launch_nothing():
    for thunk in _calls(n_rows=0).values():
        assert thunk() == 0
    for thunk in _calls(n_rows=0, A=None, row_count=None, rowptr=None, col=None, val=None).values():
        assert thunk() == 0
    _expect(_calls(n_rows=0, n_cols=0), BADARG)                         # (the shape is still checked)


# ------------------------------------------------------------------------------------------------ the restatement
FIXTURES = [R.edge_matrix(n, 100 + n) for n in (1, 5, 65, 257)] + [R.special_rows(), R.tall_matrix(50, 3),
                                                                  R.covisit_matrix(), np.zeros((3, 4), np.float32)]


@pytest.mark.parametrize("A", FIXTURES, ids=lambda a: "x".join(map(str, a.shape)))
def test_the_reference_is_torchs_conversion(A):
    rowptr, col, val = R.dense_to_csr(A)
    want = torch.from_numpy(A).to_sparse_csr()
    assert np.array_equal(rowptr, want.crow_indices().numpy())
    assert np.array_equal(col, want.col_indices().numpy()) and col.dtype == np.int32
    assert np.array_equal(val.view(np.int32), want.values().numpy().view(np.int32)) and val.dtype == np.float32
    assert np.array_equal(R.dense_of(rowptr, col, val, A.shape).view(np.int32),
                          np.where(A == 0, np.float32(0), A).view(np.int32))


def _cols(row, **kw):
    rowptr, col, _ = R.dense_to_csr(np.array([row], np.float32), **kw)
    assert rowptr.tolist() == [0, col.size]
    return col.tolist()


def test_keep_rule_on_hand_written_rows():
    row = [3, 1, 3, 3, 0, 2]
    assert _cols(row, keep=2) == [0, 2]                                # ties at the threshold: the lowest columns
    assert _cols(row, keep=4) == [0, 2, 3, 5]
    assert _cols(row, keep=6) == _cols(row, keep=9) == _cols(row) == [0, 1, 2, 3, 5]
    assert _cols([7, 7, 7, 7, 7], keep=3) == [0, 1, 2]
    assert _cols([0, 0, 5, 0], keep=3) == [2]                          # fewer non-zeros than keep: just those
    nan = float("nan")
    assert _cols([1, nan, 9, 0], keep=1) == [1]                        # NaN ranks above everything and is kept ...
    assert _cols([1, nan, 9, 0], keep=2) == [1, 2]
    assert _cols([1, nan, 9, 0], rule=R.GREATER, bound=0.0, keep=1) == []          # ... but is not greater than t
    assert _cols([1, nan, 9, 0], rule=R.GREATER, bound=0.0, keep=2) == [2]
    assert _cols([1, nan, 9, 0], rule=R.GREATER, bound=0.0) == [0, 2]
    assert _cols([-0.0, 0.0, -1, 2], keep=3) == [3]                    # both zeros selected (-0 is +0), both dropped
    assert _cols([-0.0, 0.0, -1, 2], keep=4) == [2, 3]


def test_special_rows_and_the_union():
    A = R.special_rows()
    rowptr, col, val = R.dense_to_csr(A)
    assert np.diff(rowptr).tolist() == [13, 16, 0, 16]
    first = val[:13].view(np.uint32).tolist()
    assert R.NAN_A in first and R.NAN_B in first                       # the payloads survive
    assert np.diff(R.dense_to_csr(A, R.GREATER, 0.0)[0]).tolist() == [7, 16, 0, 0]
    assert R.dense_to_csr(A, keep=3)[1][:3].tolist() == [2, 3, 10]     # NaN, +inf, NaN
    cov = R.covisit_matrix()
    assert np.array_equal(cov, cov.T) and abs((cov != 0).mean() - 0.22) < 0.02
    rp, c, v = R.dense_to_csr(cov, keep=16)
    assert np.diff(rp).max() == 16
    srp, sc, sv = R.symmetrized(rp, c, v, 300)
    S = R.dense_of(srp, sc, sv, (300, 300))
    K = R.dense_of(rp, c, v, (300, 300))
    assert np.array_equal(S, np.maximum(K, K.T)) and not np.array_equal(K, K.T)
    assert np.all(np.diff(srp) >= np.diff(rp))


def test_without_a_device():
    from pygcn_amd import CSRGraph
    with pytest.raises(RuntimeError, match="must live on a HIP device"):
        CSRGraph.from_dense(torch.rand(4, 4))
    with pytest.raises(RuntimeError, match="must live on a HIP device"):
        CSRGraph.from_dense(np.eye(3))                                 # (a float64 array, as np.load gives)
    with pytest.raises(RuntimeError, match="must live on a HIP device"):
        CSRGraph.from_torch(torch.rand(4, 4))
    with pytest.raises(RuntimeError, match="2-D"):
        CSRGraph.from_dense(torch.rand(4))
    with pytest.raises(RuntimeError, match="normalize"):
        CSRGraph.from_dense(torch.rand(4, 4), normalize="both")
