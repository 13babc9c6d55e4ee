"""What the symmetric-adjacency feature (pygcn_amd/csrc/gcn_symmetric.hip, CSRGraph.sym_normalize_ /
share_transpose) rests on that needs no GPU: the float64 helper of tests/_symmetric_ref.py on hand-computed cases,
the scipy host twin `utils.normalize_sym`, the new command-line flags, and the new C-ABI symbols."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import _symmetric_ref as SR
from conftest import ROOT, load_golden
from pygcn_amd import _native

NEW = ("gcn_sym_normalize_workspace_bytes", "gcn_sym_normalize_device", "gcn_csr_mirror_device", "gcn_gather_f32")
NAN = float("nan")


# ---------------------------------------------------------------- the helper, by hand
def test_helper_on_a_path_with_self_loops():
    """A + I of the path 0 - 1 - 2 and an isolated vertex 3: d = (2, 3, 2, 1)."""
    rowptr, col = [0, 2, 5, 7, 8], [0, 1, 0, 1, 2, 1, 2, 3]
    val = np.ones(8, np.float32)
    r6 = 1 / np.sqrt(6.0)
    np.testing.assert_allclose(SR.sym_normalize_ref(rowptr, col, val), [0.5, r6, r6, 1 / 3, r6, r6, 0.5, 1.0],
                               rtol=1e-15)
    mirror, counts = SR.mirror_ref(rowptr, col, val)
    assert mirror.tolist() == [0, 2, 1, 3, 5, 4, 6, 7] and counts == (0, 0, 0, 0)


def test_helper_on_the_rows_that_do_not_simply_divide():
    """5 vertices with bitwise symmetric weights: d = (0, -2, 3, NaN, 6).  A zero product gives 0, a negative one
    NaN, the NaN of row 3 reaches row 3 and column 3 only."""
    rowptr = [0, 2, 4, 8, 10, 12]
    col = [1, 2, 0, 2, 0, 1, 3, 4, 2, 3, 2, 4]
    val = np.array([1, -1, 1, -3, -1, -3, 5, 2, 5, NAN, 2, 4], np.float32)
    got = SR.sym_normalize_ref(rowptr, col, val)
    r18 = 2 / np.sqrt(18.0)
    want = [0, 0, 0, NAN, 0, NAN, NAN, r18, NAN, NAN, r18, 4 / 6]
    np.testing.assert_allclose(got, want, rtol=1e-15, equal_nan=True)
    mirror, counts = SR.mirror_ref(rowptr, col, val)
    assert mirror.tolist() == [2, 4, 0, 5, 1, 3, 8, 10, 6, 9, 7, 11]
    assert counts == (0, 0, 0, 0)                       # (the NaN is its own mirror: the same bits)
    val[4] = -1.0000001                                 # one ulp away from its mirror (0, 2)
    assert SR.mirror_ref(rowptr, col, val)[1] == (0, 0, 0, 2)


def test_helper_on_a_directed_matrix_with_a_duplicate_and_an_unsorted_row():
    """Row 0 stores (0, 1) twice, row 2 stores its columns as 4, 3, vertex 4 has no row entries."""
    rowptr, col = [0, 2, 3, 5, 6, 6], [1, 1, 0, 4, 3, 2]
    val = np.array([1, 2, 1, 1, 1, 7], np.float32)
    mirror, counts = SR.mirror_ref(rowptr, col, val)
    assert mirror.tolist() == [2, 2, 0, -1, 5, -1]
    # no mirror: (2, 4) and (3, 2) [row 2 is not sorted: the search misses its 3]; mirror of mirror: the second
    # (0, 1) and (2, 3); not increasing: the second (0, 1) and the 3 after the 4; value: 2 vs 1 and 1 vs 7
    assert counts == (2, 2, 2, 2)


def test_one_ulp_gate_of_the_helper():
    ref = np.array([1.0, 1.0 + 2.0 ** -24 * 0.999, 3.0, 0.0, NAN, 1e-3])
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2))
    assert SR.within_one_ulp(np.array([one, one, 3, 0, NAN, 1e-3], np.float32), ref).all()
    assert SR.within_one_ulp(np.array([up, up, 3, 0, NAN, 1e-3], np.float32), ref).all()
    two_up = np.nextafter(up, np.float32(2))
    bad = SR.within_one_ulp(np.array([two_up, one, 3, 1e-30, 1, NAN], np.float32), ref)
    assert bad.tolist() == [False, True, True, False, False, False]


# ---------------------------------------------------------------- the host twin
def _cora_plus_identity():
    z = load_golden("cora_graph.npz")
    edges, n = z["edges"].astype(np.int64), int(z["n"])
    adj = sp.coo_matrix((np.ones(edges.shape[0]), (edges[:, 0], edges[:, 1])), shape=(n, n)).tocsr()
    adj = adj.maximum(adj.T) + sp.eye(n)
    adj = sp.csr_matrix(adj)
    adj.sort_indices()
    return adj


def test_normalize_sym_is_the_float64_formula_on_cora():
    from pygcn_amd.utils import normalize, normalize_sym
    adj = _cora_plus_identity()
    got = sp.csr_matrix(normalize_sym(adj))
    got.sort_indices()
    assert np.array_equal(got.indptr, adj.indptr) and np.array_equal(got.indices, adj.indices)
    want = SR.sym_normalize_ref(adj.indptr, adj.indices, adj.data)
    # (d^-1/2 · w) · d^-1/2 against w / sqrt(d · d): a few float64 roundings apart
    np.testing.assert_allclose(got.data, want, rtol=8 * 2.0 ** -53, atol=0)
    assert abs(got - got.T).max() <= 2.0 ** -52 and abs(got - sp.csr_matrix(normalize(adj))).max() > 0.1
    # a zero row stays zero (`d_inv_sqrt[isinf] = 0`)
    m = sp.csr_matrix(np.array([[0, 0, 0], [0, 1, 3.0], [0, 3, 1]]))
    np.testing.assert_allclose(normalize_sym(m).toarray(), [[0, 0, 0], [0, .25, .75], [0, .75, .25]], rtol=1e-15)


def test_load_data_takes_the_normalisation():
    from pygcn_amd.utils import load_data
    adj = _cora_plus_identity()
    sym = load_data(normalization="sym")[0].coalesce()
    want = sp.coo_matrix(adj)
    order = np.lexsort((want.col, want.row))
    assert np.array_equal(sym.indices()[0].numpy(), want.row[order])
    assert np.array_equal(sym.indices()[1].numpy(), want.col[order])
    ref = SR.sym_normalize_ref(adj.indptr, adj.indices, adj.data)
    np.testing.assert_allclose(sym.values().numpy(), ref.astype(np.float32), rtol=2.0 ** -23, atol=0)
    with pytest.raises(ValueError):
        load_data(normalization="column")


# ---------------------------------------------------------------- the command line
def test_train_parser_takes_the_new_flags():
    code = ("import train; a = train.parser.parse_args(['--normalization', 'sym', '--share_transpose']); "
            "b = train.parser.parse_args([]); print(a.normalization, a.share_transpose, b.normalization, "
            "b.share_transpose)\n"
            "try:\n    train.parser.parse_args(['--normalization', 'column'])\n"
            "except SystemExit as e:\n    print('refused', e.code)")
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(ROOT, "pygcn_amd"), capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split("\n")[:2] == ["sym True row False", "refused 2"], out.stdout


# ---------------------------------------------------------------- the C-ABI
def test_header_tables_and_library_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert int(re.search(r"#define GCN_ABI_VERSION\s+(\d+)", hdr).group(1)) == _native.GCN_ABI_VERSION == 26
    L = _native.lib()
    assert L.gcn_abi_version() == 26
    for name in NEW:
        assert name in _native.SIGNATURES and name in _native.EXPORTS
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl and len(decl.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name
        assert getattr(L, name).argtypes == _native.SIGNATURES[name][1]
    from pygcn_amd import build
    assert any(os.path.basename(s) == "gcn_symmetric.hip" for s in build.SRCS)


def test_argument_errors_are_reported_before_any_launch():
    """Checked on the host, so no device is needed (the pointers are never dereferenced)."""
    L = _native.lib()
    h = 4096
    assert L.gcn_sym_normalize_workspace_bytes(1000) >= 8000 and L.gcn_sym_normalize_workspace_bytes(0) > 0
    assert L.gcn_sym_normalize_device(h, 0, h, h, 0, None, 0, None) == 0            # no rows: nothing to do
    assert L.gcn_sym_normalize_device(None, 0, h, h, 4, h, 4096, None) == -1
    assert L.gcn_sym_normalize_device(h, 0, h, h, -1, h, 4096, None) == -1
    assert L.gcn_sym_normalize_device(h, 0, h, h, 1000, h, 7999, None) == -3         # short workspace
    assert L.gcn_sym_normalize_device(h, 0, h, h, 1000, None, 8192, None) == -3
    assert b"gcn_sym_normalize_device" in L.gcn_last_error()
    assert L.gcn_csr_mirror_device(h, h, h, 4, 2 ** 31, h, h, None) == -1           # 32-bit positions only
    assert L.gcn_csr_mirror_device(h, h, h, 4, 8, h, None, None) == -1
    assert L.gcn_csr_mirror_device(h, h, h, 4, 8, None, h, None) == -1
    assert b"gcn_csr_mirror_device" in L.gcn_last_error()
    assert L.gcn_gather_f32(h, h, 0, 0, h, None) == 0
    assert L.gcn_gather_f32(h, h, -1, 0, h, None) == -1 and L.gcn_gather_f32(h, None, 8, 8, h, None) == -1
