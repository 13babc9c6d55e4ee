"""Symmetric adjacencies on the device (pygcn_amd/csrc/gcn_symmetric.hip; CSRGraph.sym_normalize_ /
share_transpose), every entry compared with the float64 restatements of tests/_symmetric_ref.py:

  normalisation   D^-1/2 (A + I) D^-1/2 on Cora, on a 1 000-vertex star + ring (a hub row of 999 entries, rows of
                  1 - 3, an empty row) and on 200 000 low-degree rows (past three sweeps of one wave per row):
                  within one float32 ulp of the float64 value, bitwise its own transpose; the zero / negative /
                  NaN rules
  mirror search   positions and the four counts on symmetric, directed, unsorted, duplicated and row-normalised
                  matrices, and the word share_transpose() answers
  the transposes  "pattern": the arrays of the radix sort, on this graph's rowptr / col storage; "self": the graph
  training        the shared routes against the sort route, bitwise, through rows=, a loss over all vertices and
                  the restricted forward pass; the symmetric normalisation against float64
  cache files     the relation survives save -> load
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _symmetric_ref as SR
import inputs as gin
from conftest import ROOT, assert_normwise, load_golden

pytestmark = pytest.mark.gpu

NORM_SWEEP = 16384 * 4        # rows one sweep of the normalisation kernels covers (one wave per row)
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pygcn_amd import _native
    _native.lib()
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_graph(a, b, what):
    assert a.shape == b.shape and a.nnz == b.nnz, what
    for k in ("rowptr", "col", "val"):
        assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), f"{what}: {k} differs"


# ---------------------------------------------------------------- the graphs
def _star_ring_edges():
    """1 000 vertices, built with self_loops=False: hub 0 with 998 spokes and a LISTED self-loop (999 entries), the
    spokes to 1..99 listed twice (weight 2 both ways after the symmetrization); a closed ring on 1..400 (rows of 3),
    a path 401..500 (its ends: rows of 2), 501..998 hub only (rows of 1), 999 isolated (an empty row)."""
    hub = [(0, k) for k in range(1, 999)] + [(0, 0)] + [(0, k) for k in range(1, 100)]
    ring = [(k, k + 1) for k in range(1, 400)] + [(400, 1)]
    path = [(k, k + 1) for k in range(401, 500)]
    return np.array(hub + ring + path, np.int64), 1000


def _low_degree_edges():
    n = 200_000
    rng = np.random.default_rng(3)
    i = np.arange(n)
    chords = np.stack([rng.integers(0, n, n // 2), rng.integers(0, n, n // 2)], 1)
    return np.concatenate([np.stack([i, (i + 1) % n], 1), chords]), n


def _cora_edges():
    z = load_golden("cora_graph.npz")
    return z["edges"].astype(np.int64), int(z["n"])


_EDGES = {"cora": _cora_edges, "star": _star_ring_edges, "low": _low_degree_edges}
_RAW = {}


def _raw(dev, name):
    """(rowptr, col, val, n) of max(A, A^T) [+ I], not normalised, as numpy arrays: built once per module."""
    if name not in _RAW:
        from pygcn_amd import CSRGraph
        edges, n = _EDGES[name]()
        g = CSRGraph.from_edge_list(edges, n, device=dev, normalize=False, self_loops=name != "star")
        _RAW[name] = (g.rowptr.cpu().numpy(), g.col.cpu().numpy(), g.val.cpu().numpy(), n)
    return _RAW[name]


def _graph(dev, arrays, idx64=False):
    from pygcn_amd import CSRGraph
    rowptr, col, val, n = arrays
    return CSRGraph(torch.from_numpy(rowptr.astype(np.int64 if idx64 else np.int32)).to(dev),
                    torch.from_numpy(col.astype(np.int32)).to(dev), torch.from_numpy(val.astype(np.float32)).to(dev),
                    (n, n))


def _clone(g):
    from pygcn_amd import CSRGraph
    return CSRGraph(g.rowptr.clone(), g.col.clone(), g.val.clone(), g.shape)


def test_the_graphs_are_what_the_tests_need(dev):
    from pygcn_amd import _native
    rowptr, col, val, n = _raw(dev, "star")
    length = np.diff(rowptr)
    assert n == 1000 and length[0] == 999 > _native.GCN_DEFAULT_LONG_THRESH and length[999] == 0
    assert {1, 2, 3} <= set(length.tolist()) and set(val.tolist()) == {1.0, 2.0}
    rowptr, col, val, n = _raw(dev, "low")
    assert n == 200_000 > 3 * NORM_SWEEP and np.diff(rowptr).max() < 20 and np.diff(rowptr).min() >= 3
    for name in _EDGES:                                   # the recipe's output: sorted, unique, bitwise symmetric
        assert SR.mirror_ref(*_raw(dev, name)[:3])[1] == (0, 0, 0, 0), name


# ---------------------------------------------------------------- 1. the normalisation
@pytest.mark.parametrize("name", ["cora", "star", "low"])
def test_sym_normalize_is_within_one_ulp_and_bitwise_symmetric(dev, name):
    """Gate: the device value differs from fl32(float64 helper) by the order of a double sum (relative 1e-16) and
    one final rounding, so by at most one float32 ulp, relative 2^-23."""
    raw = _raw(dev, name)
    g = _graph(dev, raw)
    assert g.sym_normalize_() is g
    got = g.val.cpu().numpy()
    ref = SR.sym_normalize_ref(*raw[:3])
    assert np.isfinite(ref).all() and (ref > 0).all()
    worst = float(np.abs(got.astype(np.float64) / ref.astype(np.float32).astype(np.float64) - 1).max())
    print(f"[symmetric] {name}: worst relative distance from fl32(float64) {worst:.3e} (gate 2^-23 = 1.19e-7)")
    ok = SR.within_one_ulp(got, ref)
    assert ok.all(), f"{name}: {int((~ok).sum())} of {ok.size} entries miss one ulp"
    _same_graph(g.t(), g, name + ": the sort-built transpose")           # (g never asked to share: t() sorts)
    assert g.t() is not g
    again = _graph(dev, raw).sym_normalize_()                            # a second run: the same bytes
    assert torch.equal(_bits(again.val), _bits(g.val))
    wide = _graph(dev, raw, idx64=True).sym_normalize_()                 # the int64_t instantiation
    assert wide.rowptr.dtype == torch.int64 and torch.equal(_bits(wide.val), _bits(g.val))
    via = _edge_list_graph(dev, name, "sym")                             # the constructor's spelling
    assert torch.equal(_bits(via.val), _bits(g.val)) and torch.equal(via.col, g.col)


def _edge_list_graph(dev, name, normalize, **kw):
    from pygcn_amd import CSRGraph
    edges, n = _EDGES[name]()
    return CSRGraph.from_edge_list(edges, n, device=dev, normalize=normalize, self_loops=name != "star", **kw)


def test_sym_normalize_zero_negative_and_nan_rules(dev):
    """d = (0, -2, 3, NaN, 6) (tests/test_symmetric_cpu.py computes this case by hand): a zero product gives 0, a
    negative one NaN, the NaN of row 3 reaches row 3 and column 3 and nothing else."""
    rowptr = np.array([0, 2, 4, 8, 10, 12])
    col = np.array([1, 2, 0, 2, 0, 1, 3, 4, 2, 3, 2, 4])
    val = np.array([1, -1, 1, -3, -1, -3, 5, 2, 5, NAN, 2, 4], np.float32)
    got = _graph(dev, (rowptr, col, val, 5)).sym_normalize_().val.cpu().numpy()
    ref = SR.sym_normalize_ref(rowptr, col, val)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).sum() == 5
    assert SR.within_one_ulp(got, ref).all()
    assert (got[[0, 1, 2, 4]] == 0).all() and not np.signbit(got[[0, 1, 2, 4]]).any()
    assert got[7] == got[10] and got[11] == np.float32(4 / 6)            # (sqrt(36) is exact)


def test_a_nan_stays_in_its_row_and_column(dev):
    rowptr, col, val, n = _raw(dev, "star")
    val = val.copy()
    row = SR.row_ids(rowptr)
    e = int(np.flatnonzero((row == 5) & (col == 4))[0])
    val[e] = NAN
    got = _graph(dev, (rowptr, col, val, n)).sym_normalize_().val.cpu().numpy()
    touched = (row == 5) | (col == 5)
    assert touched.sum() == 6 and np.array_equal(np.isnan(got), touched)
    assert SR.within_one_ulp(got, SR.sym_normalize_ref(rowptr, col, val)).all()
    clean = _graph(dev, _raw(dev, "star")).sym_normalize_().val.cpu().numpy()
    far = ~touched & ~np.isin(row, [4, 5, 6]) & ~np.isin(col, [4, 5, 6])
    assert np.array_equal(got[far], clean[far])


# ---------------------------------------------------------------- 2. the mirror search
def _check_mirror(dev, arrays, word, counts=None):
    g = _graph(dev, arrays)
    mirror, got = g._mirror_counts()
    ref_mirror, ref_counts = SR.mirror_ref(*arrays[:3])
    assert tuple(got.tolist()) == ref_counts, (got.tolist(), ref_counts)
    assert counts is None or ref_counts == counts
    assert np.array_equal(mirror[:g.nnz].cpu().numpy().astype(np.int64), ref_mirror)
    assert g.share_transpose() == word
    return g, ref_counts


def test_mirror_counts_on_symmetric_graphs(dev):
    for name in ("cora", "star", "low"):
        g, _ = _check_mirror(dev, _raw(dev, name), "self", (0, 0, 0, 0))
        assert g.t() is g


def test_mirror_counts_on_a_random_directed_graph(dev):
    from pygcn_amd import CSRGraph
    n = 3000
    rng = np.random.default_rng(17)
    edges = rng.integers(0, n, (20_000, 2))
    g = CSRGraph.from_edge_list(edges, n, device=dev, symmetrize=False, self_loops=False, normalize=False)
    arrays = (g.rowptr.cpu().numpy(), g.col.cpu().numpy(), g.val.cpu().numpy(), n)
    p = sp.csr_matrix((np.ones(g.nnz), arrays[1], arrays[0]), shape=(n, n))
    unpaired = int((p - p.multiply(p.T)).count_nonzero())
    assert unpaired > 19_000
    _, counts = _check_mirror(dev, arrays, "sort")
    assert counts[0] == unpaired and counts[2] == 0
    same = g.t()                                          # "sort": nothing changed
    assert same is not g and same.col.data_ptr() != g.col.data_ptr()


def test_mirror_counts_with_one_row_out_of_order(dev):
    rowptr, col, val, n = _raw(dev, "star")
    col, val = col.copy(), val.copy()
    e = rowptr[5]                                         # row 5 stores 0, 4, 6: make it 4, 0, 6
    col[[e, e + 1]], val[[e, e + 1]] = col[[e + 1, e]], val[[e + 1, e]]
    g, counts = _check_mirror(dev, (rowptr, col, val, n), "sort")
    assert counts[2] == 1
    assert g.t().col.data_ptr() != g.col.data_ptr()
    _same_graph(g.t(), _clone(g).t(), "unsorted row: still the sort")


def test_mirror_counts_with_a_duplicate_and_on_hub_rows(dev):
    """The hand-computed directed case of tests/test_symmetric_cpu.py, and the star's 999-entry hub row with the
    searches of 998 other rows landing in it."""
    rowptr, col = np.array([0, 2, 3, 5, 6, 6]), np.array([1, 1, 0, 4, 3, 2])
    _check_mirror(dev, (rowptr, col, np.array([1, 2, 1, 1, 1, 7], np.float32), 5), "sort", (2, 2, 2, 2))
    empty = _graph(dev, (np.zeros(4, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), 3))
    assert empty.share_transpose() == "self"


@pytest.mark.parametrize("name", ["cora", "star", "low"])
def test_mirror_counts_on_row_normalised_graphs(dev, name):
    g = _graph(dev, _raw(dev, name)).row_normalize_()
    arrays = (g.rowptr.cpu().numpy(), g.col.cpu().numpy(), g.val.cpu().numpy(), g.shape[0])
    _, counts = _check_mirror(dev, arrays, "pattern")
    assert counts[:3] == (0, 0, 0) and counts[3] > 0


def test_what_keeps_the_sort(dev):
    from pygcn_amd import CSRGraph
    g = _graph(dev, _raw(dev, "star"), idx64=True)
    assert g.share_transpose() == "sort" and g.t() is not g and g.t().rowptr.dtype == torch.int64
    r = CSRGraph(torch.tensor([0, 1, 2], dtype=torch.int32, device=dev), torch.tensor([0, 2], dtype=torch.int32, device=dev),
                 torch.ones(2, device=dev), (2, 3))
    assert r.share_transpose() == "sort" and r.t().shape == (3, 2)
    with pytest.raises(RuntimeError):
        r.sym_normalize_()


# ---------------------------------------------------------------- 3. "pattern"
@pytest.mark.parametrize("name", ["cora", "star", "low"])
def test_pattern_transpose_is_the_sorted_one_on_shared_storage(dev, name):
    g = _graph(dev, _raw(dev, name)).row_normalize_()
    assert g.share_transpose() == "pattern"
    gt = g.t()
    _same_graph(gt, _clone(g).t(), name + ": shared against sorted")
    assert gt is not g and gt.col.data_ptr() == g.col.data_ptr() and gt.rowptr.data_ptr() == g.rowptr.data_ptr()
    assert gt.val.data_ptr() != g.val.data_ptr() and gt.t() is g and g.t() is gt
    g.plan(), gt.plan()
    assert gt._keep is g._keep and gt.plan().val == gt.val.data_ptr() and g.plan().val == g.val.data_ptr()
    assert gt.plan(torch.bfloat16).items == g.plan(torch.bfloat16).items
    g.val.mul_(2)                                         # an in-place edit: the next t() follows the new values
    after = g.t()
    assert after is not gt and after.col.data_ptr() == g.col.data_ptr()
    _same_graph(after, _clone(g).t(), name + ": after val.mul_(2)")
    assert torch.equal(after.val, gt.val * 2)
    assert _edge_list_graph(dev, name, True, share_transpose=True)._share == "pattern"
    assert _edge_list_graph(dev, name, "row", share_transpose=True)._share == "pattern"


# ---------------------------------------------------------------- 4. "self"
@pytest.mark.parametrize("name", ["cora", "star", "low"])
def test_self_transpose_and_what_ends_it(dev, name):
    g = _edge_list_graph(dev, name, "sym", share_transpose=True)
    assert g._share == "self" and g.t() is g
    _same_graph(g, _clone(g).t(), name + ": the graph against its sorted transpose")
    g.val.mul_(0.5)                                       # still symmetric: verified again, still the graph
    assert g.t() is g
    assert g.row_normalize_() is g
    t = g.t()
    assert t is not g and g._share == "pattern"
    _same_graph(t, _clone(g).t(), name + ": after row_normalize_")


# ---------------------------------------------------------------- 5. / 6. training steps
N_TRAIN, F_TRAIN = 20_000, 256


def _train_graph(dev, normalization):
    from pygcn_amd import CSRGraph
    from pygcn_amd.tuning import ROWGRAD_MIN_ROWS
    from pygcn_amd.utils import rmat_edges
    assert N_TRAIN >= ROWGRAD_MIN_ROWS
    src, dst = rmat_edges(N_TRAIN, 200_000, seed=31)
    return CSRGraph.from_edge_list(torch.stack([src, dst], 1), N_TRAIN, device=dev, normalize=normalization)


def _step(model, x, g, labels, idx, mode):
    model.zero_grad(set_to_none=True)
    torch.manual_seed(11)
    if mode == "all":
        out = model(x, g)
        loss = torch.nn.functional.nll_loss(out, labels)
    else:
        out = model(x, g, rows=idx, restrict_forward=mode == "restricted")
        loss = torch.nn.functional.nll_loss(out, labels[idx])
    loss.backward()
    return out.detach().clone(), [p.grad.clone() for p in model.parameters()]


@pytest.mark.parametrize("normalization,word", [("row", "pattern"), ("sym", "self")])
def test_training_step_is_bitwise_the_sort_route(dev, normalization, word):
    from pygcn_amd import GCN
    base = _train_graph(dev, normalization)
    shared, sorted_ = _clone(base), _clone(base)
    assert shared.share_transpose() == word
    x = torch.from_numpy(gin.dense((N_TRAIN, F_TRAIN), 8)).to(dev)
    labels = torch.from_numpy(np.random.default_rng(5).integers(0, F_TRAIN, N_TRAIN)).to(dev)
    idx = torch.from_numpy(np.random.default_rng(6).permutation(N_TRAIN)[: N_TRAIN // 10]).to(dev)
    torch.manual_seed(7)
    model = GCN(F_TRAIN, F_TRAIN, F_TRAIN, dropout=0.5).to(dev)
    model.train()
    for mode in ("rows", "all", "restricted"):
        a, b = _step(model, x, shared, labels, idx, mode), _step(model, x, sorted_, labels, idx, mode)
        assert torch.equal(a[0], b[0]), f"{normalization} / {mode}: outputs"
        for k, (ga, gb) in enumerate(zip(a[1], b[1])):
            assert torch.equal(ga, gb), f"{normalization} / {mode}: gradient {k}"
        assert float(a[1][0].abs().max()) > 0
    assert (shared.t() is shared) == (word == "self") and sorted_.t().col.data_ptr() != sorted_.col.data_ptr()


@pytest.mark.parametrize("normalization,word", [("row", "pattern"), ("sym", "self")])
def test_cora_step_layer_by_layer_is_bitwise_the_sort_route(dev, normalization, word):
    from pygcn_amd import GCN
    from pygcn_amd.tuning import ROWGRAD_MIN_ROWS
    base = _edge_list_graph(dev, "cora", normalization)
    n = base.shape[0]
    assert n < ROWGRAD_MIN_ROWS
    shared, sorted_ = _clone(base), _clone(base)
    assert shared.share_transpose() == word
    x = torch.from_numpy(gin.cora_features()).to(dev)
    labels = torch.from_numpy(gin.cora_labels()).to(dev)
    idx = torch.arange(140, device=dev)
    torch.manual_seed(7)
    model = GCN(x.shape[1], 16, 7, dropout=0.5).to(dev)
    model.train()
    for mode in ("rows", "all"):
        a, b = _step(model, x, shared, labels, idx, mode), _step(model, x, sorted_, labels, idx, mode)
        assert torch.equal(a[0], b[0])
        assert all(torch.equal(ga, gb) for ga, gb in zip(a[1], b[1]))


def test_sym_normalised_training_step_against_float64(dev):
    """Outputs and the four gradients of one step on the sym-normalised 20 000-vertex graph (shared transpose:
    the graph itself) against the same step in float64 torch ops, at the project's 1e-5 contract.  Dropout is off:
    the float64 evaluation has no mask to share."""
    from pygcn_amd import GCN
    g = _train_graph(dev, "sym")
    assert g.share_transpose() == "self"
    x = torch.from_numpy(gin.dense((N_TRAIN, F_TRAIN), 8)).to(dev)
    labels = torch.from_numpy(np.random.default_rng(5).integers(0, F_TRAIN, N_TRAIN)).to(dev)
    idx = torch.from_numpy(np.random.default_rng(6).permutation(N_TRAIN)[: N_TRAIN // 10]).to(dev)
    torch.manual_seed(7)
    model = GCN(F_TRAIN, F_TRAIN, F_TRAIN, dropout=0.0).to(dev)
    model.train()
    out, grads = _step(model, x, g, labels, idx, "rows")

    row, col, v = g.coo()[0], g.col.long(), g.val.double().unsqueeze(1)

    def prop(b):
        return torch.zeros_like(b).index_add(0, row, b.index_select(0, col) * v)
    w1, b1, w2, b2 = (p.detach().double().requires_grad_() for p in model.parameters())
    assert w1.shape == (F_TRAIN, F_TRAIN) and b1.shape == (F_TRAIN,)
    h = torch.relu(prop(x.double() @ w1) + b1)
    ref = torch.log_softmax(prop(h @ w2) + b2, 1)[idx]
    torch.nn.functional.nll_loss(ref, labels[idx]).backward()
    assert_normwise(out.cpu(), ref.detach().cpu().numpy(), 1e-5, "sym step: output rows")
    for name, got, want in zip(("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias"), grads, (w1, b1, w2, b2)):
        assert_normwise(got.cpu(), want.grad.cpu().numpy(), 1e-5, "sym step: grad " + name)


# ---------------------------------------------------------------- 7. cache files
@pytest.mark.parametrize("normalization,word", [("row", "pattern"), ("sym", "self")])
def test_cache_file_keeps_the_relation(dev, tmp_path, normalization, word):
    from pygcn_amd import CSRGraph, cache
    g = _edge_list_graph(dev, "star", normalization, share_transpose=True)
    assert g._share == word
    path = str(tmp_path / "g.cache")
    g.save(path)
    meta, arr = cache.read_file(path)
    assert meta["share_transpose"] == word and not meta["has_transpose"]
    assert sorted(k for k in arr if k.startswith("t.")) == ([] if word == "self" else ["t.val"])
    for verify in (True, False):
        h = CSRGraph.load(path, device=dev, verify=verify)
        _same_graph(h, g, "loaded")
        assert h._share == word
        if word == "self":
            assert h.t() is h
        else:
            h.t().plan()
            assert h.t().col.data_ptr() == h.col.data_ptr() and h.t().t() is h and h.t()._keep is h._keep
        _same_graph(h.t(), _clone(g).t(), "loaded transpose")
        h.val.mul_(2)                                     # the loaded relation is dropped and verified like any other
        _same_graph(h.t(), _clone(h).t(), "loaded, then edited")
        assert h._share == word


def test_cache_file_of_a_default_graph_is_unchanged(dev, tmp_path):
    from pygcn_amd import CSRGraph, cache
    g = _edge_list_graph(dev, "star", True)
    path = str(tmp_path / "g.cache")
    g.save(path)
    meta, arr = cache.read_file(path)
    assert "share_transpose" not in meta and meta["has_transpose"]
    assert {"t.rowptr", "t.col", "t.val", "t.items"} <= set(arr)
    h = CSRGraph.load(path, device=dev)
    _same_graph(h, g, "loaded")
    _same_graph(h.t(), g.t(), "loaded transpose")
    assert h._share is None and h.t().col.data_ptr() != h.col.data_ptr()


# ---------------------------------------------------------------- the command line
def test_train_script_with_the_new_flags(dev):
    r = subprocess.run([sys.executable, "train.py", "--epochs", "2", "--normalization", "sym", "--share_transpose"],
                       cwd=os.path.join(ROOT, "pygcn_amd"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Epoch: 0002" in r.stdout and "Test set results" in r.stdout
