"""CSRGraph.from_dense on the device (pygcn_amd/csrc/gcn_dense.hip) against the numpy restatement of
tests/_dense_ref.py: row pointer, columns and the BITS of the values, with no tolerance — at the chunk and vector
edges, on pitched and misaligned views, on special values, past one sweep of the grid and one chunk of the select, with
a 64-bit row pointer, on empty input — and its compositions (symmetrize, normalize, share_transpose, save / load, the
layer and a model that takes the fused routes) on a co-visit-like matrix."""
import numpy as np
import pytest
import torch

import _dense_ref as R
import test_select_gpu as S
from conftest import assert_normwise
from test_norm_gpu import DEV, seeded

pytestmark = pytest.mark.gpu

COLS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500)


def convert(A, **kw):
    from pygcn_amd import CSRGraph
    g = CSRGraph.from_dense(A.to(DEV) if isinstance(A, torch.Tensor) else torch.from_numpy(A).to(DEV), **kw)
    torch.cuda.synchronize()
    return g


def reference(A, greater_than=None, keep_per_row=None):
    rule = R.NONZERO if greater_than is None else R.GREATER
    return R.dense_to_csr(A, rule, 0.0 if greater_than is None else greater_than, keep_per_row)


def assert_same(g, ref, shape, what=""):
    rowptr, col, val = ref
    assert g.shape == tuple(shape) and g.nnz == col.size, what
    assert g.col.dtype == torch.int32 and g.val.dtype == torch.float32
    assert torch.equal(g.rowptr.cpu().to(torch.int64), torch.from_numpy(rowptr)), f"{what}: rowptr"
    assert torch.equal(g.col.cpu(), torch.from_numpy(col)), f"{what}: col"
    assert torch.equal(g.val.cpu().view(torch.int32), torch.from_numpy(val).view(torch.int32)), f"{what}: val bits"


def modes(n_cols):
    return [dict(), dict(greater_than=0.25), dict(greater_than=0.25, keep_per_row=5)] + [
        dict(keep_per_row=k) for k in (1, 5, n_cols, n_cols + 7)]


@pytest.mark.parametrize("n_cols", COLS)
def test_column_counts_at_the_chunk_and_vector_edges(n_cols):
    A = R.edge_matrix(n_cols, 500 + n_cols)
    assert not A[2].any() and A[4].all() and A.shape == (7, n_cols)
    for kw in modes(n_cols):
        g = convert(A, **kw)
        assert_same(g, reference(A, **kw), A.shape, f"n_cols {n_cols} {kw}")
        assert g.rowptr.dtype == torch.int32
        if "keep_per_row" in kw:
            assert int((g.rowptr[1:] - g.rowptr[:-1]).max()) <= kw["keep_per_row"]


@pytest.mark.parametrize("view", ["rows_from_3_cols_from_1", "cols_2_to_last"])
def test_pitch_and_alignment(view):
    big = torch.from_numpy(R.edge_matrix(1030, 77, n_rows=40)).to(DEV)
    sub = big[3:, 1:] if view == "rows_from_3_cols_from_1" else big[:, 2:-1]
    assert sub.stride() == (1030, 1) and sub.shape[1] != 1030 and sub.data_ptr() % 16 != 0
    host = sub.cpu().contiguous().numpy()
    for kw in (dict(), dict(greater_than=0.25), dict(keep_per_row=5)):
        g = convert(sub, **kw)
        assert_same(g, reference(host, **kw), host.shape, f"{view} {kw}")
        c = convert(sub.contiguous(), **kw)
        assert torch.equal(g.rowptr, c.rowptr) and torch.equal(g.col, c.col)
        assert torch.equal(g.val.view(torch.int32), c.val.view(torch.int32))


def test_special_values():
    A = R.special_rows()
    g = convert(A)
    assert_same(g, reference(A), A.shape, "default")
    bits = g.val.cpu().view(torch.int32).numpy().view(np.uint32)[:13].tolist()
    assert bits.count(R.NAN_A) == 1 and bits.count(R.NAN_B) == 1                 # NaN kept, payload intact
    assert (g.rowptr[1:] - g.rowptr[:-1]).tolist() == [13, 16, 0, 16]
    for t in (0.0, -1.5, float("inf")):
        g = convert(A, greater_than=t)
        assert_same(g, reference(A, greater_than=t), A.shape, f"greater_than {t}")
        assert not torch.isnan(g.val).any()                                      # NaN dropped
    for k in (1, 2, 3, 5, 8, 13, 15):
        g = convert(A, keep_per_row=k)
        assert_same(g, reference(A, keep_per_row=k), A.shape, f"keep_per_row {k}")
        assert g.col[g.rowptr[1]:g.rowptr[2]].tolist() == list(range(k))         # a row of equal entries: lowest columns
        assert int(g.rowptr[3] - g.rowptr[2]) == 0
    g = convert(A, keep_per_row=3)
    assert g.col[:3].tolist() == [2, 3, 10]                                      # NaN, +inf, NaN: NaN ranks above +inf
    g = convert(A, keep_per_row=3, greater_than=0.0)
    assert g.col[:int(g.rowptr[1])].tolist() == [3]


def test_past_one_grid_sweep_and_one_select_chunk():
    from pygcn_amd import _native
    sweep = _native.GCN_DENSE_SWEEP_ROWS
    n = max(70_000, sweep + 5)
    assert n > sweep and n > 65535
    A = R.tall_matrix(n, 9)
    for kw in (dict(), dict(keep_per_row=3)):
        g = convert(A, **kw)
        ref = reference(A, **kw)
        assert_same(g, ref, A.shape, f"tall {kw}")
        last = min(3, 8) if kw else 8
        assert int(g.rowptr[-1] - g.rowptr[-2]) == last and int(g.rowptr[-2] - g.rowptr[-3]) == 0
        assert g.col[-last:].tolist() == list(range(last))                       # the last row: strictly decreasing
        assert g.col[:int(g.rowptr[1])].tolist() == ref[1][:ref[0][1]].tolist()


def test_int64_row_pointer():
    A = R.edge_matrix(300, 31, n_rows=50)
    for kw in (dict(), dict(keep_per_row=9)):
        small, wide = convert(A, **kw), convert(A, _rowptr_is64=True, **kw)
        assert small.rowptr.dtype == torch.int32 and wide.rowptr.dtype == torch.int64
        assert_same(wide, reference(A, **kw), A.shape, f"int64 {kw}")
        assert torch.equal(wide.rowptr, small.rowptr.to(torch.int64)) and torch.equal(wide.col, small.col)
        assert torch.equal(wide.val.view(torch.int32), small.val.view(torch.int32))


def test_empty_input():
    for A in (np.zeros((0, 5), np.float32), np.zeros((6, 6), np.float32), np.zeros((6, 0), np.float32)):
        for kw in (dict(), dict(keep_per_row=2), dict(greater_than=0.5)):
            g = convert(A, **kw)
            assert g.nnz == 0 and g.shape == A.shape and g.density == 0.0
            assert g.rowptr.tolist() == [0] * (A.shape[0] + 1) and g.col.numel() == 0 and g.val.numel() == 0
            assert torch.equal(g.to_dense(), torch.zeros(A.shape, device=DEV))
    # zeros of both signs are no entries either
    assert convert(R.special_rows()[2:3]).nnz == 0


_COVISIT = {}


def covisit():
    """(A float32 numpy, A on the device, the reference of keep_per_row=16): made once, never written to."""
    if not _COVISIT:
        A = R.covisit_matrix()
        _COVISIT["case"] = (A, torch.from_numpy(A).to(DEV), reference(A, keep_per_row=16))
    return _COVISIT["case"]


def test_round_trip_and_from_torch():
    from pygcn_amd import CSRGraph
    A, dev, _ = covisit()
    g = convert(A)
    assert_same(g, reference(A), A.shape, "covisit")
    assert torch.equal(g.to_dense().view(torch.int32), dev.view(torch.int32))
    assert abs(g.density - 0.22) < 0.02 and g.density == g.nnz / 90000
    t = CSRGraph.from_torch(dev)
    assert torch.equal(t.rowptr, g.rowptr) and torch.equal(t.col, g.col) and torch.equal(t.val, g.val)
    f64 = convert(torch.from_numpy(A.astype(np.float64)))                        # (what np.load gives the fork)
    assert torch.equal(f64.col, g.col) and torch.equal(f64.val, g.val)
    from_host = CSRGraph.from_dense(A.astype(np.float64), device=DEV)
    assert torch.equal(from_host.col, g.col) and torch.equal(from_host.val, g.val)


def test_symmetrize_normalize_share_and_cache(tmp_path):
    from pygcn_amd import CSRGraph
    A, dev, ref = covisit()
    kept = convert(A, keep_per_row=16)
    assert_same(kept, ref, A.shape, "keep 16")
    sym = convert(A, keep_per_row=16, symmetrize=True)
    assert_same(sym, R.symmetrized(*ref, 300), A.shape, "symmetrized")
    pattern = sym.to_dense() != 0
    assert torch.equal(pattern, pattern.t()) and sym.nnz > kept.nnz
    for word, method in ((True, "row_normalize_"), ("row", "row_normalize_"), ("sym", "sym_normalize_")):
        got = convert(A, keep_per_row=16, symmetrize=True, normalize=word)
        want = getattr(convert(A, keep_per_row=16, symmetrize=True), method)()
        assert torch.equal(got.col, want.col) and torch.equal(got.val.view(torch.int32), want.val.view(torch.int32))
        assert not torch.equal(got.val, sym.val)
    shared = convert(A, keep_per_row=16, symmetrize=True, normalize=True, share_transpose=True)
    assert shared._share in ("self", "pattern") and shared.share_transpose() in ("self", "pattern")
    assert convert(A, keep_per_row=16, share_transpose=True)._share is None      # (the cut is not symmetric: a sort)
    with pytest.raises(RuntimeError, match="square"):
        convert(A[:10], symmetrize=True)
    path = str(tmp_path / "covisit.gcn")
    shared.save(path)
    back = CSRGraph.load(path, device=DEV)
    assert back.shape == shared.shape and torch.equal(back.rowptr, shared.rowptr) and torch.equal(back.col, shared.col)
    assert torch.equal(back.val.view(torch.int32), shared.val.view(torch.int32)) and back._share == shared._share


def test_the_layer_on_the_converted_graph():
    """GraphConvolution(16, 32) through the CSR graph of keep_per_row=16, normalize=True against the float64
    evaluation of M·(X·W) + b, M the reference's kept matrix row-normalised in float64.  Gate: assert_normwise at the
    project's 1e-5 (the fp32 evaluation of this case's output on the CPU lies at 1.3e-7 of scale; 6 rows are empty)."""
    from pygcn_amd.layers import GraphConvolution
    A, _, ref = covisit()
    g = convert(A, keep_per_row=16, normalize=True)
    M = R.row_normalized64(R.dense_of(*ref, A.shape))
    torch.manual_seed(11)
    gc = GraphConvolution(16, 32).to(DEV)
    x, cot = seeded((300, 16), 901), seeded((300, 32), 902)
    xd = x.to(DEV).requires_grad_()
    out = gc(xd, g)
    out.backward(cot.to(DEV))
    torch.cuda.synchronize()
    W, b = gc.weight.detach().cpu().double().numpy(), gc.bias.detach().cpu().double().numpy()
    X, G = x.double().numpy(), cot.double().numpy()
    back = M.T @ G
    assert_normwise(out.detach().cpu().numpy(), M @ (X @ W) + b, what="from_dense layer: output")
    assert_normwise(gc.weight.grad.cpu().numpy(), X.T @ back, what="from_dense layer: weight.grad")
    assert_normwise(gc.bias.grad.cpu().numpy(), G.sum(0), what="from_dense layer: bias.grad")
    assert_normwise(xd.grad.cpu().numpy(), back @ W.T, what="from_dense layer: input.grad")


def test_a_model_on_the_converted_graph_takes_the_fused_routes(monkeypatch):
    """One GCN_OVER_MLP step with fused_norm and aggregate_first: on the converted graph both fused nodes run over the
    HIP sparse products; the same matrix passed as a dense tensor reaches neither the aggregate-first node nor a HIP
    product (the default layer's torch.mm branch)."""
    import torch.nn.functional as F
    from pygcn_amd import GCN_OVER_MLP
    A, _, ref = covisit()
    g = convert(A, keep_per_row=16, normalize=True)
    torch.manual_seed(42)
    model = GCN_OVER_MLP(8, 32, 32, 0.0, 3, 32 + 17 - 1 - 8, 16, 8, dim_touched=8, fused_norm=True,
                         aggregate_first=True).to(DEV).train()
    x = seeded((3, 300, 17), 911)
    x[:, :, -1] = (seeded((3, 300), 912) > 0).float()
    x, target = x.to(DEV), seeded((3, 1), 913).to(DEV)
    for adj, fused in ((g, True), (g.to_dense(), False)):
        model.zero_grad()
        spy = S.LaunchSpy(monkeypatch)
        loss = F.mse_loss(model(x, adj), target)
        loss.backward()
        torch.cuda.synchronize()
        names = spy.names()
        assert names.count("gcn_agg_linear_forward") == names.count("gcn_agg_linear_backward") == int(fused)
        if fused:
            assert names.count("gcn_bn_linear_forward") == 2 and "gcn_bn_apply_batched" not in names
        assert any(name.startswith("gcn_spmm_csr") for name in names) == fused      # dense: torch.mm, no HIP product
        assert bool(torch.isfinite(loss)) and model.GCNLayer.gc1.weight.grad is not None
        assert bool(torch.isfinite(model.GCNLayer.gc1.weight.grad).all())


def test_two_conversions_give_the_same_bytes():
    A, _, _ = covisit()
    wide = R.edge_matrix(2500, 41, n_rows=33)
    for M, kw in ((A, dict(keep_per_row=16)), (A, dict()), (wide, dict(keep_per_row=40)), (wide, dict(greater_than=0.25))):
        a, b = convert(M, **kw), convert(M, **kw)
        assert a.val.data_ptr() != b.val.data_ptr()
        assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col, b.col)
        assert torch.equal(a.val.view(torch.int32), b.val.view(torch.int32))
