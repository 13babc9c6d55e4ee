"""Everything that hangs on a graph's VALUES follows an in-place edit of them ("What hangs on a
graph's values"): `CSRGraph.val` may be edited with torch ops (`val.mul_`, an optimizer step on learned edge
weights) or by the native editors `row_normalize_()` / `sym_normalize_()`, and the next step must be the step of
a handle that never saw the old values.

The judge has two parts:

  (a) bitwise   a training step on the edited handle is `torch.equal` to the same step (same parameters, same
                generator seed) on `fresh(g)`, a CSRGraph built on clones of the edited arrays: the kernels are
                deterministic and both handles take the same route, so no tolerance is involved;
  (b) reference once per route, the edited step against the oracle's step and its float64 twin on the edited
                arrays, at the gates of tests/test_fused_gpu.py::_check (restated in `_against_reference`).

No test can pass vacuously: before judging, the oracle's step on the arrays before and after the edit (the edit
restated on the host, `_edit_host`) must differ by at least MOVED = 1e-2 of the max-norm in every compared
quantity — a condition on the inputs, computed from the reference alone.  The 256-wide cases run with dropout
0.5, which the oracle does not have: their condition is the oracle's dropout-free step, and they are judged
bitwise only.

Each route takes one step before the edit, so that every cache is full of the old values."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import inputs as gin
from conftest import assert_normwise, assert_parity

pytestmark = pytest.mark.gpu
TOL = 1e-5
MOVED = 1e-2
EDITORS = ("mul", "row", "sym")
NARROW, WIDE = (48, 64, 16), (256, 256, 256)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ---------------------------------------------------------------- graphs, editors, the fresh handle
def _arrays(n, edges, seed, editor):
    """CSR arrays (rowptr int64, col int32, val float32; numpy) of the graph BEFORE the edit.  "mul": the
    row-normalised R-MAT graph.  "row" / "sym": its pattern made symmetric, with bitwise symmetric raw weights
    uniform in (0, 1]·2⁻¹⁰ — row sums far below 1 (the hub's: 0.39), so an ∞-norm of before the normalisation
    is too small, for most rows about 2¹⁰ times."""
    from pygcn_amd.utils import rmat_graph
    rowptr, col, val = (t.numpy() for t in rmat_graph(n, edges, seed=seed, device="cpu"))
    if editor == "mul":
        return rowptr.astype(np.int64), col.astype(np.int32), val.astype(np.float32)
    a = sp.csr_matrix((np.ones(len(col), np.float32), col, rowptr), shape=(n, n))
    upper = sp.triu(a + a.T).tocoo()
    w = ((1.0 - np.random.default_rng(seed + 1).random(upper.nnz)) * 2.0 ** -10).astype(np.float32)
    upper = sp.coo_matrix((w, (upper.row, upper.col)), shape=(n, n))
    full = (upper + sp.triu(upper, 1).T).tocsr()
    full.sort_indices()
    return full.indptr.astype(np.int64), full.indices.astype(np.int32), full.data.astype(np.float32)


def _mul_weights(nnz):
    return (0.25 + 1.5 * np.random.default_rng(nnz).random(nnz)).astype(np.float32)


def _edit_host(editor, rowptr, col, val):
    """The editor restated on the host (float64, rounded once): the values after the edit."""
    if editor == "mul":
        return val * _mul_weights(len(val))
    d = np.add.reduceat(np.append(val.astype(np.float64), 0.0), rowptr[:-1])
    d[np.diff(rowptr) == 0] = 0.0
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    if editor == "row":
        return (val / d[row]).astype(np.float32)
    return (val / np.sqrt(d[row] * d[col])).astype(np.float32)


def _edit(editor, g):
    if editor == "mul":
        g.val.mul_(torch.from_numpy(_mul_weights(g.nnz)).to(g.device))
    elif editor == "row":
        g.row_normalize_()
    else:
        g.sym_normalize_()


def _graph(dev, arrays):
    from pygcn_amd import CSRGraph
    rowptr, col, val = arrays
    n = len(rowptr) - 1
    return CSRGraph(torch.from_numpy(rowptr.astype(np.int32)).to(dev), torch.from_numpy(col).to(dev),
                    torch.from_numpy(val).to(dev), (n, n))


def fresh(g):
    """A handle with no history, on clones of g's arrays as they are now."""
    from pygcn_amd import CSRGraph
    return CSRGraph(g.rowptr.clone(), g.col.clone(), g.val.detach().clone(), g.shape, item_cost=g.item_cost,
                    long_thresh=g.long_thresh)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ---------------------------------------------------------------- the reference and the two judges
def _oracle_step(oracle, arrays, x, p, labels, idx, need_x=False, f64=False):
    """{name: array} of the oracle's step: the selected rows, the loss, the parameter gradients, grad_x; with
    `f64` also its float64 twin's gradients (given the float32 oracle's ReLU pattern, as _check does)."""
    n = len(arrays[0]) - 1
    a = oracle.CSR(arrays[0], arrays[1], arrays[2], (n, n))
    loss, fw, grads, extra = oracle.gcn2_loss_backward(x, a, p, labels, idx, need_grad_x=need_x)
    ref = {"rows": fw["logp"][idx], "loss": np.array([loss])}
    ref.update({k + ".grad": v for k, v in grads.items()})
    if need_x:
        ref["x.grad"] = extra["grad_x"]
    if f64:
        ref["f64"] = oracle.gcn2_loss_backward_f64(x, a, p, labels, idx, relu_mask=fw["h1"] > 0)[2]
    return ref


def _assert_moved(before, after):
    """The condition on the inputs: the edit moves every compared quantity of the REFERENCE by MOVED of its norm."""
    for k, v in after.items():
        if k == "f64":
            continue
        moved, scale = float(np.abs(v - before[k]).max()), float(np.abs(v).max())
        assert moved >= MOVED * scale, f"the edit moves the reference's {k} by {moved:.3e} of {scale:.3e} only"


def _assert_bitwise(got, want, what):
    assert got.keys() == want.keys()
    for k in got:
        assert torch.isfinite(got[k]).all(), f"{what}: {k} is not finite"
        assert torch.equal(got[k], want[k]), \
            f"{what}: {k} differs from the fresh handle's, max|d| = {float((got[k] - want[k]).abs().max()):.3e}"


def _against_reference(got, ref):
    """tests/test_fused_gpu.py::_check, its gates unchanged."""
    assert_normwise(got["rows"].cpu(), ref["rows"], TOL, "selected rows")
    assert abs(got["loss"].item() - ref["loss"][0]) <= TOL * abs(ref["loss"][0])
    for k, v64 in ref["f64"].items():
        assert_parity(got[k + ".grad"].cpu(), ref[k + ".grad"], v64, k + ".grad")
    if "x.grad" in ref:
        assert_normwise(got["x.grad"].cpu(), ref["x.grad"], TOL, "grad_x")


# ---------------------------------------------------------------- the routes
def _rows(model, x, g, idx):
    return model(x, g, rows=idx)


def _rowgrad(model, x, g, idx):
    out = model(x, g)
    from pygcn_amd.rowgrad import RowSelectable
    assert isinstance(out, RowSelectable)
    return out[idx]


def _restricted(model, x, g, idx):
    return model(x, g, rows=idx, restrict_forward=True)


def _layers(model, x, g, idx):
    """Bare layers composed by hand, each its own node (GraphConvFunction._backward_rows): the way in of
    tests/test_fused_gpu.py::test_upstream_lines_take_the_row_sparse_route."""
    from pygcn_amd.rowgrad import RowSelectable
    h = model.gc1(x, g, relu=True, dropout=model.dropout if model.training else 0.0)
    return model.gc2(h, g, log_softmax=True).as_subclass(RowSelectable)[idx]


ROUTES = {"rows": _rows, "rowgrad": _rowgrad, "restricted": _restricted, "layers": _layers}


def _forward(route, model, x, g, idx, y):
    torch.manual_seed(11)                     # (the dropout seed is drawn from the generator)
    out = ROUTES[route](model, x, g, idx)
    return out, torch.nn.functional.nll_loss(out, y)


def _step(route, model, x, g, idx, y):
    model.zero_grad(set_to_none=True)
    x.grad = None
    out, loss = _forward(route, model, x, g, idx, y)
    loss.backward()
    got = {"rows": out.detach().as_subclass(torch.Tensor).clone(), "loss": loss.detach().as_subclass(torch.Tensor).clone()}
    got.update({k + ".grad": p.grad.clone() for k, p in model.named_parameters()})
    if x.requires_grad:
        got["x.grad"] = x.grad.clone()
    return got


class _Case:
    """One graph of its own, its inputs, a model, and the oracle's step before and after the edit."""

    def __init__(self, oracle, dev, editor, widths, n, edges, dropout=0.0, need_x=False, seed=5):
        from pygcn_amd import GCN
        fin, hid, ncls = widths
        self.editor, self.need_x, self.oracle = editor, need_x, oracle
        self.arrays = _arrays(n, edges, seed, editor)
        self.g = _graph(dev, self.arrays)
        rng = np.random.default_rng(seed + fin)
        self.x_np = gin.dense((n, fin), seed + 1)
        self.labels = rng.integers(0, ncls, n)
        self.idx_np = rng.permutation(n)[: int(0.3 * n)]                     # unsorted
        self.x = torch.from_numpy(self.x_np).to(dev).requires_grad_(need_x)
        self.idx = torch.from_numpy(self.idx_np).to(dev)
        self.y = torch.from_numpy(self.labels).to(dev)[self.idx]
        torch.manual_seed(seed)
        self.model = GCN(fin, hid, ncls, dropout=dropout).to(dev)
        self.model.train()
        self.p = {k: v.detach().cpu().numpy() for k, v in self.model.state_dict().items()}

    def reference(self, arrays, f64=False):
        return _oracle_step(self.oracle, arrays, self.x_np, self.p, self.labels, self.idx_np, self.need_x, f64)

    def assert_the_edit_matters(self):
        rowptr, col, val = self.arrays
        _assert_moved(self.reference(self.arrays), self.reference((rowptr, col, _edit_host(self.editor, *self.arrays))))

    def judge(self, route, against_reference):
        """One step (the caches fill), the edit, then the step that is judged."""
        first = _step(route, self.model, self.x, self.g, self.idx, self.y)
        assert all(torch.isfinite(v).all() for v in first.values())
        self.assert_the_edit_matters()
        _edit(self.editor, self.g)
        got = _step(route, self.model, self.x, self.g, self.idx, self.y)
        want = _step(route, copy.deepcopy(self.model), self.x, fresh(self.g), self.idx, self.y)
        _assert_bitwise(got, want, f"{route} after {self.editor}")
        if against_reference:
            edited = (self.arrays[0], self.arrays[1], self.g.val.cpu().numpy())
            _against_reference(got, self.reference(edited, f64=True))
        return got


@pytest.mark.parametrize("editor", EDITORS)
@pytest.mark.parametrize("need_x", [False, True])
def test_rows_route_follows_the_edit(oracle, dev, editor, need_x):
    """`model(x, g, rows=idx)`: RowSets.at_block is the layer-2 operand of the backward pass."""
    _Case(oracle, dev, editor, NARROW, 3000, 30000, need_x=need_x).judge("rows", against_reference=True)


@pytest.mark.parametrize("editor", EDITORS)
def test_rows_route_follows_the_edit_at_256(oracle, dev, editor, gemm_scheme):
    """256 -> 256 -> 256 with dropout 0.5: the packed layer 2, the hand-written GEMMs and, under "h2", the
    bounds that graph.inf_norm() feeds."""
    _Case(oracle, dev, editor, WIDE, 3000, 30000, dropout=0.5).judge("rows", against_reference=False)


@pytest.mark.parametrize("editor", EDITORS)
def test_upstream_lines_follow_the_edit(oracle, dev, editor):
    """`model(x, g)[idx]`: the model's one node under a RowGrad, at the least height that returns a RowSelectable."""
    from pygcn_amd.tuning import ROWGRAD_MIN_ROWS
    _Case(oracle, dev, editor, NARROW, ROWGRAD_MIN_ROWS, 160000).judge("rowgrad", against_reference=True)


def _layer_route(oracle, dev, editor, widths, monkeypatch):
    from pygcn_amd import spmm as S
    taken = []
    real = S.GraphConvFunction._backward_rows
    monkeypatch.setattr(S.GraphConvFunction, "_backward_rows",
                        staticmethod(lambda ctx, grad: (lambda r: (taken.append(r is not None), r)[1])(real(ctx, grad))))
    case = _Case(oracle, dev, editor, widths, 3000, 30000, dropout=0.0 if widths == NARROW else 0.5)
    case.judge("layers", against_reference=widths == NARROW)
    assert taken[0::2] == [True] * 3, taken         # (three steps: the last layer took the row route every time)


@pytest.mark.parametrize("editor", EDITORS)
def test_layer_route_follows_the_edit(oracle, dev, editor, monkeypatch):
    """GraphConvFunction._backward_rows, bare layers composed by hand: the last layer's at_block."""
    _layer_route(oracle, dev, editor, NARROW, monkeypatch)


@pytest.mark.parametrize("editor", EDITORS)
def test_layer_route_follows_the_edit_at_256(oracle, dev, editor, gemm_scheme, monkeypatch):
    """... and at 256 -> 256 -> 256 the bound of its GEMMs from graph.t().inf_norm(), the first layer on the
    compact rows of the RowGrad it is handed."""
    _layer_route(oracle, dev, editor, WIDE, monkeypatch)


@pytest.mark.parametrize("editor", EDITORS)
def test_restricted_route_follows_the_edit(oracle, dev, editor):
    """`restrict_forward=True`: the blocks Â[R2,:] and Â[R,R2] of RowSets.restricted() in the forward pass too."""
    _Case(oracle, dev, editor, NARROW, 3000, 30000).judge("restricted", against_reference=True)


@pytest.mark.parametrize("editor", EDITORS)
@pytest.mark.parametrize("cache", [False, True])
def test_restricted_route_follows_the_edit_at_256(oracle, dev, editor, cache, gemm_scheme):
    """... and with the input-product cache the compact Â[R2,:]·X that hangs on the row sets."""
    from pygcn_amd import fused
    case = _Case(oracle, dev, editor, WIDE, 3000, 30000, dropout=0.5)
    fused.set_input_product_cache(cache)
    try:
        case.judge("restricted", against_reference=False)
    finally:
        fused.set_input_product_cache(False)


@pytest.mark.parametrize("editor", EDITORS)
def test_cached_input_product_follows_the_edit(oracle, dev, editor):
    """`model(x, g, rows=idx)` with set_input_product_cache(True): Â·X hangs on the graph.  The step after the
    edit is the fresh handle's, and it holds exactly one forward product more than a cached step."""
    from pygcn_amd import fused
    from pygcn_amd import spmm as S
    case = _Case(oracle, dev, editor, WIDE, 3000, 30000)
    launches = []
    fused.set_input_product_cache(True)
    try:
        _step("rows", case.model, case.x, case.g, case.idx, case.y)          # (fills the cache)
        S.set_timing_records(launches)
        _step("rows", case.model, case.x, case.g, case.idx, case.y)
        cached = sum(1 for r in launches if r[0] == "fwd")
        S.set_timing_records(None)
        case.judge("rows", against_reference=False)                          # one more cached step, the edit, ...
        S.set_timing_records(launches)
        del launches[:]
        _step("rows", case.model, case.x, case.g, case.idx, case.y)          # ... and it is cached again
        again = sum(1 for r in launches if r[0] == "fwd")
        del launches[:]
        _edit(editor, case.g)                                                # a second edit
        _step("rows", case.model, case.x, case.g, case.idx, case.y)
        edited = sum(1 for r in launches if r[0] == "fwd")
    finally:
        S.set_timing_records(None)
        fused.set_input_product_cache(False)
    assert cached == again == 1 and edited == cached + 1


# ---------------------------------------------------------------- an edit between forward and backward
@pytest.mark.parametrize("editor", ["mul", "row"])
@pytest.mark.parametrize("route", ["rows", "restricted", "layers"])
def test_an_edit_between_forward_and_backward_raises(oracle, dev, editor, route):
    """ctx.graph is no saved tensor: the nodes keep the version of its values themselves."""
    case = _Case(oracle, dev, editor, NARROW, 3000, 30000)
    _step(route, case.model, case.x, case.g, case.idx, case.y)               # no edit: no error
    _, loss = _forward(route, case.model, case.x, case.g, case.idx, case.y)
    _edit(editor, case.g)
    with pytest.raises(RuntimeError, match=r"CSRGraph\(shape=\(3000, 3000\).*modified by an inplace operation"):
        loss.backward()
    _step(route, case.model, case.x, case.g, case.idx, case.y)               # the next whole step is fine


# ---------------------------------------------------------------- the handle's own state
@pytest.mark.parametrize("editor,shared", [("mul", None), ("row", None), ("sym", None), ("row", "pattern"),
                                           ("sym", "self")])
def test_the_handle_follows_the_edit(dev, editor, shared, tmp_path):
    """inf_norm(), t() (sorted, or shared as "pattern" / "self"), the schedules, and a cache file written after
    the edit — bitwise those of a fresh handle."""
    from pygcn_amd import CSRGraph
    arrays = _arrays(3000, 30000, 7, editor)
    g = _graph(dev, arrays)
    if shared:
        assert g.share_transpose() == "self"                                 # (the raw weights are symmetric)
    norm_before, t_before = g.inf_norm().clone(), g.t()
    t_before.inf_norm()
    plan, plan16, stats16 = g.plan(), g.plan(torch.bfloat16), g.schedule_stats(torch.bfloat16)
    # the condition on the inputs: the ∞-norm moves (float64, on the host)
    sums = [np.add.reduceat(np.append(np.abs(v).astype(np.float64), 0.0), arrays[0][:-1]).max()
            for v in (arrays[2], _edit_host(editor, *arrays))]
    assert abs(sums[1] - sums[0]) >= MOVED * sums[1]
    _edit(editor, g)
    f = fresh(g)
    if shared:
        assert f.share_transpose() == shared
    assert torch.equal(_bits(g.inf_norm()), _bits(f.inf_norm()))
    assert abs(float(g.inf_norm()) - sums[1]) <= 1e-4 * sums[1] and not torch.equal(g.inf_norm(), norm_before)
    gt, ft = g.t(), f.t()
    assert g._share == f._share == shared and (gt is g) == (shared == "self")
    for k in ("rowptr", "col", "val"):
        assert torch.equal(_bits(getattr(gt, k)), _bits(getattr(ft, k))), f"t().{k}"
    if shared == "pattern":
        assert gt.rowptr.data_ptr() == g.rowptr.data_ptr() and gt.col.data_ptr() == g.col.data_ptr()
    assert torch.equal(_bits(gt.inf_norm()), _bits(ft.inf_norm()))
    # the schedules hang on the pattern alone: the same objects, on the same (edited) array
    assert g.plan() is plan and g.plan(torch.bfloat16) is plan16 and plan.val == plan16.val == g.val.data_ptr()
    assert g.schedule_stats(torch.bfloat16) == stats16 == f.schedule_stats(torch.bfloat16)
    assert g.schedule_stats() == f.schedule_stats()
    path = str(tmp_path / "edited.gcn")
    g.save(path)
    h = CSRGraph.load(path, device=dev, verify=True)
    assert h._share == shared
    for a, b in ((h, g), (h.t(), gt)):
        for k in ("rowptr", "col", "val"):
            assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), f"after save / load: {k}"


# ---------------------------------------------------------------- learned edge weights
def test_learned_edge_weights_follow_the_optimizer(dev):
    """`val` as a leaf of `torch.ops.pygcn_amd.spmm_csr` (grad_val through gcn_sddmm_csr): an SGD step on the
    edge weights is an in-place edit per step.  After each of two steps, output, grad_B and grad_val are bitwise
    those of a fresh handle on clones of the current arrays, and within 1e-5 (the gate of tests/test_ops_gpu.py)
    of float64."""
    import _f64
    from pygcn_amd import CSRGraph
    from pygcn_amd.ops import sparse_mm
    from pygcn_amd.utils import rmat_graph
    n, F = 2000, 64
    rowptr, col, val = (t.to(dev) for t in rmat_graph(n, 20000, seed=13, device="cpu"))
    B = torch.from_numpy(gin.dense((n, F), 1)).to(dev).requires_grad_(True)
    G = torch.from_numpy(gin.dense((n, F), 2)).to(dev)
    row = torch.repeat_interleave(torch.arange(n, device=dev), (rowptr[1:] - rowptr[:-1]).long())
    val.requires_grad_(True)
    g = CSRGraph(rowptr, col, val, (n, n))
    assert g.val is val

    def evaluate(graph, v):
        v.grad = B.grad = None
        out = sparse_mm(graph, B)
        out.backward(G)
        return out.detach().clone(), B.grad.clone(), v.grad.clone()

    def grad_val64():
        return (G.index_select(0, row).double() * B.detach().index_select(0, col.long()).double()).sum(1)
    # a step moves the weights by 1e-1 of their norm (from the float64 gradient: a condition on the inputs)
    lr = 0.1 * float(val.detach().abs().max()) / float(grad_val64().abs().max())
    opt = torch.optim.SGD([val], lr=lr)
    evaluate(g, val)                                                         # (transpose and schedules exist)
    for step in (1, 2):
        before = val.detach().clone()
        opt.step()                                                           # val -= lr · grad_val, in place
        assert float((val.detach() - before).abs().max()) >= MOVED * float(before.abs().max())
        got = evaluate(g, val)
        v2 = val.detach().clone().requires_grad_(True)
        want = evaluate(CSRGraph(rowptr.clone(), col.clone(), v2, (n, n)), v2)
        for name, a, b in zip(("A·B", "grad_B", "grad_val"), got, want):
            assert torch.equal(a, b), f"step {step}: {name} differs from the fresh handle's"
        v = val.detach()
        assert_normwise(got[0].cpu(), _f64.spmm64(rowptr, col, v, B.detach()).cpu(), TOL, f"step {step}: A·B")
        assert_normwise(got[1].cpu(), _f64.spmm64_t(rowptr, col, v, G, n).cpu(), TOL, f"step {step}: grad_B")
        assert_normwise(got[2].cpu(), grad_val64().cpu(), TOL, f"step {step}: grad_val")


# ---------------------------------------------------------------- torch sparse tensors through as_graph
@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_sparse_tensor_adjacency_follows_an_edit_of_its_values(oracle, dev, layout):
    """The layer caches a handle on the torch sparse tensor it is given (graph.as_graph): an in-place edit of
    `adj._values()` / `adj.values()` between two calls is seen, output and gradients being those of the layer on
    a tensor built from the edited arrays."""
    from pygcn_amd.layers import GraphConvolution
    n, F = 2000, 64
    rowptr, col, val = _arrays(n, 20000, 17, "mul")
    row = np.repeat(np.arange(n), np.diff(rowptr))
    w = _mul_weights(len(val))

    def tensor(values):
        v = torch.from_numpy(values).to(dev)
        if layout == "coo":
            return torch.sparse_coo_tensor(torch.from_numpy(np.stack([row, col.astype(np.int64)])).to(dev), v, (n, n))
        return torch.sparse_csr_tensor(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col.astype(np.int64)).to(dev),
                                       v, (n, n))
    x_np, G = gin.dense((n, F), 3), torch.from_numpy(gin.dense((n, F), 4)).to(dev)
    x = torch.from_numpy(x_np).to(dev).requires_grad_(True)
    torch.manual_seed(3)
    layer = GraphConvolution(F, F).to(dev)

    def call(adj):
        layer.zero_grad(set_to_none=True)
        x.grad = None
        out = layer(x, adj)
        out.backward(G)
        return out.detach().clone(), x.grad.clone(), layer.weight.grad.clone(), layer.bias.grad.clone()
    # the condition on the inputs: the reference layer's output moves
    p = [layer.weight.detach().cpu().numpy(), layer.bias.detach().cpu().numpy()]
    ref = [oracle.gc_forward(x_np, p[0], p[1], oracle.CSR(rowptr, col, v, (n, n)))[0] for v in (val, val * w)]
    assert np.abs(ref[1] - ref[0]).max() >= MOVED * np.abs(ref[1]).max()
    adj = tensor(val)
    first = call(adj)
    assert_normwise(first[0].cpu(), ref[0], TOL, "before the edit")
    (adj._values() if layout == "coo" else adj.values()).mul_(torch.from_numpy(w).to(dev))
    got, want = call(adj), call(tensor(val * w))
    for name, a, b in zip(("output", "grad_input", "grad_weight", "grad_bias"), got, want):
        assert torch.equal(a, b), f"{layout}: {name} differs from the layer on a freshly built tensor"
    assert_normwise(got[0].cpu(), ref[1], TOL, "after the edit")
