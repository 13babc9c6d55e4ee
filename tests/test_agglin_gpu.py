"""`functional.aggregate_linear` on the MI355X (gcn_agg_linear_forward / gcn_agg_linear_backward,
pygcn_amd/csrc/gcn_agglin.hip) and the `aggregate_first` flag of the models.

y, grad_W and grad_b against the torch restatement of the REFERENCE's association, tests/_agglin_ref.py, on the CPU
— float64 the arbiter, float32 the reference arithmetic — through conftest.assert_parity at the project's 1e-5;
exactly on operands where every partial sum is representable; windows, repeated runs and the ReLU forms bitwise.
The multi-block shapes are derived from the documented formula of gcn_agg_linear_partial_rows (include/gcn_spmm.h),
so a retune moves them with it."""
import numpy as np
import pytest
import torch

import _agglin_ref as R
import _attention_ref as A
import _evaluator_ref as E
import _select_ref as G
import test_batched_norm_gpu as B
import test_norm_gpu as T
import test_select_gpu as S
from conftest import assert_normwise, assert_parity, load_golden
from test_evaluator_cpu import g9_case
from test_norm_gpu import DEV, seeded

pytestmark = pytest.mark.gpu

W32 = R.WIDTH
NODE = "AggregateLinearFunction"


def query():
    from pygcn_amd import _native
    return _native.lib().gcn_agg_linear_partial_rows


def rows_of(name, fin, k):
    return R.n_three_blocks(query(), fin, k) if name == "three_blocks" else int(name)


_GRAPHS = {}


def graph(n, exact=False):
    """(dense adjacency on the CPU, CSRGraph on the device) of R.random_csr(n): made once, never written to."""
    from pygcn_amd import CSRGraph
    key = (n, exact)
    if key not in _GRAPHS:
        rowptr, col, val = R.random_csr(n, 400 + n, exact=exact)
        _GRAPHS[key] = (R.dense_of(rowptr, col, val, n),
                        CSRGraph(rowptr.to(DEV), col.to(DEV), val.to(DEV), (n, n)))
    return _GRAPHS[key]


def device_step(csr, x, w, b, g, k, relu):
    """(y, grad_W, grad_b) of the HIP node on the device."""
    from pygcn_amd.functional import aggregate_linear
    xd, wd = x.to(DEV), w.to(DEV).requires_grad_()
    bd = b.to(DEV).requires_grad_() if b is not None else None
    y = aggregate_linear(xd, csr, wd, bd, batch=k, relu=relu)
    assert y.grad_fn.name().startswith(NODE), y.grad_fn.name()
    y.backward(g.to(DEV))
    torch.cuda.synchronize()
    return y.detach(), wd.grad, bd.grad if bd is not None else None


def sweeps(z, w, b, g, k, relu):
    """The two entry points on a given z [n, k * Fin] (device tensors): (y, grad_W, grad_b)."""
    from pygcn_amd import _native
    n, fin = z.shape[0], w.shape[0]
    y = torch.empty(n, k * W32, device=DEV)
    _native.launch("gcn_agg_linear_forward", DEV, z.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None,
                   y.data_ptr(), n, fin, W32, k, int(relu))
    rows = query()(n, fin, W32, k)
    partials = torch.empty(rows, fin * W32 + W32, dtype=torch.float64, device=DEV)
    gw, gb = torch.empty(fin, W32, device=DEV), torch.empty(W32, device=DEV)
    _native.launch("gcn_agg_linear_backward", DEV, g.data_ptr(), y.data_ptr(), z.data_ptr(), n, fin, W32, k, int(relu),
                   gw.data_ptr(), gb.data_ptr(), partials.data_ptr(), rows)
    torch.cuda.synchronize()
    return y, gw, gb


def test_the_derived_shape_has_its_properties():
    for fin, k in ((8, 1), (8, 3), (32, 20)):
        n = R.n_three_blocks(query(), fin, k)
        blocks, per_block = R.partial_rows_formula(n, k)
        assert blocks >= 3 and (n * k) % per_block != 0 and (blocks - 1) * per_block < n * k and n < 1000


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("fin", R.FINS)
@pytest.mark.parametrize("k", [1, 3, 20])
@pytest.mark.parametrize("n_name", ["1", "2", "63", "65", "1000", "three_blocks"])
def test_forward_and_backward_against_the_reference_association(n_name, k, fin):
    n = rows_of(n_name, fin, k)
    adj, csr = graph(n)
    for bias in (True, False):
        x, w, b, g = R.operands(n, k, fin, 500 + fin + k, bias=bias)
        pre64 = None
        for relu in (False, True):
            y, gw, gb = device_step(csr, x, w, b, g, k, relu)
            assert y.shape == (n, k * W32) and gw.shape == (fin, W32) and y.dtype == gw.dtype == torch.float32
            mask = None
            if relu:      # the ReLU derivative the device used, where it differs from float64's at the boundary only
                mask = (y > 0).cpu()
                R.flips_are_at_the_boundary(mask.numpy(), pre64)
            r32 = R.step(adj, x, w, b, g, torch.float32, batch=k, relu=relu, mask=mask)
            r64 = R.step(adj, x, w, b, g, torch.float64, batch=k, relu=relu, mask=mask)
            pre64 = r64[0]
            what = f"aggregate_linear [{n}x{k}x{fin}] bias={bias} relu={relu}"
            assert_parity(y.cpu().numpy(), r32[0], r64[0], what + " y")
            assert_parity(gw.cpu().numpy(), r32[1], r64[1], what + " grad_W")
            if bias:
                assert gb.shape == (W32,)
                assert_parity(gb.cpu().numpy(), r32[2], r64[2], what + " grad_b")
            else:
                assert gb is None
    if n >= 3:
        assert not y[1].any()                                       # the empty row, without bias: zeros


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("fin", R.FINS)
@pytest.mark.parametrize("n_name,k", [("65", 3), ("three_blocks", 3), ("1000", 1), ("1000", 3)])
def test_exactly_summable_operands_give_the_float64_result(n_name, k, fin, relu):
    """Small integers in x, b and the cotangent, signed powers of two in W and the adjacency (R.exact_operands):
    y, grad_W and grad_b EQUAL the float64 evaluation of the reference's association — no tolerance; a difference
    is an indexing, staging or missing-term error, never rounding."""
    n = rows_of(n_name, fin, k)
    adj, csr = graph(n, exact=True)
    x, w, b, g = R.exact_operands(n, k, fin, 600 + n + fin)
    y, gw, gb = device_step(csr, x, w, b, g, k, relu)
    r64 = R.step(adj, x, w, b, g, torch.float64, batch=k, relu=relu)
    for name, got, want in zip(("y", "grad_W", "grad_b"), (y, gw, gb), r64):
        assert np.abs(want).max() > 0, name
        assert np.array_equal(got.cpu().numpy().astype(np.float64), want), f"{name} [{n}x{k}x{fin}] relu={relu}"


# ------------------------------------------------------------------------------------------------ bitwise
@pytest.mark.parametrize("fin", R.FINS)
@pytest.mark.parametrize("n_name,k", [("65", 3), ("three_blocks", 3), ("1000", 20)])
def test_windows_runs_and_relu_forms_are_bitwise(n_name, k, fin):
    n = rows_of(n_name, fin, k)
    adj, csr = graph(n)
    x, w, b, g = R.operands(n, k, fin, 700 + fin + k)
    plain = device_step(csr, x, w, b, g, k, False)
    act = device_step(csr, x, w, b, g, k, True)
    for relu, first in ((False, plain), (True, act)):                # two runs, backward included
        for a, c in zip(first, device_step(csr, x, w, b, g, k, relu)):
            assert torch.equal(a, c)
    assert torch.equal(act[0], torch.relu(plain[0]))                 # the ReLU of the sweep is torch.relu
    masked = torch.where(act[0] > 0, g.to(DEV), torch.zeros((), device=DEV)).cpu()
    pre = device_step(csr, x, w, b, masked, k, False)                # relu backward = plain backward on g * [y > 0]
    assert torch.equal(pre[1], act[1]) and torch.equal(pre[2], act[2])
    # window j of the batched sweep is the batch = 1 sweep on a contiguous copy of the window (the same z)
    from pygcn_amd.spmm import spmm_csr
    z = spmm_csr(csr, x.to(DEV))
    wd, bd, gd = w.to(DEV), b.to(DEV), g.to(DEV)
    for relu, whole in ((False, plain), (True, act)):
        y, gw, gb = sweeps(z, wd, bd, gd, k, relu)
        assert torch.equal(y, whole[0]) and torch.equal(gw, whole[1]) and torch.equal(gb, whole[2])
        total_w, total_b = torch.zeros(fin, W32, dtype=torch.float64), torch.zeros(W32, dtype=torch.float64)
        for j in range(k):
            y1, gw1, gb1 = sweeps(z[:, j * fin:(j + 1) * fin].contiguous(), wd, bd,
                                  gd[:, j * W32:(j + 1) * W32].contiguous(), 1, relu)
            assert torch.equal(y1, y[:, j * W32:(j + 1) * W32]), (j, relu)
            total_w += gw1.double().cpu()
            total_b += gb1.double().cpu()
        # (the batched gradients are rounded once, the per-window ones k times: equal to rounding only)
        assert_normwise(gw.cpu().numpy(), total_w.numpy(), what=f"grad_W [{n}x{k}x{fin}] vs the sum over the windows")
        assert_normwise(gb.cpu().numpy(), total_b.numpy(), what=f"grad_b [{n}x{k}x{fin}] vs the sum over the windows")


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_argument_errors():
    """All pointers are valid device memory of the stated size; every bad call returns its code before a launch."""
    from pygcn_amd import _native
    L = _native.lib()
    n, k, fin = 37, 3, 8
    z, g = torch.zeros(n, k * fin, device=DEV), torch.zeros(n, k * W32, device=DEV)
    w, b = torch.zeros(fin, W32, device=DEV), torch.zeros(W32, device=DEV)
    y = torch.full((n, k * W32), 7.0, device=DEV)
    gw, gb = torch.full((fin, W32), 7.0, device=DEV), torch.full((W32,), 7.0, device=DEV)
    rows = L.gcn_agg_linear_partial_rows(n, fin, W32, k)
    assert rows == 2
    part = torch.full((rows, fin * W32 + W32), 7.0, dtype=torch.float64, device=DEV)

    def calls(n=n, fin=fin, fout=W32, k=k, zp=z.data_ptr(), wp=w.data_ptr(), yp=y.data_ptr(), gp=g.data_ptr(),
              gwp=gw.data_ptr(), pp=part.data_ptr(), rows=rows, relu=1):
        return {
            "gcn_agg_linear_forward": lambda: L.gcn_agg_linear_forward(zp, wp, b.data_ptr(), yp, n, fin, fout, k, relu,
                                                                       None),
            "gcn_agg_linear_backward": lambda: L.gcn_agg_linear_backward(gp, yp, zp, n, fin, fout, k, relu, gwp,
                                                                         gb.data_ptr(), pp, rows, None),
        }

    def expect(table, code, only=None):
        for name, call in table.items():
            if only is None or name in only:
                assert call() == code, name
                assert L.gcn_last_error().decode().startswith(name + ":"), (name, L.gcn_last_error())

    for bad in (dict(fin=5), dict(fin=0), dict(fin=36), dict(fout=16), dict(fout=64), dict(n=0), dict(k=0),
                dict(k=65536), dict(zp=None), dict(yp=None)):
        expect(calls(**bad), -1)                                           # GCN_E_BADARG
    expect(calls(wp=None), -1, ["gcn_agg_linear_forward"])
    expect(calls(gp=None), -1, ["gcn_agg_linear_backward"])
    expect(calls(gwp=None), -1, ["gcn_agg_linear_backward"])
    expect(calls(zp=z.data_ptr() + 4), -2)                                 # GCN_E_ALIGN
    expect(calls(pp=part.data_ptr() + 4), -2, ["gcn_agg_linear_backward"])
    expect(calls(rows=rows - 1), -3, ["gcn_agg_linear_backward"])          # GCN_E_WORKSPACE: one row short
    expect(calls(pp=None), -3, ["gcn_agg_linear_backward"])
    torch.cuda.synchronize()
    for t in (y, gw, gb, part):
        assert bool((t == 7.0).all())                                      # nothing was launched
    assert calls(yp=None, relu=0)["gcn_agg_linear_backward"]() == 0        # y is not read without relu
    torch.cuda.synchronize()
    assert not gw.any() and not gb.any()                                   # (z = g = 0)


# ------------------------------------------------------------------------------------------------ the models
def grads_of(model):
    return {name: p.grad.detach().cpu().numpy() for name, p in model.named_parameters()}


def compare_routes(what, on, off, ref64):
    """(output, parameter gradients) of the flag on against the flag off — the output normwise at 1e-5, the
    gradients through assert_parity with the flag-off run as the float32 reference and `ref64` as the arbiter."""
    assert_normwise(on[0], off[0], what=f"{what}: output vs the flag off")
    assert sorted(on[1]) == sorted(off[1]) == sorted(ref64)
    for name in on[1]:
        assert_parity(on[1][name], off[1][name], ref64[name], f"{what}: {name}.grad")


@pytest.mark.parametrize("mode", ["2d", "3d", "3d_fused_norm"])
def test_batch_norm_model_with_aggregate_first(mode, monkeypatch):
    from pygcn_amd import GCNBatchNorm
    n, edges = B.CASES["random600x12"][:2]
    adj_cpu, adj_dev = B._graph(n, edges)
    k = 1 if mode == "2d" else 3
    x, cot = seeded((k, n, 8), 801), seeded((k, n, W32), 802)
    torch.manual_seed(42)
    plain = GCNBatchNorm(8, W32, W32, 0.5, 3)
    state = {name: v.detach().clone() for name, v in plain.state_dict().items()}
    agg = GCNBatchNorm(8, W32, W32, 0.5, 3, fused_norm=mode == "3d_fused_norm", aggregate_first=True)
    agg.load_state_dict(state)
    plain, agg = plain.to(DEV).train(), agg.to(DEV).train()
    xin, cin = (x[0].to(DEV), cot[0].to(DEV)) if mode == "2d" else (x.to(DEV), cot.to(DEV))
    spy = S.LaunchSpy(monkeypatch)
    out = agg(xin, adj_dev)
    out.backward(cin)
    names = spy.names()
    assert names.count("gcn_agg_linear_forward") == 1 and names.count("gcn_agg_linear_backward") == 1
    assert names.count("gcn_bn_linear_forward") == (2 if mode == "3d_fused_norm" else 0)
    want = plain(xin, adj_dev)
    want.backward(cin)
    masks = ([T.device_relu_masks(plain, xin, adj_dev)] if mode == "2d" else B.batched_relu_masks(plain, xin, adj_dev))
    torch.cuda.synchronize()
    for j in range(k):
        T.check_relu_masks(masks[j], state, x[j], adj_cpu)
    params = {name: v.detach().clone().double().requires_grad_() for name, v in state.items()}
    outs = torch.stack([T.fork_forward(params, x[j].double(), adj_cpu.to(torch.float64), masks[j])[0] for j in range(k)])
    outs.backward(cot.double())
    ref64 = {name: p.grad.numpy() for name, p in params.items()}
    shape = (k, n, W32)
    compare_routes(f"GCNBatchNorm {mode}", (out.detach().cpu().numpy().reshape(shape), grads_of(agg)),
                   (want.detach().cpu().numpy().reshape(shape), grads_of(plain)), ref64)
    assert_normwise(out.detach().cpu().numpy().reshape(shape), outs.detach().numpy(), what=f"{mode}: output vs float64")


def test_an_input_that_requires_grad_takes_the_default_route(monkeypatch):
    from pygcn_amd import GCNBatchNorm
    n, edges = B.CASES["random600x12"][:2]
    _, adj_dev = B._graph(n, edges)
    torch.manual_seed(42)
    plain = GCNBatchNorm(8, W32, W32, 0.5, 3)
    agg = GCNBatchNorm(8, W32, W32, 0.5, 3, aggregate_first=True)
    agg.load_state_dict(plain.state_dict())
    plain, agg = plain.to(DEV).train(), agg.to(DEV).train()
    cot = seeded((3, n, W32), 812).to(DEV)
    for x in (seeded((n, 8), 811), seeded((3, n, 8), 811)):
        xa, xb = x.to(DEV).requires_grad_(), x.to(DEV).requires_grad_()
        spy = S.LaunchSpy(monkeypatch)
        out, want = agg(xa, adj_dev), plain(xb, adj_dev)
        c = cot if x.dim() == 3 else cot[0]
        out.backward(c)
        want.backward(c)
        torch.cuda.synchronize()
        assert "gcn_agg_linear_forward" not in spy.names()
        assert torch.equal(out, want) and xa.grad is not None and torch.equal(xa.grad, xb.grad)
        for p, q in zip(agg.parameters(), plain.parameters()):
            assert torch.equal(p.grad, q.grad)
        agg.zero_grad()
        plain.zero_grad()
    from pygcn_amd.functional import aggregate_linear
    y = aggregate_linear(seeded((n, 8), 813).to(DEV).requires_grad_(), adj_dev, agg.gc1.weight, agg.gc1.bias)
    assert not y.grad_fn.name().startswith(NODE)


def test_stack_with_aggregate_first(monkeypatch):
    from pygcn_amd.models import GCNStack
    n = 257
    adj, csr = graph(n)
    x, cot = seeded((n, 16), 821), seeded((n, W32), 822)
    torch.manual_seed(11)
    plain = GCNStack(16, W32, W32)
    state = {name: v.detach().clone() for name, v in plain.state_dict().items()}
    agg = GCNStack(16, W32, W32, aggregate_first=True)
    agg.load_state_dict(state)
    plain, agg = plain.to(DEV).train(), agg.to(DEV).train()
    spy = S.LaunchSpy(monkeypatch)
    out = agg(x.to(DEV), csr)
    out.backward(cot.to(DEV))
    calls = [args for name, args in spy.calls if name == "gcn_agg_linear_forward"]
    assert len(calls) == 1 and calls[0][-1] == 1                    # the ReLU runs inside the sweep
    want = plain(x.to(DEV), csr)
    want.backward(cot.to(DEV))
    torch.cuda.synchronize()
    params = {name: v.detach().clone().double().requires_grad_() for name, v in state.items()}
    h = x.double()
    for i in (1, 2, 3):
        h = torch.relu(adj.double() @ (h @ params[f"gc{i}.weight"]) + params[f"gc{i}.bias"])
    h.backward(cot.double())
    compare_routes("GCNStack", (out.detach().cpu().numpy(), grads_of(agg)),
                   (want.detach().cpu().numpy(), grads_of(plain)), {name: p.grad.numpy() for name, p in params.items()})


@pytest.mark.parametrize("own_flag", [True, False])
@pytest.mark.parametrize("tag", ["a_", "b_", "c_"])
def test_the_evaluator_fixture_with_aggregate_first(tag, own_flag, monkeypatch):
    """g9 at the gates of test_evaluator_gpu.py::test_the_fixture_on_the_device, with x a constant: the flag on its
    own (it receives the fixture's gradient) or inside x (no gradient asked for)."""
    from pygcn_amd import CSRGraph, GCN_OVER_MLP
    g9 = load_golden("g9_evaluator.npz")
    state, x, adj, d = g9_case(g9, tag)
    dims = [int(v) for v in g9["dims"]]
    graph9 = CSRGraph(torch.from_numpy(g9["rowptr"]).to(DEV), torch.from_numpy(g9["col"]).to(DEV),
                      torch.from_numpy(g9["val"]).to(DEV), (64, 64))
    runs = []
    for flag_on in (True, False):
        model = GCN_OVER_MLP(dims[0], dims[1], dims[2], 0.0, dims[5], dims[2] + x.shape[2] - 1 - d, dims[3], dims[4],
                             dim_touched=d, aggregate_first=flag_on)
        model.load_state_dict(state, strict=True)
        model = model.to(DEV).train()
        flag = x[:, :, -1].clone().to(DEV).requires_grad_() if own_flag else None
        spy = S.LaunchSpy(monkeypatch)
        out = model(x.to(DEV), graph9, flag=flag)
        out.sum().backward()
        torch.cuda.synchronize()
        assert spy.names().count("gcn_agg_linear_forward") == spy.names().count("gcn_agg_linear_backward") == flag_on
        runs.append((out.detach().cpu().numpy(), grads_of(model), flag.grad.cpu().numpy() if own_flag else None))
    on, off = runs
    assert_normwise(on[0], g9[tag + "out"], what=f"aggregate_first {tag}out")
    for name in on[1]:
        assert_normwise(on[1][name], g9[tag + "grad_" + name], what=f"aggregate_first {tag}grad {name}")
    _, ref64, dflag64 = E.evaluator_step(state, x, adj, d, torch.float64, lambda o: o.sum(),
                                         flag=x[:, :, -1] if own_flag else None)
    compare_routes(f"GCN_OVER_MLP {tag}", on[:2], off[:2], ref64)
    if own_flag:
        assert_normwise(on[2], g9[tag + "dflag"], what=f"aggregate_first {tag}dflag")
        assert_parity(on[2], off[2], dflag64, f"GCN_OVER_MLP {tag}: flag gradient")


@pytest.mark.parametrize("tag", ["gen_", "hier_"])
def test_the_generator_fixtures_with_aggregate_first(tag, monkeypatch):
    """g8 at the gates of test_select_gpu.py::test_generators_against_the_fixture."""
    import pygcn_amd
    from pygcn_amd import CSRGraph
    g8 = load_golden("g8_generators.npz")
    hier = tag == "hier_"
    state, x, adj, d, nn_ = G.fixture_case(g8, tag)
    dims = [int(v) for v in g8["dims"]]
    cls = pygcn_amd.Hierarchical_Generator if hier else pygcn_amd.Generator
    n = x.shape[0]
    graph8 = CSRGraph(torch.from_numpy(g8["rowptr"]).to(DEV), torch.from_numpy(g8["col"]).to(DEV),
                      torch.from_numpy(g8["val"]).to(DEV), (n, n))
    runs = []
    for flag_on in (True, False):
        model = cls(dims[0], dims[1], dims[2], 0.0, nn_, dims[2] + x.shape[1] - d - hier, dims[3], dims[4],
                    dim_touched=d, aggregate_first=flag_on)
        model.load_state_dict(state, strict=True)
        model = model.to(DEV).train()
        spy = S.LaunchSpy(monkeypatch)
        scores = model.scores(x.to(DEV), graph8)
        assert spy.names().count("gcn_agg_linear_forward") == flag_on
        flag = model(x.to(DEV), graph8)
        flag.sum().backward()
        torch.cuda.synchronize()
        runs.append((scores.detach().cpu().numpy(), grads_of(model), flag.detach().cpu().numpy()))
    on, off = runs
    s64, _, g64 = G.generator_step(state, x, adj, d, nn_, torch.float64, hier)
    assert_parity(on[0], g8[tag + "scores"], s64, f"aggregate_first {tag}scores")
    G.assert_flag_exact(on[2], on[0], g8[tag + "vac_flag"], nn_, f"aggregate_first {tag}flag")
    for name in state:
        assert_parity(on[1][name], g8[tag + "grad_" + name], g64[name], f"aggregate_first {tag}grad {name}")
    compare_routes(f"{cls.__name__}", on[:2], off[:2], g64)


def test_the_soft_generator_fixture_with_aggregate_first(monkeypatch):
    """g7 at the gates of test_attention_gpu.py::test_soft_generator_reinforce_step."""
    from pygcn_amd import CSRGraph, SoftGenerator
    g7 = load_golden("g7_soft_generator.npz")
    state, x, adj, d, picked, reward = A.fixture_case(g7)
    dims = [int(v) for v in g7["dims"]]
    n = x.shape[0]
    graph7 = CSRGraph(torch.from_numpy(g7["rowptr"]).to(DEV), torch.from_numpy(g7["col"]).to(DEV),
                      torch.from_numpy(g7["val"]).to(DEV), (n, n))
    runs = []
    for flag_on in (True, False):
        model = SoftGenerator(dims[0], dims[1], dims[2], 0.0, dims[5], dims[3], dims[4], dim_touched=d,
                              aggregate_first=flag_on)
        model.load_state_dict(state, strict=True)
        model = model.to(DEV).train()
        spy = S.LaunchSpy(monkeypatch)
        attn = model(x.to(DEV), graph7)
        loss = -reward * torch.log(attn[picked.to(DEV)]).sum()
        loss.backward()
        torch.cuda.synchronize()
        assert spy.names().count("gcn_agg_linear_forward") == spy.names().count("gcn_agg_linear_backward") == flag_on
        runs.append((attn.detach().cpu().numpy(), grads_of(model), float(loss.detach())))
    on, off = runs
    attn64, grads64 = A.reinforce_step(state, x, adj, d, picked, reward, torch.float64)
    assert_parity(on[0], g7["attn"], attn64, "aggregate_first SoftGenerator attn")
    assert_normwise(on[2], float(g7["loss"]), what="aggregate_first SoftGenerator loss")
    for name in state:
        assert_parity(on[1][name], g7["grad_" + name], grads64[name], f"aggregate_first SoftGenerator grad {name}")
    compare_routes("SoftGenerator", on[:2], off[:2], grads64)


# ------------------------------------------------------------------------------------------------ cache, syncs
def test_the_input_product_cache_spares_layer_1_its_sparse_product(monkeypatch):
    """With fused.set_input_product_cache(True) a second step launches no sparse product on Fin-wide rows — the
    only one layer 1 has — and an in-place change of x brings it back; the results are the same bits."""
    from pygcn_amd import fused
    from pygcn_amd.models import GCNStack
    n, fin = 257, 8
    _, csr = graph(n)
    torch.manual_seed(12)
    model = GCNStack(fin, W32, W32, aggregate_first=True).to(DEV).train()
    x, cot = seeded((n, fin), 831).to(DEV), seeded((n, W32), 832).to(DEV)
    spy = S.LaunchSpy(monkeypatch)

    def step():
        model.zero_grad()
        before = len(spy.calls)
        out = model(x, csr)
        out.backward(cot)
        torch.cuda.synchronize()
        narrow = [args for name, args in spy.calls[before:] if name == "gcn_spmm_csr_ep" and args[6] == fin]
        return out.detach().clone(), model.gc1.weight.grad.clone(), len(narrow)

    base = step()
    assert base[2] == 1                                             # forward only: the backward pass has none
    try:
        fused.set_input_product_cache(True)
        first, second = step(), step()
        assert first[2] == 1 and second[2] == 0
        for a, b in zip(second[:2], base[:2]):
            assert torch.equal(a, b)
        x.add_(1.0)                                                 # an in-place change: the cached product is stale
        changed = step()
        assert changed[2] == 1 and not torch.equal(changed[0], base[0])
        assert step()[2] == 0
    finally:
        fused.set_input_product_cache(False)
        if hasattr(csr, "_input_product"):
            del csr._input_product
    fresh = step()
    assert fresh[2] == 1 and torch.equal(fresh[0], changed[0]) and torch.equal(fresh[1], changed[1])
    x.sub_(1.0)


def test_no_host_synchronisation():
    import torch.nn.functional as F
    from pygcn_amd import GCN_OVER_MLP
    n, edges = B.CASES["random600x12"][:2]
    _, adj_dev = B._graph(n, edges)
    torch.manual_seed(42)
    model = GCN_OVER_MLP(8, 32, 32, 0.5, 3, 32 + 17 - 1 - 8, 16, 8, dim_touched=8, aggregate_first=True).to(DEV).train()
    x = seeded((3, n, 17), 841)
    x[:, :, -1] = B.bernoulli_mask(3, n, 842)
    x, target = x.to(DEV), seeded((3, 1), 843).to(DEV)
    flag = x[:, :, -1].clone().requires_grad_()
    F.mse_loss(model(x, adj_dev, flag=flag), target).backward()    # (first use builds the graph's plans)
    kept = {}

    def forward(**kw):
        kept["loss"] = F.mse_loss(model(x, adj_dev, **kw), target)

    for kw in (dict(flag=flag), dict()):
        assert S.count_host_syncs(lambda: forward(**kw)) == 0
        assert kept["loss"].grad_fn is not None
        assert S.count_host_syncs(lambda: kept["loss"].backward()) == 0
    assert model.GCNLayer.gc1.weight.grad is not None
