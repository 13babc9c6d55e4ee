"""CPU side of `functional.aggregate_linear` (pygcn_amd/agglin.py) and of the `aggregate_first` flag: the header,
the binding table, the documented formula of gcn_agg_linear_partial_rows, the exactly summable fixture of
tests/_agglin_ref.py, `supported()` outside the rule and the composition that runs there, and the flag on the models
and in get_model.  No GPU needed."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _agglin_ref as R
from conftest import ROOT
from test_evaluator_cpu import KEYS, config

NAMES = ("gcn_agg_linear_partial_rows", "gcn_agg_linear_forward", "gcn_agg_linear_backward")
COUNTS = (4, 10, 13)


def test_header_table_and_library():
    from pygcn_amd import _native, build
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert re.search(r"#define GCN_ABI_VERSION\s+26\b", hdr) and _native.GCN_ABI_VERSION == 26
    assert _native.lib().gcn_abi_version() == 26                    # additive: the number did not move
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = __import__("ctypes").CDLL(_native.LIB_PATH)
    for name, count in zip(NAMES, COUNTS):
        assert name in _native.SIGNATURES and name in _native.EXPORTS
        assert not name.endswith("_workspace_bytes")
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", code)
        assert decl and len(decl.group(1).split(",")) == count == len(_native.SIGNATURES[name][1]), name
        assert hasattr(raw, name) and getattr(_native.lib(), name).argtypes == _native.SIGNATURES[name][1]
    assert _native.SIGNATURES[NAMES[0]][0] is __import__("ctypes").c_int64
    assert any(src.endswith("gcn_agglin.hip") for src in build.SRCS)


def test_row_query_follows_its_documented_formula():
    """B = ceil(M / R), M = n * batch, R = 64 * ceil(M / (64 * 2048)); 0 outside Fin in {4, 8, ..., 32}, Fout = 32,
    n >= 1, 1 <= batch <= 65535."""
    from pygcn_amd import _native
    query = _native.lib().gcn_agg_linear_partial_rows
    assert query(1, 8, 32, 1) == 1 and query(64, 8, 32, 1) == 1 and query(65, 8, 32, 1) == 2
    assert query(64 * 2048, 16, 32, 1) == 2048 and query(64 * 2048 + 1, 16, 32, 1) == 1025
    for n in (1, 2, 63, 65, 1000, 131072, 131073, 1_000_000):
        for batch in (1, 3, 20):
            for fin in (4, 8, 12, 16, 20, 24, 28, 32):
                assert query(n, fin, 32, batch) == R.partial_rows_formula(n, batch)[0]
    assert query(1_000_000, 8, 32, 20) <= 2048
    for n, fin, fout, batch in ((37, 5, 32, 1), (37, 0, 32, 1), (37, 36, 32, 1), (37, 64, 32, 1), (37, 8, 16, 1),
                                (37, 8, 64, 1), (0, 8, 32, 1), (-1, 8, 32, 1), (37, 8, 32, 0), (37, 8, 32, 65536)):
        assert query(n, fin, fout, batch) == 0
    n = R.n_three_blocks(query, 8, 3)
    blocks, per_block = R.partial_rows_formula(n, 3)
    assert blocks >= 3 and (3 * n) % per_block != 0 and n < 1000


@pytest.mark.parametrize("n,k,fin", [(65, 3, 4), (43, 3, 32), (1000, 1, 16), (1000, 3, 8)])
@pytest.mark.parametrize("relu", [False, True])
def test_the_exact_fixture_is_exactly_summable(n, k, fin, relu):
    """float32 and float64 evaluations of the reference's association are equal bit for bit, and so is the
    aggregate-first association: no order of summation rounds anything."""
    rowptr, col, val = R.random_csr(n, 300 + n, exact=True)
    adj = R.dense_of(rowptr, col, val, n)
    x, w, b, g = R.exact_operands(n, k, fin, 310 + n + fin)
    r32 = R.step(adj, x, w, b, g, torch.float32, batch=k, relu=relu)
    r64 = R.step(adj, x, w, b, g, torch.float64, batch=k, relu=relu)
    for a, c in zip(r32, r64):
        assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), c)
        assert np.abs(c).max() > 0
    z = adj.double() @ x.double()
    y = torch.cat([z[:, j * fin:(j + 1) * fin] @ w.double() + b.double() for j in range(k)], dim=1)
    y = torch.relu(y) if relu else y
    assert np.array_equal(y.numpy(), r64[0])
    assert float(z.abs().max()) < 2 ** 13 and float(y.abs().max()) < 2 ** 20
    assert int((g != 0).any(1).sum()) <= 16


def test_the_graph_has_an_empty_row_and_a_hub():
    rowptr, col, val = R.random_csr(65, 1)
    length = (rowptr[1:] - rowptr[:-1]).tolist()
    assert length[1] == 0 and length[0] == 65 and max(length[2:]) <= 8
    assert set(np.abs(R.random_csr(65, 1, exact=True)[2].numpy()).tolist()) <= {0.5, 1.0, 2.0}


def test_outside_the_rule_it_is_the_composition():
    """A CPU tensor, a dense adjacency, an input that requires grad: `supported` is false and the call is
    GraphConvolution.forward_wide's composition, bit for bit, gradients included."""
    from pygcn_amd import agglin
    from pygcn_amd.functional import aggregate_linear
    from pygcn_amd.layers import GraphConvolution
    assert aggregate_linear is agglin.aggregate_linear
    n, k, fin = 21, 3, 8
    x, w, b, g = R.operands(n, k, fin, 320)
    adj = torch.rand(n, n)
    assert not agglin.supported(x, adj, w, b, k)
    assert not agglin.supported(x.clone().requires_grad_(), adj, w, b, k)
    assert not agglin.supported(x, adj.to_sparse_csr(), w, b, k)               # (a CPU sparse tensor: no CSRGraph)
    torch.manual_seed(5)
    gc = GraphConvolution(fin, 32)
    for relu in (False, True):
        xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
        got = aggregate_linear(xa, adj, gc.weight, gc.bias, batch=k, relu=relu)
        want = gc.forward_wide(xb, adj, k, relu=relu)
        assert got.shape == (n, k * 32) and torch.equal(got, want)
        gc.zero_grad()
        got.backward(g)
        grads = [p.grad.clone() for p in gc.parameters()]
        gc.zero_grad()
        want.backward(g)
        assert torch.equal(xa.grad, xb.grad) and all(torch.equal(a, p.grad) for a, p in zip(grads, gc.parameters()))
        assert torch.equal(gc.forward_aggregate_first(x, adj, k, relu=relu), want)
    r32 = R.step(adj, x, gc.weight, gc.bias, g, torch.float32, batch=k)
    assert np.allclose(aggregate_linear(x, adj, gc.weight, gc.bias, batch=k).detach().numpy(), r32[0], atol=1e-5)
    with pytest.raises(RuntimeError, match="x must be"):
        aggregate_linear(x, adj, w, b, batch=2)


def test_aggregate_first_models_construct_with_the_default_keys():
    from pygcn_amd import GCN_OVER_MLP, Generator, Hierarchical_Generator, SoftGenerator, get_model
    from pygcn_amd.models import GCNBatchNorm, GCNStack
    plain, agg = GCNBatchNorm(8, 32, 32, 0.5, 3), GCNBatchNorm(8, 32, 32, 0.5, 3, aggregate_first=True)
    assert agg.aggregate_first is True and plain.aggregate_first is False and agg.fused_norm is False
    assert list(agg.state_dict()) == list(plain.state_dict())
    stack, stack_agg = GCNStack(8, 32, 32), GCNStack(8, 32, 32, aggregate_first=True)
    assert stack_agg.aggregate_first is True and stack.aggregate_first is False
    assert list(stack_agg.state_dict()) == list(stack.state_dict())
    ev = GCN_OVER_MLP(8, 32, 32, 0.0, 5, 40, 16, 8, 8, aggregate_first=True)
    assert ev.GCNLayer.aggregate_first is True and ev.GCNLayer.fused_norm is False and list(ev.state_dict()) == KEYS
    both = GCN_OVER_MLP(8, 32, 32, 0.0, 5, 40, 16, 8, 8, fused_norm=True, aggregate_first=True)
    assert both.GCNLayer.aggregate_first is True and both.GCNLayer.fused_norm is True
    assert Generator(8, 32, 32, 0.0, 5, 34, 16, 8, 8, aggregate_first=True).GCNLayer.aggregate_first is True
    hier = Hierarchical_Generator(8, 32, 32, 0.0, 5, 34, 16, 8, 8, aggregate_first=True)
    assert hier.GCNLayer.aggregate_first is True
    assert SoftGenerator(8, 32, 32, 0.0, 5, 16, 8, 8, aggregate_first=True).GCN.aggregate_first is True
    on = SimpleNamespace(aggregate_first=True, **vars(config()))
    assert get_model(config(), "GNN_OVER_MLP").GCNLayer.aggregate_first is False
    assert get_model(on, "GNN_OVER_MLP").GCNLayer.aggregate_first is True
    assert list(get_model(on, "GNN_OVER_MLP").state_dict()) == KEYS
    for name in ("Generator", "Hierarchical_Generator"):
        assert get_model(on, name).GCNLayer.aggregate_first is True
        assert get_model(config(), name).GCNLayer.aggregate_first is False
    assert get_model(on, "SoftGenerator").GCN.aggregate_first is True
    assert get_model(config(), "SoftGenerator").GCN.aggregate_first is False


def test_aggregate_first_model_on_the_cpu_is_the_default_model():
    """Outside the rule (CPU tensors, a dense adjacency) the flag changes nothing: the same nodes, the same bits."""
    from pygcn_amd.models import GCNBatchNorm, GCNStack
    torch.manual_seed(3)
    adj = torch.eye(20) * 0.5 + torch.ones(20, 20) / 40
    plain, agg = GCNBatchNorm(8, 32, 32, 0.5, 3), GCNBatchNorm(8, 32, 32, 0.5, 3, aggregate_first=True)
    agg.load_state_dict(plain.state_dict())
    for x in (torch.randn(1, 20, 8), torch.randn(3, 20, 8)):       # (a 2-D input needs the HIP device)
        a, b = plain(x, adj), agg(x, adj)
        assert a.shape == b.shape and torch.equal(a, b)
        a.sum().backward()
        b.sum().backward()
    for p, q in zip(plain.parameters(), agg.parameters()):
        assert torch.equal(p.grad, q.grad)
    stack, stack_agg = GCNStack(8, 32, 32), GCNStack(8, 32, 32, aggregate_first=True)
    stack_agg.load_state_dict(stack.state_dict())
    x3 = torch.randn(3, 20, 8)
    assert torch.equal(stack(x3, adj), stack_agg(x3, adj))
