"""CPU side of `functional.relu_batch_norm_linear` (pygcn_amd/normlin.py): the torch restatement
tests/_normlin_ref.py against F.batch_norm, the two identities of its backward sums, the `fused_norm` flag of
GCNBatchNorm / GCN_OVER_MLP / get_model, the header, the binding table, the workspace query and the composition
that runs outside the shape rule.  No GPU needed."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _normlin_ref as R
from conftest import ROOT
from test_evaluator_cpu import KEYS, config

NAMES = ("gcn_bn_linear_workspace_bytes", "gcn_bn_linear_forward", "gcn_bn_linear_backward_sums",
         "gcn_bn_linear_backward_apply")
COUNTS = (4, 11, 16, 11)


def data(n, k, fin, fout, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, k * fin, generator=g, dtype=dtype)
    for j in range(k):
        z[:, j * fin + 3] = -z[:, j * fin + 3].abs() - 0.5          # relu(z) is all zero in this column
    w = torch.randn(fin, fout, generator=g, dtype=dtype)
    ds = torch.randn(n, k * fout, generator=g, dtype=dtype)
    return z, w, ds


@pytest.mark.parametrize("n,k,fin,fout", [(2, 1, 32, 32), (33, 3, 32, 32), (50, 2, 8, 5)])
def test_restatement_is_batch_norm_times_weight_in_float64(n, k, fin, fout):
    z, w, ds = data(n, k, fin, fout, 5)
    za, wa = z.clone().requires_grad_(), w.clone().requires_grad_()
    zb, wb = z.clone().requires_grad_(), w.clone().requires_grad_()
    got = R.relu_batch_norm_linear(za, wa, batch=k)
    want = torch.cat([F.batch_norm(torch.relu(zb[:, j * fin:(j + 1) * fin]), None, None, None, None, True, 0.0, 1e-5)
                      @ wb for j in range(k)], dim=1)
    got.backward(ds)
    want.backward(ds)
    for a, b in ((got, want), (za.grad, zb.grad), (wa.grad, wb.grad)):
        assert a.shape == b.shape
        assert float((a.detach() - b.detach()).abs().max()) <= 1e-12 * float(b.detach().abs().max())
    assert not za.grad[:, 3].any()                                  # the dead column passes no gradient


def test_the_two_identities_of_the_backward_sums_in_float64():
    z, w, ds = data(257, 1, 32, 32, 6)
    direct, folded, P = R.backward_sums(z, w, ds)
    assert not P[3].any() and float(direct[1][3]) == 0.0            # xhat of the all-zero column is zero
    for a, b in zip(direct, folded):
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())


def test_fused_norm_models_construct_with_the_default_keys():
    from types import SimpleNamespace
    from pygcn_amd import GCN_OVER_MLP, get_model
    from pygcn_amd.models import GCNBatchNorm
    plain, fused = GCNBatchNorm(8, 32, 32, 0.5, 3), GCNBatchNorm(8, 32, 32, 0.5, 3, fused_norm=True)
    assert fused.fused_norm is True and plain.fused_norm is False
    assert list(fused.state_dict()) == list(plain.state_dict())
    ev = GCN_OVER_MLP(8, 32, 32, 0.0, 5, 40, 16, 8, 8, fused_norm=True)
    assert ev.GCNLayer.fused_norm is True and list(ev.state_dict()) == KEYS
    assert GCN_OVER_MLP(8, 32, 32, 0.0, 5, 40, 16, 8, 8).GCNLayer.fused_norm is False
    assert get_model(config(), "GNN_OVER_MLP").GCNLayer.fused_norm is False
    on = get_model(SimpleNamespace(fused_norm=True, **vars(config())), "GNN_OVER_MLP")
    assert on.GCNLayer.fused_norm is True and list(on.state_dict()) == KEYS


def test_fused_norm_model_on_the_cpu_is_the_default_model():
    """Outside the shape rule (CPU tensors) the flag changes nothing: the same nodes, the same bits."""
    from pygcn_amd.models import GCNBatchNorm
    torch.manual_seed(3)
    plain = GCNBatchNorm(8, 32, 32, 0.5, 3)
    fused = GCNBatchNorm(8, 32, 32, 0.5, 3, fused_norm=True)
    fused.load_state_dict(plain.state_dict())
    adj = torch.eye(20) * 0.5 + torch.ones(20, 20) / 40
    for x in (torch.randn(1, 20, 8), torch.randn(3, 20, 8)):       # (a 2-D input needs the HIP device)
        a, b = plain(x, adj), fused(x, adj)
        assert a.shape == b.shape and torch.equal(a, b)
        a.sum().backward()
        b.sum().backward()
    for p, q in zip(plain.parameters(), fused.parameters()):
        assert torch.equal(p.grad, q.grad)


def test_aggregate_is_the_layers_second_half():
    from pygcn_amd.layers import GraphConvolution
    torch.manual_seed(4)
    gc = GraphConvolution(8, 5)
    adj, x = torch.rand(9, 9), torch.randn(9, 2 * 8)
    support = (x.reshape(18, 8) @ gc.weight).view(9, 10)
    assert torch.equal(gc.aggregate(support, adj, 2, relu=True), gc.forward_wide(x, adj, 2, relu=True))
    with pytest.raises(RuntimeError, match="support must be"):
        gc.aggregate(support, adj, 3)


def test_header_table_and_library():
    from pygcn_amd import _native, build
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert re.search(r"#define GCN_ABI_VERSION\s+26\b", hdr) and _native.GCN_ABI_VERSION == 26
    assert _native.lib().gcn_abi_version() == 26
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = __import__("ctypes").CDLL(_native.LIB_PATH)
    for name, count in zip(NAMES, COUNTS):
        assert name in _native.SIGNATURES and name in _native.EXPORTS
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", code)
        assert decl and len(decl.group(1).split(",")) == count == len(_native.SIGNATURES[name][1]), name
        assert hasattr(raw, name) and getattr(_native.lib(), name).argtypes == _native.SIGNATURES[name][1]
    assert any(src.endswith("gcn_normlin.hip") for src in build.SRCS)


def test_workspace_query_follows_its_documented_formula():
    """batch * (B + 1) * 1152 * sizeof(double), T = ceil(n / (128 * 512)), R = 128 * T, B = ceil(n / R); 0 outside
    Fin = Fout = 32, n >= 2, 1 <= batch <= 65535."""
    from pygcn_amd import _native
    L = _native.lib()
    assert L.gcn_bn_linear_workspace_bytes(2, 32, 32, 1) == 2 * 1152 * 8
    for n in (2, 128, 129, 65536, 65537, 1_000_000):
        for batch in (1, 3, 20, 65535):
            tiles = -(-n // (128 * 512))
            blocks = -(-n // (128 * tiles))
            assert L.gcn_bn_linear_workspace_bytes(n, 32, 32, batch) == batch * (blocks + 1) * 1152 * 8
    for n, fin, fout, batch in ((37, 24, 32, 1), (37, 32, 24, 1), (37, 64, 64, 1), (1, 32, 32, 1), (0, 32, 32, 1),
                                (37, 32, 32, 0), (37, 32, 32, 65536)):
        assert L.gcn_bn_linear_workspace_bytes(n, fin, fout, batch) == 0


@pytest.mark.parametrize("case", ["cpu", "bf16", "width16", "ragged"])
def test_outside_the_rule_it_is_the_composition(case):
    from pygcn_amd.functional import relu_batch_norm, relu_batch_norm_linear
    from pygcn_amd.gemm import DenseMMFunction
    from pygcn_amd.normlin import supported
    k, n = 3, 21
    fin, fout = {"width16": (16, 16), "ragged": (32, 7)}.get(case, (32, 32))
    dtype = torch.bfloat16 if case == "bf16" else torch.float32
    z, w, ds = (t.to(dtype) for t in data(n, k, fin, fout, 8, torch.float32))
    assert not supported(z, w, k)
    za, wa = z.clone().requires_grad_(), w.clone().requires_grad_()
    zb, wb = z.clone().requires_grad_(), w.clone().requires_grad_()
    got = relu_batch_norm_linear(za, wa, batch=k)
    want = DenseMMFunction.apply(relu_batch_norm(zb, batch=k).reshape(n * k, fin), wb).view(n, k * fout)
    assert got.shape == (n, k * fout) and torch.equal(got, want)
    got.backward(ds)
    want.backward(ds)
    assert torch.equal(za.grad, zb.grad) and torch.equal(wa.grad, wb.grad)
    with pytest.raises(RuntimeError, match="z must be"):
        relu_batch_norm_linear(z, w, batch=2)


def test_exports():
    from pygcn_amd import functional, normlin
    assert functional.relu_batch_norm_linear is normlin.relu_batch_norm_linear
