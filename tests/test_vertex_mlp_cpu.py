"""The generators' score head off the device: the restatement tests/_vertex_mlp_ref.py against the fixture
g8_generators.npz, the CPU route of functional.vertex_mlp (the literal module composition, bitwise), the C ABI's
three new entry points in the header, the signature table and the library, the workspace rule, and the models'
`fused_head` option."""
import ctypes
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import _select_ref as R
import _vertex_mlp_ref as V
from conftest import ROOT, assert_parity, load_golden

NAMES = ("gcn_vmlp_workspace_bytes", "gcn_vmlp_forward", "gcn_vmlp_backward")


def restated_scores(state, x, adj, d, hierarchical, dtype):
    """The GCN part of _select_ref.generator_scores, then the restated head."""
    p = {k: v.to(dtype) for k, v in state.items()}
    x, adj = x.to(dtype), adj.to(dtype)
    h = x[:, :d]
    for i in (1, 2, 3):
        h = F.relu(torch.sparse.mm(adj, h @ p[f"GCNLayer.gc{i}.weight"]) + p[f"GCNLayer.gc{i}.bias"])
    mlp = {k[len("MLPLayers."):]: v for k, v in p.items() if k.startswith("MLPLayers.")}
    out = V.head(h, x, d, mlp, batch_norm=not hierarchical, skip_last=int(hierarchical))
    if hierarchical:
        return torch.where(x[:, -1] == 0, torch.min(out).expand(out.shape[0]), out.squeeze(1)).unsqueeze(1)
    return out


@pytest.mark.parametrize("tag", ["gen_", "hier_"])
def test_restatement_reproduces_the_fixture(tag):
    g8 = load_golden("g8_generators.npz")
    state, x, adj, d, _ = R.fixture_case(g8, tag)
    s32 = restated_scores(state, x, adj, d, tag == "hier_", torch.float32)
    s64 = restated_scores(state, x, adj, d, tag == "hier_", torch.float64)
    assert_parity(s32.numpy(), g8[tag + "scores"], s64.numpy(), tag + "scores of the restatement")


@pytest.mark.parametrize("batch_norm", [True, False])
@pytest.mark.parametrize("bias", [True, False])
def test_cpu_route_is_the_module_composition(batch_norm, bias):
    from pygcn_amd import functional
    from pygcn_amd.models import GeneratorMLPLayers, MLPLayers
    torch.manual_seed(3)
    n, c, d, t, skip = 70, 5, 4, 3, int(not batch_norm)
    mlp = (GeneratorMLPLayers if batch_norm else MLPLayers)(c + t, 7, 3, 1, bias=bias)
    h = torch.relu(torch.randn(n, c)).requires_grad_()
    x = torch.randn(n, d + t + skip)
    got = functional.vertex_mlp(h, x, d, mlp, batch_norm, skip_last=skip)
    h2 = h.detach().clone().requires_grad_()
    want = mlp(torch.cat((h2, x[:, d:d + t]), dim=1))
    assert got.shape == (n, 1) and torch.equal(got, want)
    ds = torch.randn(n, 1)
    (got * ds).sum().backward()
    grads = {k: p.grad.clone() for k, p in mlp.named_parameters()}
    assert len(grads) == (6 if bias else 3) and all(float(g.abs().max()) > 0 for g in grads.values())
    mlp.zero_grad()
    (want * ds).sum().backward()
    assert torch.equal(h.grad, h2.grad) and float(h.grad.abs().max()) > 0
    for k, p in mlp.named_parameters():
        assert torch.equal(grads[k], p.grad), k
    # the masks of the CPU route: the ReLU derivative of the composition
    _, m1, m2 = functional.vertex_mlp(h.detach(), x, d, mlp, batch_norm, skip_last=skip, return_masks=True)
    params = {k: v.detach() for k, v in mlp.named_parameters()}
    z1, z2 = V.pre_activations(h.detach(), x, d, params, batch_norm, skip)
    assert m1.dtype == torch.int64 and m1.shape == (n,)
    assert torch.equal(V.unpack(m1, 7, torch.bool), z1 > 0) and torch.equal(V.unpack(m2, 3, torch.bool), z2 > 0)
    with pytest.raises(RuntimeError, match="vertex_mlp"):
        functional.vertex_mlp(h, x, x.shape[1] + 1, mlp, batch_norm)


def test_header_table_and_library():
    from pygcn_amd import _native, build
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert re.search(r"#define GCN_ABI_VERSION\s+26\b", hdr) and _native.GCN_ABI_VERSION == 26
    assert _native.lib().gcn_abi_version() == 26
    assert "pygcn/models.py:368-370" in hdr and ":391-393" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in _native.SIGNATURES and name in _native.EXPORTS
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", code)
        assert decl and len(decl.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name
        assert hasattr(raw, name) and getattr(_native.lib(), name).argtypes == _native.SIGNATURES[name][1]
    assert any(src.endswith("gcn_head.hip") for src in build.SRCS)


def test_workspace_rule():
    from pygcn_amd import _native
    ws = _native.lib().gcn_vmlp_workspace_bytes
    assert ws(64, 32, 9, 32, 32) > 0 and ws(64, 1, 0, 1, 1) > 0 and ws(10_000_000, 64, 32, 64, 64) > 0
    for n, c, t, h1, h2 in ((64, 0, 2, 16, 8), (64, 65, 2, 16, 8), (64, 32, 33, 16, 8), (64, 32, -1, 16, 8),
                            (64, 32, 2, 0, 8), (64, 32, 2, 65, 8), (64, 32, 2, 16, 0), (64, 32, 2, 16, 65),
                            (63, 32, 2, 16, 8), (0, 32, 2, 16, 8), (-5, 32, 2, 16, 8)):
        assert ws(n, c, t, h1, h2) == 0, (n, c, t, h1, h2)
    assert ws(2 ** 18, 32, 9, 32, 32) == ws(10_000_000, 32, 9, 32, 32) == ws(2048 * 64, 32, 9, 32, 32)
    assert ws(64, 32, 9, 32, 32) < ws(4099, 32, 9, 32, 32) < ws(2 ** 18, 32, 9, 32, 32)
    # the documented formula (include/gcn_spmm.h), each part rounded up to 16 bytes
    up = lambda b: (b + 15) // 16 * 16        # noqa: E731
    for n, c, t, h1, h2 in ((4099, 32, 9, 32, 32), (150001, 5, 3, 7, 3), (2 ** 18, 8, 1, 64, 8)):
        hp = 16 if max(h1, h2) <= 16 else 32 if max(h1, h2) <= 32 else 64
        b, k = min(-(-n // 64), 2048), c + t
        want = up(b * (1 + 3 * hp) * 8) + up(b * (k + hp) * hp * 4) + up((1 + 3 * hp + (k + hp) * hp) * 8) + 256 * 4
        assert ws(n, c, t, h1, h2) == want


def _config(**kw):
    base = dict(gcn_nfeat=8, gcn_nhid=32, gcn_nclass=32, gcn_dropout=0.0, NN=5, dim_touched=8, linear_nin=34,
                linear_nhid1=16, linear_nhid2=8, linear_nout=1, linear_bias=True)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("name", ["Generator", "Hierarchical_Generator"])
def test_models_take_fused_head(name):
    import pygcn_amd
    cls = getattr(pygcn_amd, name)
    plain = cls(8, 32, 32, 0.0, 5, 34, 16, 8, dim_touched=8)
    fused = cls(8, 32, 32, 0.0, 5, 34, 16, 8, dim_touched=8, fused_head=True)
    assert plain.fused_head is False and fused.fused_head is True
    assert list(plain.state_dict()) == list(fused.state_dict())
    assert list(plain.state_dict())[-6:] == [f"MLPLayers.linear{i}.{w}" for i in (1, 2, 3) for w in ("weight", "bias")]
    fused.load_state_dict(plain.state_dict(), strict=True)
    assert pygcn_amd.get_model(_config(), name).fused_head is False
    assert pygcn_amd.get_model(_config(fused_head=True), name).fused_head is True
    assert type(pygcn_amd.get_model(_config(fused_head=True), name)) is cls


def test_exported():
    from pygcn_amd import functional, head
    assert functional.vertex_mlp is head.vertex_mlp
    assert callable(functional.vertex_mlp)
