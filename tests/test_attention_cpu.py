"""CPU side of the vertex-attention readout (the head of the fork's SoftGenerator, reference
pygcn/models.py:289-329, 412-433): the fixture against the torch restatement, the model's state_dict, the
documented torch compositions, the workspace formula and the binding table.  No GPU needed."""
import os
import re

import pytest
import torch

import _attention_ref as R
from conftest import ROOT, assert_normwise, assert_parity, load_golden

NAMES = ("gcn_attn_workspace_bytes", "gcn_attn_scores", "gcn_attn_normalize", "gcn_attn_backward")


@pytest.fixture(scope="module")
def g7():
    return load_golden("g7_soft_generator.npz")


def test_fixture_matches_the_restatement(g7):
    """The reference's own run (the fixture) against tests/_attention_ref.py: the restatement IS the fork's
    arithmetic, so the GPU tests may use it where the reference does not exist."""
    state, x, adj, d, picked, reward = R.fixture_case(g7)
    assert x.shape == (64, 10) and d == 8 and g7["attn"].shape == (64,)
    attn32, grads32 = R.reinforce_step(state, x, adj, d, picked, reward, torch.float32)
    attn64, grads64 = R.reinforce_step(state, x, adj, d, picked, reward, torch.float64)
    assert_normwise(g7["attn"], attn32, what="g7 attn vs float32 restatement")
    assert_parity(g7["attn"], attn32, attn64, "g7 attn")
    assert sorted(grads32) == sorted(state) and len(state) == 12
    for name in state:
        assert_normwise(g7["grad_" + name], grads32[name], what=f"g7 grad {name} vs float32 restatement")
        assert_parity(g7["grad_" + name], grads32[name], grads64[name], f"g7 grad {name}")
    assert abs(float(g7["attn"].sum(dtype="float64")) - 1.0) < 1e-6


def test_state_dict_is_the_forks(g7):
    from pygcn_amd import SoftGenerator
    from pygcn_amd.models import GCNStack
    d, nhid, nclass, nhid1, nhid2, nn_ = (int(v) for v in g7["dims"])
    model = SoftGenerator(d, nhid, nclass, 0.0, nn_, nhid1, nhid2, dim_touched=d)
    want = {name[len("param_"):]: g7[name] for name in g7.files if name.startswith("param_")}
    got = model.state_dict()
    assert list(got) == list(want)
    for name, v in want.items():
        assert tuple(got[name].shape) == v.shape and got[name].dtype == torch.float32, name
    model.load_state_dict({k: torch.from_numpy(v) for k, v in want.items()}, strict=True)
    assert isinstance(model.GCN, GCNStack) and model.GCN.nlayers == 3
    assert model.NN == nn_ and model.dim_touched == d
    assert model.saved_log_probs == [] and model.rewards == []
    model.saved_log_probs.append(1.0)                    # plain lists, as the fork's driver uses them
    assert "saved_log_probs" not in model.state_dict()
    nobias = SoftGenerator(d, nhid, nclass, 0.0, nn_, nhid1, nhid2, linear_bias=False)
    assert nobias.PoolMLP.linear1.bias is None and nobias.dim_touched is None


def test_sharded_adjacency_is_refused():
    from pygcn_amd import SoftGenerator
    from pygcn_amd.sharded import ShardedGraph
    m = SoftGenerator(8, 4, 4, 0.0, 5, 3, 3)
    with pytest.raises(RuntimeError, match="ShardedGraph adjacency is not supported"):
        m(torch.zeros(5, 8), object.__new__(ShardedGraph))


def test_cpu_tensors_take_the_literal_composition():
    from pygcn_amd.functional import vertex_attention, vertex_mean
    gen = torch.Generator().manual_seed(7)
    n, c, k = 53, 32, 3
    h = torch.randn(n, c, generator=gen, requires_grad=True)
    key = torch.randn(c, generator=gen, requires_grad=True)
    g = torch.randn(n, generator=gen)
    want = torch.softmax((h * key).sum(-1), dim=-1)
    for kk in (key, key.view(1, c)):
        got = vertex_attention(h, kk)
        assert got.shape == (n,) and torch.equal(got, want)
        for a, b in zip(torch.autograd.grad(got, (h, key), g), torch.autograd.grad(want, (h, key), g, retain_graph=True)):
            assert torch.equal(a, b)
    assert torch.equal(want, R.head(h, key.view(1, c)))   # the fork's torch.mul(key, x).sum(dim=1), softmax over dim 0
    mean = vertex_mean(h)
    assert mean.shape == (1, c) and torch.equal(mean, torch.mean(h, dim=0).unsqueeze(0))
    # [k, N, C] with one key per sample, contiguous or the permuted view of [N, k*C] storage
    store = torch.randn(n, k * c, generator=gen)
    for h3 in (torch.randn(k, n, c, generator=gen), store.view(n, k, c).permute(1, 0, 2)):
        key3 = torch.randn(k, c, generator=gen)
        got = vertex_attention(h3, key3)
        assert got.shape == (k, n)
        assert torch.equal(got, torch.softmax((h3 * key3[:, None, :]).sum(-1), dim=-1))
        for j in range(k):
            assert torch.allclose(got[j], vertex_attention(h3[j], key3[j]), rtol=1e-6, atol=1e-9)
        assert vertex_mean(h3).shape == (k, c) and torch.equal(vertex_mean(h3), h3.mean(-2))
    # float64 and an odd width are the same composition
    h7 = torch.randn(n, 7, generator=gen, dtype=torch.float64)
    k7 = torch.randn(7, generator=gen, dtype=torch.float64)
    assert torch.equal(vertex_attention(h7, k7), torch.softmax((h7 * k7).sum(-1), dim=-1))
    with pytest.raises(RuntimeError, match="key"):
        vertex_attention(h, torch.zeros(c + 1))
    with pytest.raises(RuntimeError, match="key"):
        vertex_attention(h3, torch.zeros(c))
    with pytest.raises(RuntimeError, match="vertex_mean"):
        vertex_mean(torch.zeros(4))


def test_workspace_query_follows_its_documented_formula():
    """gcn_attn_workspace_bytes = batch * B * max(C, 2) * sizeof(double), B = min(ceil(n / 64), 2048);
    0 outside the rule."""
    from pygcn_amd import _native
    L = _native.lib()
    for n in (1, 64, 65, 131072, 131073):
        for c in (4, 32, 256):
            for batch in (1, 3):
                want = batch * min(-(-n // 64), 2048) * max(c, 2) * 8
                assert L.gcn_attn_workspace_bytes(n, c, batch, 0) == want, (n, c, batch)
    assert L.gcn_attn_workspace_bytes(37, 128, 3, 1) == 3 * 128 * 8
    for n, c, batch, dt in ((0, 32, 1, 0), (37, 6, 1, 0), (37, 2048, 1, 0), (37, 32, 0, 0), (37, 32, 65536, 0),
                            (37, 4, 1, 1), (37, 32, 1, 2)):
        assert L.gcn_attn_workspace_bytes(n, c, batch, dt) == 0, (n, c, batch, dt)
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert "gcn_attn_workspace_bytes = batch * B * max(C, 2) * sizeof(double)" in hdr


def test_binding_table_and_library_have_the_four_entry_points():
    import ctypes
    from pygcn_amd import _native
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    for name in NAMES:
        assert name in _native.SIGNATURES and name in _native.EXPORTS
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", code)
        assert decl and len(decl.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name
        assert hasattr(raw, name) and getattr(L, name).argtypes == _native.SIGNATURES[name][1]
    assert "pygcn/models.py:324-329" in hdr
