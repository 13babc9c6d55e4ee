"""CPU side of the batched GCNBatchNorm feature (k samples side by side, [N, k*F]) and of the masked mean
pool: the documented torch compositions, the workspace formulas, the header's record and the message
for a library that lacks a bound symbol.  No GPU needed."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT


def test_cpu_tensor_takes_the_torch_composition_with_repeated_parameters():
    from pygcn_amd.functional import relu_batch_norm
    from pygcn_amd.norm import supported
    gen = torch.Generator().manual_seed(5)
    k, nf = 3, 16
    z = torch.randn(37, k * nf, generator=gen, requires_grad=True)
    w = torch.randn(nf, generator=gen, requires_grad=True)
    b = torch.randn(nf, generator=gen, requires_grad=True)
    g = torch.randn(37, k * nf, generator=gen)
    assert not supported(z, k)
    for relu in (True, False):
        x = torch.relu(z) if relu else z
        got = relu_batch_norm(z, w, b, eps=1e-3, relu=relu, batch=k)
        want = F.batch_norm(x, None, None, w.repeat(k), b.repeat(k), True, 0.0, 1e-3)
        assert torch.equal(got, want)
        grads = torch.autograd.grad(got, (z, w, b), g, retain_graph=True)
        for a, c in zip(grads, torch.autograd.grad(want, (z, w, b), g, retain_graph=True)):
            assert torch.equal(a, c)
        # one BatchNorm1d applied to each sample in turn, sharing weight and bias
        loop = torch.cat([F.batch_norm(x[:, j * nf:(j + 1) * nf], None, None, w, b, True, 0.0, 1e-3)
                          for j in range(k)], 1)
        assert float((got - loop).detach().abs().max()) <= 1e-6 * float(loop.detach().abs().max())
        for a, c in zip(grads, torch.autograd.grad(loop, (z, w, b), g)):
            assert float((a - c).abs().max()) <= 1e-6 * float(c.abs().max())
    assert torch.equal(relu_batch_norm(z, batch=k), F.batch_norm(torch.relu(z), None, None, None, None, True, 0.0, 1e-5))
    with pytest.raises(RuntimeError, match="batch"):
        relu_batch_norm(z, batch=5)              # 48 columns are not 5 windows


def pool_layer(x):
    """reference pygcn/models.py:271-286 (PoolLayer.forward) restated: x [k, N, C + 1], the last feature
    the 0/1 vertex mask; every sample is divided by the vertex count of sample 0."""
    x = (x.permute(2, 1, 0) * x[:, :, -1].T).permute(2, 1, 0)                             # :272 (`.T` of a 3-D tensor)
    return torch.sum(x[:, :, :-1], axis=1) / len(torch.nonzero(x[0, :, -1], as_tuple=True)[0])   # :279


def test_masked_mean_pool_on_the_cpu_is_the_forks_pool_layer():
    from pygcn_amd.functional import masked_mean_pool
    gen = torch.Generator().manual_seed(6)
    k, n, c = 4, 53, 7
    h = torch.randn(k, n, c, generator=gen, requires_grad=True)
    mask = (torch.rand(k, n, generator=gen) < 0.3).float()
    want = pool_layer(torch.cat([h, mask[:, :, None]], 2))
    got = masked_mean_pool(h, mask, count=(mask[0] != 0).sum())
    assert got.shape == (k, c) and torch.equal(got, want)
    cot = torch.randn(k, c, generator=gen)
    assert torch.equal(torch.autograd.grad(got, h, cot)[0], torch.autograd.grad(want, h, cot)[0])
    # the default count is each sample's own; a [N, C] input is one sample
    own = masked_mean_pool(h, mask)
    for j in range(k):
        ref = (h[j] * mask[j][:, None]).sum(0) / (mask[j] != 0).sum()
        assert torch.allclose(own[j], ref, rtol=1e-6, atol=1e-7)
        assert torch.equal(masked_mean_pool(h[j], mask[j]), own[j:j + 1])
    assert torch.equal(masked_mean_pool(h, mask, count=7), masked_mean_pool(h, mask, count=torch.full((k,), 7)))
    with pytest.raises(RuntimeError, match="mask"):
        masked_mean_pool(h, mask[:, :-1])


def test_workspace_queries_follow_their_documented_formulas():
    """gcn_bn_batched_workspace_bytes = batch * gcn_bn_workspace_bytes; gcn_pool_workspace_bytes =
    batch * B * C * sizeof(double), B = min(ceil(n / 64), 2048); 0 outside the rule (the WINDOW width
    obeys it, 1 <= batch <= 65535; the pool takes a single row, BatchNorm does not)."""
    from pygcn_amd import _native
    L = _native.lib()
    for n in (2, 64, 65, 130, 4099, 10_000_000):
        for nf, dt in ((16, 0), (256, 0), (1024, 0), (128, 1), (8, 1)):
            one = L.gcn_bn_workspace_bytes(n, nf, dt)
            assert one == min(-(-n // 64), 2048) * 4 * nf * 8         # (unchanged: tests/test_norm_cpu.py)
            for batch in (1, 3, 20, 65535):
                assert L.gcn_bn_batched_workspace_bytes(n, nf, batch, dt) == batch * one
                assert L.gcn_pool_workspace_bytes(n, nf, batch, dt) == batch * min(-(-n // 64), 2048) * nf * 8
    assert L.gcn_pool_workspace_bytes(1, 16, 3, 0) == 3 * 16 * 8
    for n, nf, batch, dt in ((37, 16, 0, 0), (37, 16, 65536, 0), (37, 16, -1, 0), (37, 7, 3, 0), (37, 24, 3, 0),
                             (37, 2048, 3, 0), (37, 4, 3, 1), (37, 16, 3, 2)):
        assert L.gcn_bn_batched_workspace_bytes(n, nf, batch, dt) == 0
        assert L.gcn_pool_workspace_bytes(n, nf, batch, dt) == 0
    assert L.gcn_bn_batched_workspace_bytes(1, 16, 3, 0) == 0 and L.gcn_pool_workspace_bytes(0, 16, 3, 0) == 0
    for n, nf, dt in ((1, 16, 0), (0, 16, 0), (37, 7, 0), (37, 24, 0), (37, 2048, 0), (37, 4, 1), (37, 16, 2)):
        assert L.gcn_bn_workspace_bytes(n, nf, dt) == 0


def test_header_declares_the_new_entry_points_at_abi_26():
    from pygcn_amd import _native
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert re.search(r"#define GCN_ABI_VERSION\s+26\b", hdr) and _native.GCN_ABI_VERSION == 26
    assert "pygcn/models.py:343-349" in hdr and "pygcn/models.py:267-286" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("gcn_bn_batched_workspace_bytes", "gcn_bn_stats_batched", "gcn_bn_apply_batched",
                 "gcn_bn_backward_sums_batched", "gcn_bn_backward_apply_batched", "gcn_pool_workspace_bytes",
                 "gcn_masked_colsum", "gcn_masked_broadcast"):
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _native.SIGNATURES


def test_a_library_without_a_bound_symbol_is_named(monkeypatch):
    """The additions did not move the ABI number, so an older library passes the version check: binding
    must say which symbol is missing and how to rebuild."""
    from pygcn_amd import _native
    _native.lib()
    table = dict(_native.SIGNATURES)
    table["gcn_not_in_this_library"] = (_native.i, [_native.p])
    monkeypatch.setattr(_native, "SIGNATURES", table)
    monkeypatch.setattr(_native, "_lib", None)
    with pytest.raises(_native.NativeLibraryError, match="gcn_not_in_this_library") as err:
        _native.lib()
    assert "python -m pygcn_amd.build" in str(err.value)
    assert _native._lib is None


def test_sharded_adjacency_is_refused_for_batched_input():
    from pygcn_amd import GCNBatchNorm
    from pygcn_amd.sharded import ShardedGraph
    m = GCNBatchNorm(8, 4, 3, 0.0)
    with pytest.raises(RuntimeError, match="ShardedGraph adjacency is not supported"):
        m(torch.zeros(2, 5, 8), object.__new__(ShardedGraph))
