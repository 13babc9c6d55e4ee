"""CPU side of the ReLU + BatchNorm feature: the module surface of GCNBatchNorm (the fork's live `GCN`,
reference pygcn/models.py:17-71), the torch fallback of relu_batch_norm, and the header's record of the
new entry points.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT


def test_state_dict_is_the_forks():
    """reference pygcn/models.py:21-26: gc1 (nfeat -> nhid), gc2 (nhid -> nhid), gc3 (nhid -> nclass),
    each a GraphConvolution with weight [in, out] and bias [out]; apply_bn registers nothing."""
    from pygcn_amd import GCNBatchNorm
    m = GCNBatchNorm(nfeat=1433, nhid=16, nclass=7, dropout=0.5, NN=3)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [
        ("gc1.weight", (1433, 16)), ("gc1.bias", (16,)), ("gc2.weight", (16, 16)), ("gc2.bias", (16,)),
        ("gc3.weight", (16, 7)), ("gc3.bias", (7,))]
    assert [n for n, _ in m.named_parameters()] == list(m.state_dict())
    assert not list(m.buffers())
    assert (m.dropout, m.NN) == (0.5, 3) and GCNBatchNorm(8, 4, 3, 0.1).NN is None


def test_seeded_initialisation_is_three_layers_in_order():
    from pygcn_amd import GCNBatchNorm, GraphConvolution
    torch.manual_seed(42)
    m = GCNBatchNorm(32, 16, 7, 0.5)
    torch.manual_seed(42)
    layers = [GraphConvolution(32, 16), GraphConvolution(16, 16), GraphConvolution(16, 7)]
    for i, gc in enumerate(layers, 1):
        np.testing.assert_array_equal(getattr(m, f"gc{i}").weight.detach().numpy(), gc.weight.detach().numpy())
        np.testing.assert_array_equal(getattr(m, f"gc{i}").bias.detach().numpy(), gc.bias.detach().numpy())


def test_cpu_tensor_takes_the_torch_composition():
    from pygcn_amd.functional import relu_batch_norm
    from pygcn_amd.norm import supported
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(37, 16, generator=gen, requires_grad=True)
    w = torch.randn(16, generator=gen, requires_grad=True)
    b = torch.randn(16, generator=gen, requires_grad=True)
    g = torch.randn(37, 16, generator=gen)
    assert not supported(z)
    for relu in (True, False):
        got = relu_batch_norm(z, w, b, eps=1e-3, relu=relu)
        want = F.batch_norm(torch.relu(z) if relu else z, None, None, w, b, True, 0.0, 1e-3)
        assert torch.equal(got, want)
        for a, c in zip(torch.autograd.grad(got, (z, w, b), g), torch.autograd.grad(want, (z, w, b), g)):
            assert torch.equal(a, c)
    assert torch.equal(relu_batch_norm(z), F.batch_norm(torch.relu(z), None, None, None, None, True, 0.0, 1e-5))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        relu_batch_norm(torch.zeros(1, 16))


def test_functional_imports_flat_before_any_other_module():
    """`from functional import ...` with cwd = the package directory, as pygcn_amd/train.py does on its
    first import line (the reference's flat-module convention, pygcn/train.py:15-16)."""
    import subprocess
    import sys
    code = "from functional import nll_loss, relu_batch_norm; from models import GCNBatchNorm; print(GCNBatchNorm(8, 4, 3, 0.5).gc3)"
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(ROOT, "pygcn_amd"),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "GraphConvolution (4 -> 3)" in out.stdout


def test_sharded_adjacency_is_refused():
    from pygcn_amd import GCNBatchNorm
    from pygcn_amd.sharded import ShardedGraph
    m = GCNBatchNorm(8, 4, 3, 0.0)
    with pytest.raises(RuntimeError, match="ShardedGraph"):
        m(torch.zeros(5, 8), object.__new__(ShardedGraph))


def test_workspace_query_follows_the_documented_formula():
    """gcn_bn_workspace_bytes = B * 4 * F * sizeof(double), B = min(ceil(n / 64), 2048); 0 outside the
    shape rule (F a multiple of the 16-byte lane width v with F/v dividing 256, n >= 2)."""
    from pygcn_amd import _native
    L = _native.lib()
    for n in (2, 64, 65, 130, 4099, 10_000_000):
        for nf, dt, v in ((16, 0, 4), (256, 0, 4), (1024, 0, 4), (128, 1, 8), (8, 1, 8)):
            assert L.gcn_bn_workspace_bytes(n, nf, dt) == min(-(-n // 64), 2048) * 4 * nf * 8
    for n, nf, dt in ((1, 16, 0), (0, 16, 0), (37, 7, 0), (37, 24, 0), (37, 2048, 0), (37, 4, 1), (37, 16, 2)):
        assert L.gcn_bn_workspace_bytes(n, nf, dt) == 0


def test_header_records_the_abi_step_and_cites_the_reference():
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert re.search(r"#define GCN_ABI_VERSION\s+26\b", hdr)
    assert "new entry points only; nothing existing changed" in hdr
    assert "pygcn/models.py:49,53" in hdr and "pygcn/models.py:41-45" in hdr
