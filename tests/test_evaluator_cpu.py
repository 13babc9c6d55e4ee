"""CPU side of the evaluator GCN_OVER_MLP (pygcn_amd/evaluator.py, models.PoolLayer / GCN_OVER_MLP / get_model):
the restatement of the fork's lines (tests/_evaluator_ref.py) against the fixture g9_evaluator.npz, the torch
route of `evaluator_ingest`, `PoolLayer` and `masked_mean_pool(mask_grad=True)` against it, `get_model`, the
state_dict keys, the workspace formula and the binding table.  No GPU needed."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import _evaluator_ref as R
from conftest import ROOT, assert_normwise, load_golden

NAMES = ("gcn_eval_workspace_bytes", "gcn_eval_ingest", "gcn_eval_ingest_backward")
KEYS = [f"GCNLayer.gc{i}.{p}" for i in (1, 2, 3) for p in ("weight", "bias")] + \
       [f"MLPLayers.linear{i}.{p}" for i in (1, 2, 3) for p in ("weight", "bias")]


@pytest.fixture(scope="module")
def g9():
    return load_golden("g9_evaluator.npz")


def g9_case(g9, tag):
    """(state, x, adj, dim_touched) of one fixture case; c_ shares a_'s parameters."""
    ptag = "a_" if tag == "c_" else tag
    state = {name: torch.from_numpy(g9[ptag + "param_" + name]) for name in KEYS}
    adj = torch.sparse_csr_tensor(torch.from_numpy(g9["rowptr"]), torch.from_numpy(g9["col"]).long(),
                                  torch.from_numpy(g9["val"]), (64, 64))
    return state, torch.from_numpy(g9[tag + "x"]), adj, int(g9["dims"][0])


@pytest.mark.parametrize("tag", ["a_", "b_", "c_"])
def test_restatement_reproduces_the_fixture(g9, tag):
    """The imported reference model's output, parameter gradients and flag gradient of out.sum(), at 1e-5."""
    state, x, adj, d = g9_case(g9, tag)
    assert sorted(k for k in g9.files if k.startswith(tag + "grad_")) == sorted(tag + "grad_" + k for k in KEYS)
    out, grads, dflag = R.evaluator_step(state, x, adj, d, torch.float32, lambda o: o.sum())
    assert_normwise(out, g9[tag + "out"], what=f"{tag}out")
    assert_normwise(dflag, g9[tag + "dflag"], what=f"{tag}dflag")
    for name in KEYS:
        assert_normwise(grads[name], g9[tag + "grad_" + name], what=f"{tag}grad {name}")


def literal(x, d, flag=None):
    """The four results of evaluator_ingest written out: the [N, k*d] layout of the GCN's columns, the mask, the
    masked sums of the untouched columns (the pooled part of reference pygcn/models.py:351,272,279 before the
    division) and torch.nonzero's count per sample."""
    k, n, f = x.shape
    m = x[:, :, -1] if flag is None else flag.reshape(k, n)
    wide = torch.stack([x[j, :, :d] for j in range(k)], 1).reshape(n, k * d)
    esum = torch.stack([(x[j, :, d:f - 1] * m[j][:, None]).sum(0) for j in range(k)])
    nonzero = torch.tensor([len(torch.nonzero(m[j], as_tuple=True)[0]) for j in range(k)])
    return wide, m, esum, nonzero


@pytest.mark.parametrize("with_flag", [False, True])
@pytest.mark.parametrize("k,n,f,d", [(1, 1, 2, 1), (3, 37, 17, 8), (3, 37, 9, 8), (3, 37, 5, 0), (1, 37, 9, 8)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_torch_route_of_evaluator_ingest(dtype, k, n, f, d, with_flag):
    from pygcn_amd.functional import evaluator_ingest
    gen = torch.Generator().manual_seed(17)
    x = torch.randn(k, n, f, generator=gen, dtype=dtype)
    x[:, :, -1] = (torch.rand(k, n, generator=gen) < 0.4).to(dtype)
    x[0, 0, -1] = 1.0
    flags = [None]
    if with_flag:
        base = (torch.rand(k, n, generator=gen) < 0.4).to(dtype)
        flags = [base] + ([base.reshape(n), base.reshape(n, 1)] if k == 1 else [])
    cots = (torch.randn(n, k * d, generator=gen, dtype=dtype), torch.randn(k, n, generator=gen, dtype=dtype),
            torch.randn(k, f - 1 - d, generator=gen, dtype=dtype))
    for flag in flags:
        xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
        fa = flag.clone().requires_grad_() if flag is not None else None
        fb = flag.clone().requires_grad_() if flag is not None else None
        got, want = evaluator_ingest(xa, d, fa), literal(xb, d, fb)
        assert got[0].shape == (n, k * d) and got[1].shape == (k, n) and got[2].shape == (k, f - 1 - d)
        assert got[3].dtype == torch.int64 and got[3].shape == (k,)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        for out_a, out_b, cot in zip(got[:3], want[:3], cots):
            if not out_a.requires_grad:
                continue
            ins_a, ins_b = [xa] + ([fa] if flag is not None else []), [xb] + ([fb] if flag is not None else [])
            for ga, gb in zip(torch.autograd.grad(out_a, ins_a, cot, retain_graph=True, allow_unused=True),
                              torch.autograd.grad(out_b, ins_b, cot, retain_graph=True, allow_unused=True)):
                assert (ga is None) == (gb is None) and (ga is None or torch.equal(ga, gb))
        if flag is not None:        # the last column of x is not read: no gradient reaches it
            total = got[1].sum() + got[2].sum()
            assert not bool(torch.autograd.grad(total, xa, retain_graph=True)[0][:, :, -1].any())
    with pytest.raises(RuntimeError, match="flag"):
        evaluator_ingest(x, d, torch.zeros(k + 1, n, dtype=dtype))
    with pytest.raises(RuntimeError, match="k, N, F"):
        evaluator_ingest(x[0], d)
    with pytest.raises(RuntimeError, match="dim_touched"):
        evaluator_ingest(x, f)


def test_a_nan_counts_as_nonzero_and_the_mask_multiplies():
    from pygcn_amd.functional import evaluator_ingest
    x = torch.ones(2, 5, 4)
    x[0, 1, -1] = float("nan")
    x[1, :, -1] = 0.0
    x[1, 2, 1] = float("nan")
    _, _, esum, nonzero = evaluator_ingest(x, 1)
    assert nonzero.tolist() == [5, 0]
    assert torch.isnan(esum).tolist() == [[True, True], [True, False]]       # 0 * NaN = NaN, in its column only


@pytest.mark.parametrize("with_flag", [False, True])
@pytest.mark.parametrize("tag", ["a_", "b_", "c_"])
def test_pool_layer_and_model_pieces_agree_with_the_restatement(g9, tag, with_flag):
    """PoolLayer on the fixture's x is the restated :272,279; the evaluator assembled from the torch routes
    (evaluator_ingest, the restated GCN, masked_mean_pool(mask_grad=True), the restated MLP) gives the
    restatement's output and gradients, with the flag inside x and on its own."""
    from pygcn_amd.functional import evaluator_ingest, masked_mean_pool
    from pygcn_amd.models import PoolLayer
    from test_norm_gpu import fork_forward
    state, x, adj, d = g9_case(g9, tag)
    for dtype in (torch.float32, torch.float64):
        xa, xb = x.to(dtype).detach().requires_grad_(), x.to(dtype).detach().requires_grad_()
        got, want = PoolLayer()(xa), R.pool_layer(xb)
        assert got.shape == (x.shape[0], x.shape[2] - 1)
        assert_normwise(got.detach().numpy(), want.detach().numpy(), rel=1e-6, what="PoolLayer")
        cot = torch.randn(got.shape, generator=torch.Generator().manual_seed(3), dtype=dtype)
        assert_normwise(torch.autograd.grad(got, xa, cot)[0].numpy(), torch.autograd.grad(want, xb, cot)[0].numpy(),
                        rel=1e-6, what="PoolLayer dx")
    k, n, f = x.shape
    flag = (torch.rand(k, n, generator=torch.Generator().manual_seed(4)) < 0.3).float() if with_flag else None
    loss = lambda o: ((o - 0.25) ** 2).mean()      # noqa: E731  (F.mse_loss against a constant)
    want_out, want_grads, want_dflag = R.evaluator_step(state, x, adj, d, torch.float64, loss, flag=flag)
    params = {name: v.double().requires_grad_() for name, v in state.items()}
    gcn = {name[len("GCNLayer."):]: v for name, v in params.items() if name.startswith("GCNLayer.")}
    xin = x.double().detach().requires_grad_(not with_flag)
    fin = flag.double().requires_grad_() if with_flag else None
    wide, mask, esum, nonzero = evaluator_ingest(xin, d, fin)
    assert wide.requires_grad == (not with_flag) and mask.requires_grad
    h = torch.stack([fork_forward(gcn, wide.view(n, k, d)[:, j], adj.double())[0] for j in range(k)])
    pooled = masked_mean_pool(h, mask, count=nonzero[0], mask_grad=True)
    feats = torch.cat((pooled, esum / nonzero[0]), 1)
    out = R.mlp_layers(params, feats)
    loss(out).backward()
    assert_normwise(out.detach().numpy(), want_out, rel=1e-9, what="assembled output")
    assert_normwise((fin.grad if with_flag else xin.grad[:, :, -1]).numpy(), want_dflag, rel=1e-9, what="flag gradient")
    for name in KEYS:
        assert_normwise(params[name].grad.numpy(), want_grads[name], rel=1e-9, what=name)


def test_masked_mean_pool_mask_gradient_on_the_torch_route():
    from pygcn_amd.functional import masked_mean_pool
    gen = torch.Generator().manual_seed(8)
    k, n, c = 3, 41, 6
    h = torch.randn(k, n, c, generator=gen, requires_grad=True)
    mask = (torch.rand(k, n, generator=gen) < 0.4).float().requires_grad_()
    count = (mask[0] != 0).sum()
    cot = torch.randn(k, c, generator=gen)
    out = masked_mean_pool(h, mask, count=count, mask_grad=True)
    dh, dmask = torch.autograd.grad(out, (h, mask), cot)
    coef = cot / count
    assert torch.allclose(dmask, (h.detach() * coef[:, None, :]).sum(2), rtol=1e-6, atol=1e-7)
    assert torch.equal(dh, mask.detach()[:, :, None] * coef[:, None, :].expand(k, n, c))
    # the default: today's behaviour, the mask detached
    plain = masked_mean_pool(h, mask, count=count)
    assert torch.equal(plain, out) and torch.equal(masked_mean_pool(h, mask, count=count, mask_grad=False), out)
    plain.backward(cot)
    assert mask.grad is None and torch.equal(h.grad, dh)
    # a [N, C] input with a [N] mask
    m1 = mask.detach()[0].clone().requires_grad_()
    masked_mean_pool(h[0], m1, mask_grad=True).sum().backward()
    assert m1.grad.shape == (n,) and torch.allclose(m1.grad, h.detach()[0].sum(1) / count, rtol=1e-6, atol=1e-7)


def config(**over):
    base = dict(gcn_nfeat=8, gcn_nhid=32, gcn_nclass=32, gcn_dropout=0.0, NN=5, dim_touched=8, linear_nin=40,
                linear_nhid1=16, linear_nhid2=8, linear_nout=1, linear_bias=True)
    base.update(over)
    return SimpleNamespace(**base)


def test_get_model_returns_the_classes_of_the_fork():
    from pygcn_amd import GCN_OVER_MLP, Generator, Hierarchical_Generator, SoftGenerator, get_model
    from pygcn_amd.models import GCNBatchNorm, MLPLayers, PoolLayer
    ev = get_model(config(), "GNN_OVER_MLP")
    assert type(ev) is GCN_OVER_MLP and ev.dim_touched == 8
    assert isinstance(ev.GCNLayer, GCNBatchNorm) and isinstance(ev.PoolLayer, PoolLayer)
    assert isinstance(ev.MLPLayers, MLPLayers) and ev.MLPLayers.linear1.in_features == 40
    assert ev.GCNLayer.NN == 5 and list(ev.PoolLayer.parameters()) == []
    assert list(ev.state_dict()) == KEYS                                   # the fork's keys: its checkpoints load
    assert list(get_model(config(linear_bias=False), "GNN_OVER_MLP").MLPLayers.state_dict()) == \
        ["linear1.weight", "linear2.weight", "linear3.weight"]
    mlp = get_model(config(linear_nin=16), "MLP")
    assert type(mlp) is nn.Sequential and isinstance(mlp[0], PoolLayer) and isinstance(mlp[1], MLPLayers)
    assert mlp(torch.ones(2, 5, 17)).shape == (2, 1)
    for name, cls in (("Generator", Generator), ("Hierarchical_Generator", Hierarchical_Generator),
                      ("SoftGenerator", SoftGenerator)):
        m = get_model(config(linear_nin=33), name)
        assert type(m) is cls and m.NN == 5 and m.dim_touched == 8
    assert get_model(config(linear_nin=33), "Generator").MLPLayers.linear1.in_features == 33
    assert get_model(config(), "SoftGenerator").PoolMLP.linear1.in_features == 32
    with pytest.raises(TypeError, match="broken in the fork"):
        get_model(config())                                                # the fork's default name
    with pytest.raises(TypeError, match="broken in the fork"):
        get_model(config(), "GCN")
    with pytest.raises(ValueError, match="unknown model name"):
        get_model(config(), "GNN")


def test_model_argument_errors():
    from pygcn_amd import GCN_OVER_MLP
    from pygcn_amd.sharded import ShardedGraph
    m = GCN_OVER_MLP(8, 32, 32, 0.0, 5, 40, 16, 8, 8)
    with pytest.raises(RuntimeError, match="k, N, F"):
        m(torch.zeros(5, 17), torch.eye(5))
    with pytest.raises(RuntimeError, match="ShardedGraph adjacency is not supported"):
        m(torch.zeros(2, 5, 17), object.__new__(ShardedGraph))
    with pytest.raises(RuntimeError, match="ShardedGraph adjacency is not supported"):
        m.GCNLayer.forward_wide(torch.zeros(5, 16), object.__new__(ShardedGraph), 2)


def test_workspace_query_follows_its_documented_formula():
    """gcn_eval_workspace_bytes = B * batch * (F - d) * sizeof(double), B = min(ceil(n / 64), 2048); 0 outside
    2 <= F <= 64, 0 <= d <= F - 1, 1 <= batch <= 65535, n >= 1."""
    from pygcn_amd import _native
    L = _native.lib()
    for n in (1, 64, 65, 129, 4099, 10_000_000):
        for f, d in ((2, 0), (2, 1), (9, 8), (17, 8), (5, 0), (64, 31), (64, 63)):
            for batch in (1, 3, 20, 65535):
                assert L.gcn_eval_workspace_bytes(n, f, d, batch) == min(-(-n // 64), 2048) * batch * (f - d) * 8
    for n, f, d, batch in ((0, 9, 8, 1), (-1, 9, 8, 1), (37, 1, 0, 1), (37, 65, 8, 1), (37, 9, 9, 1), (37, 9, -1, 1),
                           (37, 9, 8, 0), (37, 9, 8, 65536)):
        assert L.gcn_eval_workspace_bytes(n, f, d, batch) == 0


def test_header_declares_the_new_entry_points_at_abi_26():
    from pygcn_amd import _native, build
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert re.search(r"#define GCN_ABI_VERSION\s+26\b", hdr) and _native.GCN_ABI_VERSION == 26
    assert _native.lib().gcn_abi_version() == 26
    assert "pygcn/models.py:333-355" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = __import__("ctypes").CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in _native.SIGNATURES and name in _native.EXPORTS
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", code)
        assert decl and len(decl.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name
        assert hasattr(raw, name) and getattr(_native.lib(), name).argtypes == _native.SIGNATURES[name][1]
    assert any(src.endswith("gcn_eval.hip") for src in build.SRCS)


def test_exports():
    import pygcn_amd
    from pygcn_amd import functional
    assert {"GCN_OVER_MLP", "get_model"} <= set(pygcn_amd.__all__)
    assert callable(functional.evaluator_ingest) and callable(functional.masked_mean_pool)
    x = torch.zeros(2, 3, 4, dtype=torch.float16)
    assert functional.evaluator_ingest(x, 2)[0].dtype == torch.float16          # other dtypes: the torch route
    assert np.array_equal(functional.evaluator_ingest(x.float().permute(0, 2, 1), 1)[3].numpy(), [0, 0])
