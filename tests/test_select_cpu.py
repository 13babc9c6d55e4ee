"""CPU side of vertex selection (pygcn_amd/select.py, the generator models): the numpy restatement
(tests/_select_ref.py) — its order against torch's argsort, the law of its race keys — the reference's literal
lines on CPU tensors, the fixture g8_generators.npz, the workspace formula and the binding table.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import _select_ref as R
from conftest import ROOT, assert_normwise, assert_parity, load_golden

NAMES = ("gcn_select_workspace_bytes", "gcn_select_kth", "gcn_select_indices", "gcn_topk_flag", "gcn_race_keys",
         "gcn_race_keys_dev")
P8 = np.array([.30, .22, .15, .12, .09, .06, .04, .02], np.float32)


@pytest.fixture(scope="module")
def g8():
    return load_golden("g8_generators.npz")


def test_restated_order_is_torchs_descending_argsort():
    x = np.array([3, np.nan, 1, 2, 5], np.float32)
    assert torch.argsort(torch.from_numpy(x), descending=True).tolist() == [1, 4, 0, 3, 2]
    assert R.draw_order(x[None], 5)[0].tolist() == [1, 4, 0, 3, 2]
    odd = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.0, -1.0, 3.4e38, -3.4e38], np.float32)
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)
    t = R.order_key(np.concatenate([odd, nans]))
    assert t[0] == t[1] == 0x80000000 and bool((t[10:] == 0xFFFFFFFF).all()) and t[2] == 0xFF800000 and t[3] == 0x007FFFFF
    finite = odd[2:]
    assert np.array_equal(np.argsort(t[2:10], kind="stable"), np.argsort(finite, kind="stable"))
    back = R.key_float(t)
    assert np.array_equal(back[:10].view(np.uint32)[2:], odd.view(np.uint32)[2:]) and back[1].view(np.uint32) == 0
    assert bool((back[10:].view(np.uint32) == 0x7FC00000).all())
    keys = np.array([[2, 7, 7, 1, 7, 0]], np.float32)
    thr, gt = R.kth_largest(keys, 2)
    assert thr[0] == 7 and gt[0] == 0 and R.topk_indices(keys, 2).tolist() == [[1, 2]]
    thr, gt = R.kth_largest(keys, 4)
    assert thr[0] == 2 and gt[0] == 3 and R.topk_indices(keys, 4).tolist() == [[0, 1, 2, 4]]


def test_restated_philox_is_the_published_generator():
    """Known-answer vectors of Random123's kat_vectors for philox4x32-10."""
    zero = R.philox4x32_10(np.zeros((1, 4), np.uint32), (0, 0))[0]
    assert [hex(v) for v in zero] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    ones = R.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    assert [hex(v) for v in ones] == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]


def test_restated_race_has_the_law_of_draws_without_replacement():
    """4096 windows of the same p at seed 42: each vertex's frequency as FIRST pick within 4 sigma of p_r, every
    ordered first-two pair within 4.5 sigma of p_a p_b / (1 - p_a).  (The seed is fixed: 1.13 and 3.13.)"""
    keys = R.race_keys(np.tile(P8, (4096, 1)), 42)
    assert keys.dtype == np.float32 and bool((keys > 0).all())
    order = R.draw_order(keys, 2)
    z1, z2 = R.race_statistics(order[:, 0], order[:, 1], P8)
    print(f"first pick: max {z1:.2f} sigma; ordered pair: max {z2:.2f} sigma")
    assert z1 <= 4.0 and z2 <= 4.5
    assert not np.array_equal(keys, R.race_keys(np.tile(P8, (4096, 1)), 43))
    assert np.array_equal(R.race_keys(P8[None], 42)[0], keys[0]) and not np.array_equal(keys[0], keys[1])
    zero = R.race_keys(np.array([[0.5, 0.0, 0.5, 0.0]], np.float32), 7)
    assert zero[0, 1] == 0 and zero[0, 3] == 0 and not np.signbit(zero[0, 1])
    assert R.draw_order(zero, 4)[0, 2:].tolist() == [1, 3]


def test_topk_flag_on_cpu_is_the_reference_lines():
    from pygcn_amd.functional import topk_flag
    gen = torch.Generator().manual_seed(11)
    for dtype in (torch.float32, torch.float64):
        s = torch.randn(53, 1, generator=gen, dtype=dtype, requires_grad=True)
        g = torch.randn(53, 1, generator=gen, dtype=dtype)
        for nn_ in (0, 5, 52):
            want, got = R.literal_flag(s, nn_), topk_flag(s, nn_)
            assert got.shape == (53, 1) and torch.equal(got, want) and int((got != 0).sum()) == nn_
            assert torch.equal(torch.autograd.grad(got, s, g)[0], torch.autograd.grad(want, s, g)[0])
            flat = topk_flag(s.detach().view(53), nn_)
            assert flat.shape == (53,) and torch.equal(flat, want.detach().view(53))
    rows = torch.randn(3, 53, generator=gen)
    got = topk_flag(rows, 7)
    assert got.shape == (3, 53)
    for j in range(3):
        assert torch.equal(got[j], R.literal_flag(rows[j].view(-1, 1), 7).view(-1))
    tied = torch.tensor([1.0, 3.0, 3.0, 2.0, 0.5])       # ties at the threshold are not selected
    assert topk_flag(tied, 1).tolist() == [0, 0, 0, 0, 0] and topk_flag(tied, 2).tolist() == [0, 1, 1, 0, 0]
    for bad in (-1, 5):
        with pytest.raises(RuntimeError, match="0 <= NN <= N - 1"):
            topk_flag(tied, bad)
    with pytest.raises(RuntimeError, match="neither"):
        topk_flag(torch.zeros(2, 3, 4), 1)


def test_selection_log_prob_is_categoricals(g8):
    from pygcn_amd.functional import sample_without_replacement, selection_log_prob
    gen = torch.Generator().manual_seed(12)
    w = torch.rand(3, 40, generator=gen, dtype=torch.float64) + 0.01      # not normalised: Categorical normalises
    idx = torch.stack([torch.randperm(40, generator=gen)[:6] for _ in range(3)])
    for dtype, tol in ((torch.float64, 1e-13), (torch.float32, 1e-6)):
        p = w.to(dtype).clone().requires_grad_()
        got = selection_log_prob(p, idx)
        assert got.shape == (3,) and got.dtype == dtype
        p64 = w.detach().clone().requires_grad_()
        want = torch.stack([torch.distributions.Categorical(p64[j]).log_prob(idx[j]).sum() for j in range(3)])
        assert_normwise(got.detach().numpy(), want.detach().numpy(), rel=tol, what=f"log-prob {dtype}")
        got.sum().backward()
        want.sum().backward()
        assert_normwise(p.grad.numpy(), p64.grad.numpy(), rel=max(tol, 1e-12) * 10, what=f"log-prob gradient {dtype}")
    one = selection_log_prob(w[0], idx[0])
    assert one.shape == () and float(one.detach()) == pytest.approx(float(want[0].detach()), rel=1e-12)
    # the fork's own loop over g7's attention, recorded in the fixture
    g7 = load_golden("g7_soft_generator.npz")
    lp = selection_log_prob(torch.from_numpy(g7["attn"]), torch.from_numpy(g8["g7_picked"]))
    assert_normwise(float(lp), float(g8["g7_log_prob"].reshape(())), rel=1e-6, what="g7 log-prob")
    picks = sample_without_replacement(torch.from_numpy(P8), 5)           # CPU: torch.multinomial
    assert picks.shape == (5,) and picks.dtype == torch.int64 and len(set(picks.tolist())) == 5
    with pytest.raises(RuntimeError, match="1 <= NN <= N"):
        sample_without_replacement(torch.from_numpy(P8), 9)


def test_fixture_matches_the_restatement(g8):
    """The reference's own run against tests/_select_ref.py, so the GPU tests may use the restatement (and its
    float64) where the reference does not exist; and the margin that keeps the chosen set stable."""
    for tag, hier in (("gen_", False), ("hier_", True)):
        state, x, adj, d, nn_ = R.fixture_case(g8, tag)
        assert x.shape == (64, 10) and d == 8 and nn_ == 5 and len(state) == 12
        s32, f32, g32 = R.generator_step(state, x, adj, d, nn_, torch.float32, hier)
        s64, f64, g64 = R.generator_step(state, x, adj, d, nn_, torch.float64, hier)
        assert_parity(g8[tag + "scores"], s32, s64, tag + "scores")
        R.assert_flag_exact(f32, s32, g8[tag + "vac_flag"], nn_, tag + "restated flag")
        R.assert_flag_exact(g8[tag + "vac_flag"], g8[tag + "scores"], g8[tag + "vac_flag"], nn_, tag + "fixture flag")
        assert np.array_equal(f32 != 0, f64 != 0)
        for name in state:
            assert_parity(g8[tag + "grad_" + name], g32[name], g64[name], tag + "grad " + name)
        top = np.sort(g8[tag + "scores"].ravel())[::-1]
        assert top[nn_ - 1] - top[nn_] >= 1e-3 * np.abs(top).max()


class TorchTrunk(nn.Module):
    """GCNStack's parameters under torch's CPU sparse product: the GraphConvolution layers have no CPU path, so
    the models' own lines after the trunk are run on CPU tensors over this stand-in."""

    def __init__(self, stack):
        super().__init__()
        self.gc1, self.gc2, self.gc3 = stack.gc1, stack.gc2, stack.gc3

    def forward(self, x, adj):
        for gc in (self.gc1, self.gc2, self.gc3):
            x = torch.relu(torch.sparse.mm(adj, x @ gc.weight) + gc.bias)
        return x


@pytest.mark.parametrize("tag", ["gen_", "hier_"])
def test_models_on_cpu_reproduce_the_fixture(g8, tag):
    import pygcn_amd
    from pygcn_amd.models import GCNStack, GeneratorMLPLayers, MLPLayers
    from pygcn_amd.sharded import ShardedGraph
    state, x, adj, d, nn_ = R.fixture_case(g8, tag)
    dims = [int(v) for v in g8["dims"]]
    cls = pygcn_amd.Generator if tag == "gen_" else pygcn_amd.Hierarchical_Generator
    nin = dims[2] + x.shape[1] - d - (tag == "hier_")
    model = cls(dims[0], dims[1], dims[2], 0.0, nn_, nin, dims[3], dims[4], dim_touched=d)
    assert list(model.state_dict()) == list(state)
    model.load_state_dict(state, strict=True)
    assert isinstance(model.GCNLayer, GCNStack) and model.NN == nn_ and model.dim_touched == d
    assert isinstance(model.MLPLayers, GeneratorMLPLayers if tag == "gen_" else MLPLayers)
    with pytest.raises(RuntimeError, match="ShardedGraph adjacency is not supported"):
        model(x, object.__new__(ShardedGraph))
    model.GCNLayer = TorchTrunk(model.GCNLayer)
    scores = model.scores(x, adj)
    flag = model(x, adj)
    assert scores.shape == (64, 1) and flag.shape == (64, 1)
    assert_normwise(scores.detach().numpy(), g8[tag + "scores"], what=tag + "scores on CPU")
    R.assert_flag_exact(flag.detach().numpy(), scores.detach().numpy(), g8[tag + "vac_flag"], nn_, tag + "flag on CPU")
    flag.sum().backward()
    params = dict(model.named_parameters())
    for name in state:
        assert_normwise(params[name].grad.numpy(), g8[tag + "grad_" + name], what=tag + "grad " + name + " on CPU")


def test_mlp_stacks_are_the_forks_lines():
    import torch.nn.functional as F
    from pygcn_amd.models import GeneratorMLPLayers, MLPLayers
    torch.manual_seed(3)
    x = torch.randn(37, 11)
    plain, bn = MLPLayers(11, 16, 8), GeneratorMLPLayers(11, 16, 8, bias=True)
    want = plain.linear3(F.relu(plain.linear2(F.relu(plain.linear1(x)))))
    assert torch.equal(plain(x), want) and want.shape == (37, 1)
    fresh = lambda t: nn.BatchNorm1d(t.size()[1])(t)     # noqa: E731  (the fork's apply_bn, without .cuda())
    want = bn.linear3(fresh(F.relu(bn.linear2(fresh(F.relu(bn.linear1(x)))))))
    assert torch.equal(bn.eval()(x), want)               # batch statistics under eval() too, as the fork
    assert list(bn.state_dict()) == [f"linear{i}.{w}" for i in (1, 2, 3) for w in ("weight", "bias")]
    assert MLPLayers(4, 3, 2, bias=False).linear1.bias is None


def test_soft_generator_policy_methods_exist_and_forward_is_unchanged():
    from pygcn_amd import SoftGenerator
    m = SoftGenerator(8, 4, 4, 0.0, 5, 3, 3)
    assert callable(m.select_action) and callable(m.log_prob)
    assert list(m.state_dict()) == [f"GCN.gc{i}.{w}" for i in (1, 2, 3) for w in ("weight", "bias")] + \
        [f"PoolMLP.linear{i}.{w}" for i in (1, 2, 3) for w in ("weight", "bias")]


def test_workspace_query_follows_its_documented_formula():
    from pygcn_amd import _native
    L = _native.lib()
    for n in (1, 1024, 1025, 2050, 1024 * 1024, 1024 * 1024 + 37, 2 ** 31 - 1):
        for batch in (1, 3):
            want = batch * (3 * 2048 + 8 + 2 * min(-(-n // 1024), 1024)) * 4
            assert L.gcn_select_workspace_bytes(n, batch) == want, (n, batch)
    for n, batch in ((0, 1), (2 ** 31, 1), (37, 0), (37, 65536)):
        assert L.gcn_select_workspace_bytes(n, batch) == 0, (n, batch)
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert "gcn_select_workspace_bytes = batch * (3 * 2048 + 8 + 2 * B) * sizeof(int32_t)" in hdr


def test_binding_table_and_library_have_the_entry_points():
    import ctypes
    from pygcn_amd import _native, build
    hdr = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(_native.LIB_PATH)
    L = _native.lib()
    for name in NAMES:
        assert name in _native.SIGNATURES and name in _native.EXPORTS
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", code)
        assert decl and len(decl.group(1).split(",")) == len(_native.SIGNATURES[name][1]), name
        assert hasattr(raw, name) and getattr(L, name).argtypes == _native.SIGNATURES[name][1]
    assert any(src.endswith("gcn_select.hip") for src in build.SRCS)
    assert "pygcn/models.py:373-377" in hdr and "rl-policy-generator.py:324-336" in hdr
