"""functional.vertex_mlp on the device (pygcn_amd/csrc/gcn_head.hip): scores, dh and every parameter gradient
against float64 — the restatement tests/_vertex_mlp_ref.py evaluated with the DEVICE's ReLU masks, after asserting
that those differ from float64's own only at the ReLU boundary (tests/_sampling.py::device_relu_mask says why) —
the fixture g8_generators.npz through both generator models with fused_head=True, the edges of the shape rule,
run-to-run reproducibility, peak memory, host synchronisation, non-finite input and the C ABI's argument errors."""
import functools

import numpy as np
import pytest
import torch

import _select_ref as R
import _vertex_mlp_ref as V
from conftest import assert_parity, load_golden
from test_select_gpu import LaunchSpy, count_host_syncs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 8                                    # leading columns of x that must not be read: NaN

# one full tile; a one-row tail tile; many blocks with a partial tile; a block that walks more than one tile
# (64-row tiles, <= 2048 blocks: 150001 rows are 2344 tiles)
SIZES = (64, 65, 4099, 150001)
# a WAVE that walks more than one tile: a block's waves take the tiles of its slab in turn, so a slab must hold
# more tiles than the block has waves — 600001 rows are 9376 tiles, 5 per block: with 4 waves (HP <= 32) wave 0
# walks two, with the 2 waves a block has at HP = 64 they walk three and two
LONG = 600001
WIDTHS = ((32, 2, 16, 8), (32, 9, 32, 32), (8, 1, 64, 8), (32, 0, 32, 32), (5, 3, 7, 3))


def make_mlp(c, t, h1, h2, batch_norm, bias, seed):
    from pygcn_amd.models import GeneratorMLPLayers, MLPLayers
    torch.manual_seed(seed)
    return (GeneratorMLPLayers if batch_norm else MLPLayers)(c + t, h1, h2, 1, bias=bias)    # U(+-1/sqrt(fan_in))


def make_inputs(n, c, t, skip_last=0):
    g = torch.Generator().manual_seed(1234 + n)
    h = torch.relu(torch.randn(n, c, generator=g))
    x = torch.randn(n, D + t + skip_last, generator=g)
    x[:, :D] = float("nan")
    if skip_last:
        x[:, -skip_last:] = float("nan")
    ds = torch.randn(n, 1, generator=g)
    return h, x, ds


def device_step(mlp, h, x, ds, batch_norm, skip_last=0, return_masks=True):
    """(scores, dh, {name: grad}, masks) of one forward + backward of (scores * ds).sum() on the device."""
    from pygcn_amd.functional import vertex_mlp
    mlp.zero_grad()
    hd = h.to(DEV).requires_grad_()
    out = vertex_mlp(hd, x.to(DEV), D, mlp, batch_norm, skip_last=skip_last, return_masks=return_masks)
    scores, masks = (out[0], out[1:]) if return_masks else (out, None)
    (scores * ds.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return scores.detach(), hd.grad, {k: p.grad.clone() for k, p in mlp.named_parameters()}, masks


def reference_step(mlp_cpu, h, x, ds, batch_norm, skip_last, masks, dtype):
    """The restatement in `dtype` on the CPU, with the device's masks when given."""
    params = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in mlp_cpu.named_parameters()}
    hh = h.to(dtype).clone().requires_grad_()
    scores = V.head(hh, x.to(dtype), D, params, batch_norm, skip_last, masks)     # (the NaN columns are never read)
    (scores * ds.to(dtype)).sum().backward()
    return scores.detach().numpy(), hh.grad.numpy(), {k: p.grad.numpy() for k, p in params.items()}


def check_parity(n, widths, batch_norm, bias, skip_last=0):
    import copy
    c, t, h1, h2 = widths
    mlp_cpu = make_mlp(c, t, h1, h2, batch_norm, bias, seed=n + 7 * c + h1)
    h, x, ds = make_inputs(n, c, t, skip_last)
    mlp = copy.deepcopy(mlp_cpu).to(DEV)
    spy_names = []
    from pygcn_amd import _native
    real = _native.launch
    _native.launch = lambda name, *a, **kw: (spy_names.append(name), real(name, *a, **kw))[1]
    try:
        scores, dh, grads, (m1, m2) = device_step(mlp, h, x, ds, batch_norm, skip_last)
    finally:
        _native.launch = real
    assert spy_names == ["gcn_vmlp_forward", "gcn_vmlp_backward"], spy_names
    assert scores.shape == (n, 1) and dh.shape == (n, c) and m1.dtype == torch.int64 and m1.shape == (n,)
    # float64's own pre-activations: the device's masks may differ only at the ReLU boundary
    p64 = {k: v.detach().double() for k, v in mlp_cpu.named_parameters()}
    z1, z2 = V.pre_activations(h.double(), x.double(), D, p64, batch_norm, skip_last)
    k1, f1 = V.assert_masks_near(m1.cpu(), z1, "layer 1")
    k2, f2 = V.assert_masks_near(m2.cpu(), z2, "layer 2")
    s64, dh64, g64 = reference_step(mlp_cpu, h, x, ds, batch_norm, skip_last, (k1, k2), torch.float64)
    # ref32: the torch float32 composition on the CPU (its own masks, torch's fp32 batch statistics)
    from pygcn_amd.functional import vertex_mlp
    mlp_cpu.zero_grad()
    h32 = h.clone().requires_grad_()
    s32 = vertex_mlp(h32, x, D, mlp_cpu, batch_norm, skip_last=skip_last)
    (s32 * ds).sum().backward()
    what = f"n={n} widths={widths} bn={batch_norm} bias={bias}"
    print(f"{what}: mask flips {f1}, {f2}")
    assert_parity(scores.cpu().numpy(), s32.detach().numpy(), s64, what + " scores")
    assert_parity(dh.cpu().numpy(), h32.grad.numpy(), dh64, what + " dh")
    assert sorted(grads) == sorted(g64) and len(grads) == (6 if bias else 3)
    for k, p in mlp_cpu.named_parameters():
        assert_parity(grads[k].cpu().numpy(), p.grad.numpy(), g64[k], f"{what} grad {k}")


@pytest.mark.parametrize("batch_norm", [True, False], ids=["bn", "plain"])
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "x".join(map(str, w)))
@pytest.mark.parametrize("n", SIZES)
def test_parity_against_float64(n, widths, batch_norm):
    check_parity(n, widths, batch_norm, bias=True)


@pytest.mark.parametrize("batch_norm", [True, False], ids=["bn", "plain"])
@pytest.mark.parametrize("widths", ((32, 9, 32, 32), (8, 1, 64, 8)), ids=lambda w: "x".join(map(str, w)))
def test_parity_where_a_wave_walks_several_tiles(widths, batch_norm):
    """The state a wave carries from tile to tile — the fp32 outer-product registers, the double column sums, the
    reused LDS tiles — against float64, at the smallest N that has it (LONG)."""
    check_parity(LONG, widths, batch_norm, bias=True)


@pytest.mark.parametrize("batch_norm", [True, False], ids=["bn", "plain"])
def test_without_a_gradient_for_h(batch_norm):
    """h without requires_grad: the backward sweep is handed no dh and skips it; the parameter gradients are bit for
    bit those of the call that forms dh."""
    from pygcn_amd.functional import vertex_mlp
    n, (c, t, h1, h2) = 4099, (32, 9, 32, 32)
    mlp = make_mlp(c, t, h1, h2, batch_norm, True, seed=5).to(DEV)
    h, x, ds = make_inputs(n, c, t)
    _, dh, want, _ = device_step(mlp, h, x, ds, batch_norm)
    assert dh is not None and float(dh.abs().max()) > 0
    mlp.zero_grad()
    (vertex_mlp(h.to(DEV), x.to(DEV), D, mlp, batch_norm) * ds.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    for k, p in mlp.named_parameters():
        assert torch.equal(p.grad, want[k]), k


@pytest.mark.parametrize("batch_norm", [True, False], ids=["bn", "plain"])
@pytest.mark.parametrize("n", (65, 4099))
def test_parity_without_bias_and_with_a_skipped_last_column(n, batch_norm):
    check_parity(n, (32, 2, 16, 8), batch_norm, bias=False)
    check_parity(n, (32, 2, 16, 8), batch_norm, bias=True, skip_last=1)


# ------------------------------------------------------------------------------------------------ fixture
@pytest.mark.parametrize("tag", ["gen_", "hier_"])
def test_generators_with_the_fused_head_against_the_fixture(monkeypatch, tag):
    """tests/test_select_gpu.py::test_generators_against_the_fixture with fused_head=True: the same gates, and
    the launches are the fused sweeps' — no ReLU + BatchNorm sweep of pygcn_amd/norm.py."""
    import pygcn_amd
    from pygcn_amd import CSRGraph
    g8 = load_golden("g8_generators.npz")
    hier = tag == "hier_"
    state, x, adj, d, nn_ = R.fixture_case(g8, tag)
    dims = [int(v) for v in g8["dims"]]
    cls = pygcn_amd.Hierarchical_Generator if hier else pygcn_amd.Generator
    model = cls(dims[0], dims[1], dims[2], 0.0, nn_, dims[2] + x.shape[1] - d - hier, dims[3], dims[4], dim_touched=d,
                fused_head=True)
    model.load_state_dict(state, strict=True)
    model = model.to(DEV).train()
    n = x.shape[0]
    graph = CSRGraph(torch.from_numpy(g8["rowptr"]).to(DEV), torch.from_numpy(g8["col"]).to(DEV),
                     torch.from_numpy(g8["val"]).to(DEV), (n, n))
    spy = LaunchSpy(monkeypatch)
    scores = model.scores(x.to(DEV), graph)
    flag = model(x.to(DEV), graph)
    flag.sum().backward()
    torch.cuda.synchronize()
    for name in ("gcn_select_kth", "gcn_topk_flag", "gcn_vmlp_forward", "gcn_vmlp_backward"):
        assert name in spy.names(), (name, spy.names())
    assert not [name for name in spy.names() if name.startswith("gcn_bn_")], spy.names()
    assert flag.shape == (n, 1) and flag.dtype == torch.float32
    s64, f64, g64 = R.generator_step(state, x, adj, d, nn_, torch.float64, hier)
    assert_parity(scores.detach().cpu().numpy(), g8[tag + "scores"], s64, tag + "scores, fused head")
    R.assert_flag_exact(flag.detach().cpu().numpy(), scores.detach().cpu().numpy(), g8[tag + "vac_flag"], nn_,
                        tag + "flag, fused head")
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(state)
    for name in state:
        assert_parity(params[name].grad.cpu().numpy(), g8[tag + "grad_" + name], g64[name],
                      f"{tag}grad {name}, fused head")


# --------------------------------------------------------------------------------------------- rule edges
@pytest.mark.parametrize("edge", ["n63", "h65", "float16", "x_requires_grad"])
@pytest.mark.parametrize("batch_norm", [True, False], ids=["bn", "plain"])
def test_outside_the_rule_is_the_module_composition(monkeypatch, edge, batch_norm):
    from pygcn_amd.functional import vertex_mlp
    n, c, t, h1, h2 = (63 if edge == "n63" else 200), 32, 2, (65 if edge == "h65" else 16), 8
    mlp = make_mlp(c, t, h1, h2, batch_norm, True, seed=11).to(DEV)
    h, x, ds = make_inputs(n, c, t)
    x = torch.nan_to_num(x, nan=0.5)                       # (x.requires_grad: its gradient is compared too)
    dtype = torch.float16 if edge == "float16" else torch.float32
    mlp = mlp.to(dtype)

    def step(fn):
        mlp.zero_grad()
        hd = h.to(DEV, dtype).requires_grad_()
        xd = x.to(DEV, dtype).requires_grad_(edge == "x_requires_grad")
        s = fn(hd, xd)
        (s * ds.to(DEV, dtype)).sum().backward()
        return [s.detach(), hd.grad, xd.grad] + [p.grad.clone() for p in mlp.parameters()]
    spy = LaunchSpy(monkeypatch)
    got = step(lambda hd, xd: vertex_mlp(hd, xd, D, mlp, batch_norm))
    assert not [name for name in spy.names() if name.startswith("gcn_vmlp_")], spy.names()
    want = step(lambda hd, xd: mlp(torch.cat((hd, xd[:, D:]), dim=1)))
    for a, b in zip(got, want):
        assert (a is None and b is None) or torch.equal(a, b)


# ----------------------------------------------------------------------------- reproducibility, memory, syncs
def test_bitwise_reproducible():
    n, (c, t, h1, h2) = 150001, (32, 9, 32, 32)
    mlp = make_mlp(c, t, h1, h2, True, True, seed=5).to(DEV)
    h, x, ds = make_inputs(n, c, t)
    runs = [device_step(mlp, h, x, ds, True) for _ in range(2)]
    (s0, dh0, g0, m0), (s1, dh1, g1, m1) = runs
    assert torch.equal(s0, s1) and torch.equal(dh0, dh1) and torch.equal(m0[0], m1[0]) and torch.equal(m0[1], m1[1])
    assert len(g0) == 6 and all(torch.equal(g0[k], g1[k]) for k in g0)


def test_peak_memory_holds_no_hidden_activation():
    """Forward + backward at N = 2^18 allocate the scores, dh and the workspace and small change — the torch route
    keeps five [N, 32] tensors (168 MB) and cannot meet the bound."""
    from pygcn_amd import _native
    from pygcn_amd.functional import vertex_mlp
    n, (c, t, h1, h2) = 2 ** 18, (32, 9, 32, 32)
    mlp = make_mlp(c, t, h1, h2, True, True, seed=5).to(DEV)
    h, x, ds = make_inputs(n, c, t)
    hd, xd, dsd = h.to(DEV).requires_grad_(), x.to(DEV), ds.to(DEV)
    (vertex_mlp(hd, xd, D, mlp, True) * dsd).sum().backward()         # (first use: the parameters' .grad exist)
    hd.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    (vertex_mlp(hd, xd, D, mlp, True) * dsd).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    bound = n * c * 4 + n * 4 + _native.lib().gcn_vmlp_workspace_bytes(n, c, t, h1, h2) + (8 << 20)
    print(f"peak above the live bytes {peak}, bound {bound}")
    assert peak <= bound, (peak, bound)


def test_no_host_synchronisation():
    from pygcn_amd.functional import vertex_mlp
    n, (c, t, h1, h2) = 4099, (32, 9, 32, 32)
    h, x, ds = make_inputs(n, c, t)
    for batch_norm in (True, False):
        mlp = make_mlp(c, t, h1, h2, batch_norm, True, seed=5).to(DEV)
        hd, xd, dsd = h.to(DEV).requires_grad_(), x.to(DEV), ds.to(DEV)
        (vertex_mlp(hd, xd, D, mlp, batch_norm) * dsd).sum().backward()      # (first use)
        kept = []
        assert count_host_syncs(lambda: kept.append(vertex_mlp(hd, xd, D, mlp, batch_norm, return_masks=True)[0])) == 0
        assert count_host_syncs(lambda: (kept[0] * dsd).sum().backward()) == 0


# ------------------------------------------------------------------------------------------ non-finite input
def test_nan_rows():
    from pygcn_amd.functional import vertex_mlp
    n, (c, t, h1, h2), r = 4099, (32, 9, 32, 32), 3000
    h, x, _ = make_inputs(n, c, t)
    bad = h.clone()
    bad[r, 5] = float("nan")
    with torch.no_grad():
        plain = make_mlp(c, t, h1, h2, False, True, seed=5).to(DEV)
        clean, dirty = (vertex_mlp(v.to(DEV), x.to(DEV), D, plain, False) for v in (h, bad))
        assert bool(torch.isnan(dirty[r, 0])) and not bool(torch.isnan(clean).any())
        keep = torch.arange(n, device=DEV) != r
        assert torch.equal(clean[keep], dirty[keep])
        bn = make_mlp(c, t, h1, h2, True, True, seed=5).to(DEV)
        assert bool(torch.isnan(vertex_mlp(bad.to(DEV), x.to(DEV), D, bn, True)).all())
        assert not bool(torch.isnan(vertex_mlp(h.to(DEV), x.to(DEV), D, bn, True)).any())


# -------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors():
    """Valid device memory everywhere; each bad call returns its code before any launch (the outputs keep their
    fill) and names itself in gcn_last_error()."""
    from pygcn_amd import _native
    L = _native.lib()
    n, c, t, h1, h2, ldx = 100, 4, 2, 3, 2, 6
    f = functools.partial(torch.zeros, device=DEV)
    h, x = f(n, c), f(n, ldx)
    w1, b1, w2, b2, w3, b3 = f(h1, c + t), f(h1), f(h2, h1), f(h2), f(1, h2), f(1)
    stats, scores, ds, dh = f(256), torch.full((n,), 7.0, device=DEV), f(n), torch.full((n, c), 7.0, device=DEV)
    need = L.gcn_vmlp_workspace_bytes(n, c, t, h1, h2)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p = lambda v: v.data_ptr()                  # noqa: E731

    def forward(hp=p(h), nn=n, ld=ldx, dd=4, wsb=need):
        return L.gcn_vmlp_forward(hp, p(x), ld, dd, nn, c, t, p(w1), p(b1), h1, p(w2), p(b2), h2, p(w3), p(b3), 1,
                                  p(stats), p(scores), None, None, p(ws), wsb, None)

    def backward(hp=p(h), nn=n, ld=ldx, dd=4, wsb=need):
        return L.gcn_vmlp_backward(hp, p(x), ld, dd, nn, c, t, p(w1), p(b1), h1, p(w2), p(b2), h2, p(w3), p(b3), 1,
                                   p(stats), p(ds), p(dh), None, None, None, None, None, None, p(ws), wsb, None)
    for call, who in ((forward, b"gcn_vmlp_forward"), (backward, b"gcn_vmlp_backward")):
        for kw, code in ((dict(hp=None), -1), (dict(nn=-1), -1), (dict(ld=5), -1), (dict(dd=5), -1),
                         (dict(wsb=need - 1), -3)):
            assert call(**kw) == code, (who, kw)
            assert who in L.gcn_last_error(), (who, kw, L.gcn_last_error())
    torch.cuda.synchronize()
    assert bool((scores == 7.0).all()) and bool((dh == 7.0).all())
    assert forward() == 0 and backward() == 0
    torch.cuda.synchronize()
    assert not bool((scores == 7.0).any()) and not bool((dh == 7.0).any())
    assert np.isfinite(scores.cpu().numpy()).all()
