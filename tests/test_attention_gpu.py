"""The vertex-attention sweeps on the MI355X (gcn_attn_scores / gcn_attn_normalize / gcn_attn_backward,
pygcn_amd/csrc/gcn_norm.hip), `vertex_attention` / `vertex_mean` and the fork's SoftGenerator (reference
pygcn/models.py:289-329, 412-433).

A window's results are held BITWISE against the batch = 1 call on a contiguous copy of the window; the
autograd node against tests/_attention_ref.py on the CPU (float64 the arbiter, float32 the reference
arithmetic, conftest.assert_parity at the project's 1e-5; bf16 at 2^-8 on the bf16-rounded inputs).  The
parity inputs keep |score| <= 16: a stored fp32 score carries 6e-8 * |s| of relative error into attn."""
import numpy as np
import pytest
import torch

import _attention_ref as R
from conftest import assert_normwise, assert_parity, load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def n_big(c, dtype):
    """The smallest row count whose sweep spans >= 3 blocks with a ragged last one, from the documented
    formula of gcn_attn_workspace_bytes (include/gcn_spmm.h): B * max(C, 2) * sizeof(double) bytes for B
    blocks, block b sweeping rows [b * R, min((b + 1) * R, n)), R = ceil(n / B)."""
    from pygcn_amd import _native
    from pygcn_amd.norm import _DTYPES
    for n in range(1, 1 << 22):
        blocks = _native.lib().gcn_attn_workspace_bytes(n, c, 1, _DTYPES[dtype]) // (max(c, 2) * 8)
        rows = -(-n // blocks)
        if blocks >= 3 and (blocks - 1) * rows < n and n % rows != 0:
            return n
    raise AssertionError("no multi-block shape below 2^22 rows")


def rows_of(name, c, dtype=torch.float32):
    return n_big(c, dtype) if name == "n_big" else int(name)


def seeded(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def sweeps(store, key, ds_or_g, k, need_dh=True):
    """Every result of the three entry points over storage [n, k*C] on the device.  `ds_or_g` [k, n]: the
    cotangent g (ds is then formed from attn as the autograd node forms it) or, as a (ds,) tuple, ds itself."""
    from pygcn_amd.attention import attn_backward, attn_normalize, attn_scores
    n, c = store.shape[0], store.shape[1] // k
    scores, stats = attn_scores(store, key, n, k, c)
    attn = attn_normalize(scores.clone(), stats)
    if isinstance(ds_or_g, tuple):
        ds = ds_or_g[0].contiguous()
    else:
        ds = (attn * (ds_or_g - (ds_or_g * attn).sum(1, keepdim=True))).contiguous()
    dh, dkey = attn_backward(store, ds, key, n, k, c, need_dh=need_dh)
    torch.cuda.synchronize()
    return dict(scores=scores, stats=stats, attn=attn, ds=ds, dh=dh, dkey=dkey)


WIDTHS = [(4, torch.float32), (32, torch.float32), (256, torch.float32), (512, torch.float32), (128, torch.bfloat16)]


def check_windows(n, c, dtype, k):
    store = torch.relu(seeded((n, k * c), 201)).to(dtype).to(DEV)
    key = (seeded((k * c,), 202) * (2.0 / c ** 0.5)).to(DEV)
    g = seeded((k, n), 203).to(DEV)
    got = sweeps(store, key, g, k)
    s64 = torch.einsum("nkc,kc->kn", store.double().view(n, k, c), key.double().view(k, c))
    assert float(s64.abs().max()) <= 16.0
    assert_normwise(got["scores"].cpu().numpy(), s64.cpu().numpy(), what=f"scores [{n}x({k}x{c}) {dtype}]")
    for j in range(k):
        w = slice(j * c, (j + 1) * c)
        ref = sweeps(store[:, w].contiguous(), key[w].contiguous(), (got["ds"][j:j + 1],), 1)
        for name in ("scores", "stats", "attn"):
            assert torch.equal(got[name][j:j + 1], ref[name]), f"{name}, window {j} of {k} [{n}x{c} {dtype}]"
        assert torch.equal(got["dh"][:, w], ref["dh"]), f"dh, window {j} of {k} [{n}x{c} {dtype}]"
        assert torch.equal(got["dkey"][w], ref["dkey"]), f"dkey, window {j} of {k} [{n}x{c} {dtype}]"
    return got


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("c,dtype", WIDTHS)
@pytest.mark.parametrize("n_name", ["1", "37", "n_big"])
def test_windows_equal_the_2d_path_bitwise(n_name, c, dtype, k):
    """CG = C / V threads per row: 1 (C = 4), 8, 64 (one full wave), 128 (crosses waves), 16 (bf16)."""
    check_windows(rows_of(n_name, c, dtype), c, dtype, k)


@pytest.mark.parametrize("k", [1, 3])
def test_windows_with_more_than_64_rows_per_block(k):
    """n = 2048 * 64 + 37 at C = 16: every one of the 2048 blocks sweeps more than 64 rows (8 MB per window)."""
    from pygcn_amd import _native
    n, c = 2048 * 64 + 37, 16
    assert _native.lib().gcn_attn_workspace_bytes(n, c, 1, 0) == 2048 * c * 8
    got = check_windows(n, c, torch.float32, k)
    sums = got["attn"].double().sum(1)
    assert bool(((sums - 1.0).abs() <= 1e-6).all()), sums


# ------------------------------------------------------------------------- autograd node against float64
def hip_step(h, key, g, wide=False):
    """(attn, dh, dkey) through `vertex_attention` on the device; `wide`: h [k, N, C] travels as the permuted
    view of contiguous [N, k*C] storage."""
    from pygcn_amd.functional import vertex_attention
    if wide:
        k, n, c = h.shape
        hd = h.permute(1, 0, 2).reshape(n, k * c).contiguous().to(DEV).view(n, k, c).permute(1, 0, 2)
    else:
        hd = h.to(DEV)
    hd.requires_grad_()
    kd = key.to(DEV).requires_grad_()
    attn = vertex_attention(hd, kd)
    assert attn.grad_fn.name().startswith("VertexAttentionFunction"), attn.grad_fn.name()
    attn.backward(g.to(DEV))
    torch.cuda.synchronize()
    return attn.detach().cpu(), hd.grad.cpu(), kd.grad.cpu()


GATED = [(37, 32, 1.0), (6000, 32, 1.0), (6000, 256, 0.25), (200000, 256, 0.25), (6000, 1024, 0.125)]


@pytest.mark.parametrize("n,c,scale", GATED)
def test_node_fp32_against_float64(n, c, scale):
    h, key, g = R.recipe(n, c, scale)
    got = hip_step(h, key, g)
    ref32, ref64 = R.attention_step(h, key, g, torch.float32), R.attention_step(h, key, g, torch.float64)
    for name, a, r32, r64 in zip(("attn", "dh", "dkey"), got, ref32, ref64):
        assert a.dtype == torch.float32 and a.shape == r32.shape, name
        assert_parity(a.numpy(), r32.numpy(), r64.numpy(), f"{name} [{n}x{c}, key scale {scale}]")


def test_node_fp32_batched_against_float64():
    """[k, N, C] with one key per sample, over the permuted view; key as [1, C] in the 2-D form."""
    k, n, c = 3, 6000, 32
    h, key, g = R.recipe(n, c, 1.0, k=k)
    got = hip_step(h, key, g, wide=True)
    ref32, ref64 = R.attention_step(h, key, g, torch.float32), R.attention_step(h, key, g, torch.float64)
    for name, a, r32, r64 in zip(("attn", "dh", "dkey"), got, ref32, ref64):
        assert a.shape == r32.shape, name
        for j in range(k):        # each sample against its own scale
            assert_parity(a[j].numpy(), r32[j].numpy(), r64[j].numpy(), f"{name}, sample {j} of [{k}x{n}x{c}]")
    one = hip_step(h[0], key[:1], g[0])
    assert one[0].shape == (n,) and one[2].shape == (1, c)
    assert torch.equal(one[0], got[0][0])        # (the gradients' ds passes through torch's row sum: not held bitwise)
    assert_normwise(one[1].numpy(), got[1][0].numpy(), what="dh, 2-D call vs sample 0")
    assert_normwise(one[2][0].numpy(), got[2][0].numpy(), what="dkey, 2-D call vs sample 0")


def test_node_bf16():
    """bf16 storage: fp32 arithmetic on the bf16-rounded inputs, one rounding of each stored result."""
    n, c = 6000, 128
    h, key, g = (t.bfloat16() for t in R.recipe(n, c, 0.25))
    got = hip_step(h, key, g)
    assert all(a.dtype == torch.bfloat16 for a in got)
    ref64 = R.attention_step(h.float(), key.float(), g.float(), torch.float64)
    for name, a, r64 in zip(("attn", "dh", "dkey"), got, ref64):
        assert_normwise(a.double().numpy(), r64.numpy(), rel=2.0 ** -8, what=f"bf16 {name} [{n}x{c}]")


# ------------------------------------------------------------------------------------------ properties
def test_two_runs_are_bitwise_equal():
    k, c = 3, 32
    n = n_big(c, torch.float32)
    store = torch.relu(seeded((n, k * c), 211)).to(DEV)
    key, g = (0.3 * seeded((k * c,), 212)).to(DEV), seeded((k, n), 213).to(DEV)
    a, b = sweeps(store, key, g, k), sweeps(store, key, g, k)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_basic_values():
    c = 32
    one = sweeps(seeded((1, c), 221).to(DEV), seeded((c,), 222).to(DEV), seeded((1, 1), 223).to(DEV), 1)
    assert float(one["attn"][0, 0]) == 1.0 and bool((one["dh"] == 0).all()) and bool((one["dkey"] == 0).all())
    assert float(one["stats"][0, 1]) == 1.0 and float(one["stats"][0, 0]) == float(one["scores"][0, 0])
    k, n = 3, n_big(c, torch.float32)
    got = sweeps(torch.relu(seeded((n, k * c), 224)).to(DEV), (0.5 * seeded((k * c,), 225)).to(DEV),
                 seeded((k, n), 226).to(DEV), k)
    sums = got["attn"].double().sum(1)
    assert bool(((sums - 1.0).abs() <= 1e-6).all()), sums
    assert bool((got["attn"] >= 0).all())


def test_a_nan_stays_in_its_window():
    """One NaN written into valid memory of window 1 of 3: that window's attn is all NaN, as torch's softmax,
    and windows 0 and 2 keep their bits."""
    k, c = 3, 32
    n = n_big(c, torch.float32)
    store = torch.relu(seeded((n, k * c), 231)).to(DEV)
    key, g = (0.3 * seeded((k * c,), 232)).to(DEV), seeded((k, n), 233).to(DEV)
    clean = sweeps(store, key, g, k)
    store[n // 2, c + 9] = float("nan")
    bad = sweeps(store, key, g, k)
    assert bool(torch.isnan(bad["attn"][1]).all()) and bool(torch.isnan(bad["dh"][:, c:2 * c]).all())
    assert bool(torch.isnan(torch.softmax(bad["scores"][1].cpu(), 0)).all())
    for j in (0, 2):
        w = slice(j * c, (j + 1) * c)
        for name in ("scores", "stats", "attn", "ds"):
            assert torch.equal(bad[name][j], clean[name][j]), (name, j)
        assert torch.equal(bad["dh"][:, w], clean["dh"][:, w]) and torch.equal(bad["dkey"][w], clean["dkey"][w])


def test_attn_may_alias_scores_and_dh_may_be_null():
    from pygcn_amd.attention import attn_normalize
    k, c = 3, 32
    n = n_big(c, torch.float32)
    store = torch.relu(seeded((n, k * c), 241)).to(DEV)
    key, g = (0.3 * seeded((k * c,), 242)).to(DEV), seeded((k, n), 243).to(DEV)
    got = sweeps(store, key, g, k)
    apart = attn_normalize(got["scores"], got["stats"], out=torch.empty_like(got["scores"]))
    assert apart.data_ptr() != got["scores"].data_ptr() and torch.equal(apart, got["attn"])
    in_place = got["scores"].clone()
    assert attn_normalize(in_place, got["stats"]).data_ptr() == in_place.data_ptr()
    assert torch.equal(in_place, got["attn"])
    without = sweeps(store, key, (got["ds"],), k, need_dh=False)
    assert without["dh"] is None and torch.equal(without["dkey"], got["dkey"])
    # through the node: h without requires_grad costs no dh
    from pygcn_amd.functional import vertex_attention
    kd = key[:c].clone().requires_grad_()
    h0 = store[:, :c].contiguous()
    vertex_attention(h0, kd).backward(g[0])
    assert h0.grad is None
    assert_normwise(kd.grad.cpu().numpy(), got["dkey"][:c].cpu().numpy(), what="dkey of a node whose h needs no gradient")


def test_c_abi_argument_errors():
    """All pointers are valid device memory of the stated size; every call returns before a launch."""
    from pygcn_amd import _native
    L = _native.lib()
    n, c, k = 37, 16, 3
    h = torch.randn(n + 1, k * c, device=DEV)
    key = torch.zeros(k * c, device=DEV)
    rows = torch.zeros(k, n, device=DEV)
    stats = torch.zeros(k, 2, dtype=torch.float64, device=DEV)
    dkey = torch.zeros(k * c, dtype=torch.float64, device=DEV)
    need = L.gcn_attn_workspace_bytes(n, c, k, 0)
    assert need == k * c * 8
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    hp, kp, rp, sp, dp, wp = (t.data_ptr() for t in (h, key, rows, stats, dkey, ws))

    def calls(n=n, c=c, k=k, hp=hp, need=need, wp=wp):
        return {
            "gcn_attn_scores": lambda: L.gcn_attn_scores(0, hp, kp, n, c, k, rp, sp, wp, need, None),
            "gcn_attn_backward": lambda: L.gcn_attn_backward(0, hp, rp, kp, hp, dp, n, c, k, wp, need, None),
        }

    def expect(table, code):
        for name, call in table.items():
            assert call() == code, name
            assert L.gcn_last_error().decode().startswith(name + ":"), (name, L.gcn_last_error())

    expect(calls(c=24, k=2), -1)                 # GCN_E_BADARG: width outside the shape rule
    expect(calls(c=7), -1)
    expect(calls(n=0), -1)
    expect(calls(k=0), -1)
    expect(calls(k=65536), -1)
    expect(calls(hp=None), -1)                   # GCN_E_BADARG: NULL tensor
    expect(calls(hp=hp + 4), -2)                 # GCN_E_ALIGN: h (and dh) off the 16-byte grid
    expect(calls(need=need - 1), -3)             # GCN_E_WORKSPACE: one byte short
    expect(calls(wp=None), -3)
    norm = {"gcn_attn_normalize": lambda: L.gcn_attn_normalize(rp, None, rp, n, k, None)}
    expect(norm, -1)
    expect({"gcn_attn_normalize": lambda: L.gcn_attn_normalize(rp, sp, rp, 0, k, None)}, -1)
    expect({"gcn_attn_normalize": lambda: L.gcn_attn_normalize(rp, sp, rp, n, 0, None)}, -1)
    expect({"gcn_attn_normalize": lambda: L.gcn_attn_normalize(rp, sp + 4, rp, n, k, None)}, -2)
    assert L.gcn_attn_backward(0, hp, rp, kp, None, dp, n, c, k, wp, need, None) == 0      # dh may be NULL
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- model
class LaunchSpy:
    """Records (name, args) of every _native.launch while it forwards them."""

    def __init__(self, monkeypatch):
        from pygcn_amd import _native
        self.calls, real = [], _native.launch

        def launch(name, device, *args, **kw):
            self.calls.append((name, args))
            return real(name, device, *args, **kw)
        monkeypatch.setattr(_native, "launch", launch)

    def names(self):
        return [name for name, _ in self.calls]


def test_soft_generator_reinforce_step(monkeypatch):
    """The fixture's model on the device: forward, -reward * sum log attn[picked], backward — attn and every
    parameter gradient against the reference's own run, float64 from the restatement as the arbiter."""
    from pygcn_amd import CSRGraph, SoftGenerator
    from pygcn_amd.sharded import ShardedGraph
    g7 = load_golden("g7_soft_generator.npz")
    state, x, adj, d, picked, reward = R.fixture_case(g7)
    dims = [int(v) for v in g7["dims"]]
    model = SoftGenerator(dims[0], dims[1], dims[2], 0.0, dims[5], dims[3], dims[4], dim_touched=d)
    model.load_state_dict(state, strict=True)
    model = model.to(DEV).train()
    n = x.shape[0]
    graph = CSRGraph(torch.from_numpy(g7["rowptr"]).to(DEV), torch.from_numpy(g7["col"]).to(DEV),
                     torch.from_numpy(g7["val"]).to(DEV), (n, n))
    spy = LaunchSpy(monkeypatch)
    attn = model(x.to(DEV), graph)
    assert attn.shape == (n,) and attn.dtype == torch.float32
    loss = -reward * torch.log(attn[picked.to(DEV)]).sum()
    loss.backward()
    torch.cuda.synchronize()
    for name in ("gcn_masked_colsum", "gcn_attn_scores", "gcn_attn_normalize", "gcn_attn_backward",
                 "gcn_masked_broadcast"):
        assert name in spy.names(), (name, spy.names())
    attn64, grads64 = R.reinforce_step(state, x, adj, d, picked, reward, torch.float64)
    assert_parity(attn.detach().cpu().numpy(), g7["attn"], attn64, "SoftGenerator attn")
    assert_normwise(float(loss), float(g7["loss"]), what="SoftGenerator loss")
    params = dict(model.named_parameters())
    assert sorted(params) == sorted(state)
    for name in state:
        assert_parity(params[name].grad.cpu().numpy(), g7["grad_" + name], grads64[name], f"SoftGenerator grad {name}")
    with pytest.raises(RuntimeError, match="ShardedGraph adjacency is not supported"):
        model(x.to(DEV), object.__new__(ShardedGraph))


def test_attention_reads_the_batched_models_output_in_place(monkeypatch):
    """GCNBatchNorm's batched result, the [k, N, C] permuted view of [N, k*C] storage, goes into the sweeps as
    it lies (the pointer the kernel gets is the view's), and gives what the per-sample loop gives."""
    from pygcn_amd import CSRGraph, GCNBatchNorm
    from pygcn_amd.functional import vertex_attention, vertex_mean
    from pygcn_amd.utils import rmat_graph
    k, n, c = 3, 37, 32
    rowptr, col, val = rmat_graph(n, 300, seed=5, device="cpu")
    graph = CSRGraph(rowptr.to(DEV), col.to(DEV), val.to(DEV), (n, n))
    torch.manual_seed(42)
    model = GCNBatchNorm(12, 16, c, dropout=0.0).to(DEV).train()
    out = model(seeded((k, n, 12), 251).to(DEV), graph)
    assert out.shape == (k, n, c) and not out.is_contiguous()
    key = (0.5 * seeded((k, c), 252)).to(DEV).requires_grad_()
    spy = LaunchSpy(monkeypatch)
    attn = vertex_attention(out, key)
    mean = vertex_mean(out)
    assert attn.shape == (k, n) and mean.shape == (k, c)
    seen = dict(spy.calls)
    assert seen["gcn_attn_scores"][1] == out.data_ptr() and seen["gcn_attn_scores"][3:6] == (n, c, k)
    assert seen["gcn_masked_colsum"][1] == out.data_ptr()
    g = seeded((k, n), 253).to(DEV)
    grads = torch.autograd.grad(attn, (out, key), g)
    assert grads[0].shape == out.shape and grads[1].shape == key.shape
    with torch.no_grad():
        assert_normwise(mean.cpu().numpy(), out.mean(1).cpu().numpy(), what="vertex_mean vs torch's mean")
    for j in range(k):
        hj = out[j].detach().contiguous().requires_grad_()
        kj = key[j].detach().clone().requires_grad_()
        aj = vertex_attention(hj, kj)
        aj.backward(g[j])
        for name, a, b in (("attn", attn[j], aj), ("dh", grads[0][j], hj.grad), ("dkey", grads[1][j], kj.grad)):
            assert_normwise(a.detach().cpu().numpy(), b.detach().cpu().numpy(), what=f"{name}, sample {j} vs the loop")
    h64, key64 = out.detach().cpu().double(), key.detach().cpu().double()
    assert_normwise(attn.detach().cpu().numpy(), R.head(h64, key64).numpy(), what="batched attn vs float64")
