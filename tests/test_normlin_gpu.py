"""`functional.relu_batch_norm_linear` on the MI355X (gcn_bn_linear_forward / _backward_sums / _backward_apply,
pygcn_amd/csrc/gcn_normlin.hip) and the `fused_norm` flag of GCNBatchNorm / GCN_OVER_MLP.

s, dz and grad_W against the torch restatement tests/_normlin_ref.py on the CPU — float64 the arbiter, float32 the
reference arithmetic — through conftest.assert_parity at the project's 1e-5; the forward product EXACTLY on signed
permutations of powers of two; windows of a batched call, repeated runs and the gradient-free variant bitwise.  The
two shapes that depend on the launch geometry are derived from the documented formula of
gcn_bn_linear_workspace_bytes (include/gcn_spmm.h), so a retune moves them with it."""
import numpy as np
import pytest
import torch

import _normlin_ref as R
import test_batched_norm_gpu as B
import test_norm_gpu as T
import test_select_gpu as S
from conftest import assert_normwise, assert_parity, load_golden
from test_evaluator_cpu import g9_case
from test_norm_gpu import DEV, seeded

pytestmark = pytest.mark.gpu

W32 = 32
ROW = 1152 * 8          # bytes of one partial row: P[32][32] and four column sums, in double


def geometry(n, k=1):
    """(blocks B, rows per block R, tiles per wave T, block cap) of an n-row sweep, from the documented formula:
    batch * (B + 1) * 1152 * sizeof(double) bytes, T = ceil(n / (128 * cap)), R = 128 * T, B = ceil(n / R)."""
    from pygcn_amd import _native
    L = _native.lib()
    cap = L.gcn_bn_linear_workspace_bytes(1 << 40, W32, W32, k) // (k * ROW) - 1
    blocks = L.gcn_bn_linear_workspace_bytes(n, W32, W32, k) // (k * ROW) - 1
    tiles = -(-n // (128 * cap))
    assert blocks == -(-n // (128 * tiles)), "the workspace query left its documented formula"
    return blocks, 128 * tiles, tiles, cap


def n_three_blocks(k=3):
    """The smallest n whose sweep spans >= 3 blocks with a ragged last one."""
    for n in range(2, 1 << 22):
        blocks, rows, _, _ = geometry(n, k)
        if blocks >= 3 and (blocks - 1) * rows < n and n % rows != 0:
            return n
    raise AssertionError("no multi-block shape below 2^22 rows")


def n_two_tiles(k=2):
    """The smallest n at which a wave walks >= 2 tiles of 32 rows with a partial last tile: the last wave that has
    rows owns n mod (32 T) of them."""
    cap = geometry(2, k)[3]
    for n in range(128 * cap + 1, 128 * cap + 4096):
        tiles = geometry(n, k)[2]
        last = n % (32 * tiles)
        if tiles >= 2 and last > 32 and last % 32 != 0:
            return n
    raise AssertionError("no two-tile shape found")


SHAPES = [("2", 1), ("31", 1), ("33", 3), ("64", 20), ("1000", 3), ("three_blocks", 3), ("two_tiles", 2)]


def rows_of(name, k):
    return n_three_blocks(k) if name == "three_blocks" else n_two_tiles(k) if name == "two_tiles" else int(name)


def test_the_derived_shapes_have_their_properties():
    n = n_three_blocks(3)
    blocks, rows, tiles, _ = geometry(n, 3)
    assert blocks >= 3 and n % rows != 0 and (blocks - 1) * rows < n
    n = n_two_tiles(2)
    blocks, rows, tiles, cap = geometry(n, 2)
    last = n % (32 * tiles)
    assert tiles >= 2 and 32 < last < 32 * tiles and last % 32 != 0 and blocks <= cap
    assert n < 1 << 18                                              # (a few MB per tensor: the test stays quick)


_CACHE = {}


def inputs(n, k, seed=201):
    """z [n, k*32]: standard normal with per-column offsets in +-2 and scales 2^-3 .. 2^3, one all-negative column
    per window; W [32, 32] and a cotangent dS [n, k*32].  Made once per shape and never written to."""
    key = (n, k, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        z = seeded((n, k * W32), seed)
        scale = torch.from_numpy(2.0 ** rng.integers(-3, 4, k * W32).astype(np.float32))
        offset = torch.from_numpy(rng.uniform(-2, 2, k * W32).astype(np.float32))
        z = z * scale + offset
        for j in range(k):
            c = j * W32 + (5 * j + 3) % W32
            z[:, c] = -z[:, c].abs() - 0.25
        w = seeded((W32, W32), seed + 1) / 4
        ds = seeded((n, k * W32), seed + 2)
        _CACHE[key] = (z, w, ds)
    return _CACHE[key]


_REFS = {}


def reference(n, k):
    key = (n, k)
    if key not in _REFS:
        z, w, ds = inputs(n, k)
        _REFS[key] = (R.step(z, w, ds, torch.float32, batch=k), R.step(z, w, ds, torch.float64, batch=k))
    return _REFS[key]


def fused_step(z, w, ds, k, z_grad=True):
    """(s, dz, grad_W) of the HIP node on the device."""
    from pygcn_amd.functional import relu_batch_norm_linear
    zd, wd = z.to(DEV).requires_grad_(z_grad), w.to(DEV).requires_grad_()
    s = relu_batch_norm_linear(zd, wd, batch=k)
    assert s.grad_fn.name().startswith("ReluBatchNormLinearFunction"), s.grad_fn.name()
    s.backward(ds.to(DEV))
    torch.cuda.synchronize()
    return s.detach(), zd.grad, wd.grad


@pytest.mark.parametrize("n_name,k", SHAPES)
def test_forward_and_backward_against_float64(n_name, k):
    n = rows_of(n_name, k)
    z, w, ds = inputs(n, k)
    s, dz, gw = fused_step(z, w, ds, k)
    assert s.shape == (n, k * W32) and dz.shape == z.shape and gw.shape == (W32, W32)
    assert s.dtype == dz.dtype == gw.dtype == torch.float32
    r32, r64 = reference(n, k)
    for name, got, a32, a64 in zip(("s", "dz", "grad_W"), (s, dz, gw), r32, r64):
        assert_parity(got.cpu().numpy(), a32, a64, f"relu_batch_norm_linear {name} [{n}x{k}x32]")
    dead = [j * W32 + (5 * j + 3) % W32 for j in range(k)]
    assert not dz[:, dead].any()                                    # the mask is z > 0 exactly


@pytest.mark.parametrize("n_name,k", [("33", 3), ("three_blocks", 3)])
def test_signed_permutations_of_powers_of_two_are_exact(n_name, k):
    """s is, element for element (==), the permuted, scaled and negated columns of relu_batch_norm(z, batch=k):
    xhat is formed as bn_apply_kernel forms it and the product is a true fp32 fmaf chain."""
    from pygcn_amd.functional import relu_batch_norm, relu_batch_norm_linear
    n = rows_of(n_name, k)
    z = inputs(n, k)[0].to(DEV)
    rng = np.random.default_rng(7)
    perm = rng.permutation(W32)
    coef = (rng.choice([-1.0, 1.0], W32) * 2.0 ** rng.integers(-3, 4, W32)).astype(np.float32)
    w = torch.zeros(W32, W32)
    w[torch.arange(W32), torch.from_numpy(perm)] = torch.from_numpy(coef)
    with torch.no_grad():
        s = relu_batch_norm_linear(z, w.to(DEV), batch=k)
        y = relu_batch_norm(z, batch=k)
    torch.cuda.synchronize()
    want = torch.empty_like(y)
    to, factor = torch.from_numpy(perm).to(DEV), torch.from_numpy(coef).to(DEV)
    for j in range(k):
        want[:, j * W32 + to] = y[:, j * W32:(j + 1) * W32] * factor     # column i goes to perm[i], times coef[i]
    assert bool(torch.isfinite(s).all()) and bool((s == want).all())


@pytest.mark.parametrize("n_name,k", [("33", 3), ("three_blocks", 3), ("two_tiles", 2)])
def test_windows_runs_and_the_gradient_free_call_are_bitwise(n_name, k, monkeypatch):
    """A window of the batched call is the batch = 1 call on a contiguous copy (s, dz: torch.equal); two runs are
    torch.equal; without a gradient for z, grad_W is torch.equal and the apply sweep is not launched.

    grad_W of the batched call is the windows' double sums added in window order and rounded ONCE, which the
    per-window calls (each rounded to fp32) cannot reproduce bit for bit: it is held to assert_normwise 1e-5
    against the sum of the per-window results."""
    n = rows_of(n_name, k)
    z, w, ds = inputs(n, k)
    s, dz, gw = fused_step(z, w, ds, k)
    again = fused_step(z, w, ds, k)
    for a, b in zip((s, dz, gw), again):
        assert torch.equal(a, b)
    total = torch.zeros(W32, W32, dtype=torch.float64)
    for j in range(k):
        cols = slice(j * W32, (j + 1) * W32)
        s1, dz1, gw1 = fused_step(z[:, cols].contiguous(), w, ds[:, cols].contiguous(), 1)
        assert torch.equal(s1, s[:, cols]) and torch.equal(dz1, dz[:, cols]), j
        total += gw1.double().cpu()
    assert_normwise(gw.cpu().numpy(), total.numpy(), what=f"grad_W [{n}x{k}] vs the sum over the windows")
    spy = S.LaunchSpy(monkeypatch)
    s0, dz0, gw0 = fused_step(z, w, ds, k, z_grad=False)
    assert dz0 is None and torch.equal(s0, s) and torch.equal(gw0, gw)
    names = spy.names()
    assert names.count("gcn_bn_linear_forward") == 1 and names.count("gcn_bn_linear_backward_sums") == 1
    assert "gcn_bn_linear_backward_apply" not in names and "gcn_bn_apply_batched" not in names


@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_nan_and_inf_stay_in_their_window(poison):
    n, k, j, col, row = 33, 3, 1, 7, 5
    z, w, ds = inputs(n, k)
    clean = fused_step(z, w, ds, k)
    bad = z.clone()
    bad[row, j * W32 + col] = poison
    s, dz, _ = fused_step(bad, w, ds, k)
    for other in range(k):
        if other != j:
            cols = slice(other * W32, (other + 1) * W32)
            assert torch.equal(s[:, cols], clean[0][:, cols]) and torch.equal(dz[:, cols], clean[1][:, cols])
    assert not bool(torch.isfinite(s[:, j * W32:(j + 1) * W32]).any())      # xhat of the column is NaN in every row
    passes = ~(bad[:, j * W32 + col] <= 0)                                  # (a NaN z passes its gradient)
    assert bool(passes.any()) and not bool(torch.isfinite(dz[:, j * W32 + col].cpu()[passes]).any())


def test_no_host_synchronisation():
    from pygcn_amd.functional import relu_batch_norm_linear
    n, k = n_three_blocks(3), 3
    z, w, ds = inputs(n, k)
    zd, wd, dsd = z.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), ds.to(DEV)
    relu_batch_norm_linear(zd, wd, batch=k).backward(dsd)                  # (first use)
    kept = []
    assert S.count_host_syncs(lambda: kept.append(relu_batch_norm_linear(zd, wd, batch=k))) == 0
    assert S.count_host_syncs(lambda: kept[0].backward(dsd)) == 0


def test_nothing_of_the_activations_size_is_kept():
    """n = 100 000, k = 4: y = BN(relu(z)) would be 51 MB.  Above the state before the call the fused forward
    retains <= bytes(s) + 1 MiB and peaks at <= bytes(s) + W + 1 MiB; its backward peaks at <= bytes(dz) + W + 1 MiB
    above what is live when it starts (W = gcn_bn_linear_workspace_bytes).  The composition of the two separate
    nodes exceeds the first bound: the measurement can fail."""
    from pygcn_amd import _native
    from pygcn_amd.functional import relu_batch_norm, relu_batch_norm_linear
    from pygcn_amd.gemm import DenseMMFunction
    n, k, mib = 100_000, 4, 1 << 20
    zd = (seeded((n, k * W32), 211) * 2 + 0.5).to(DEV).requires_grad_()
    wd = (seeded((W32, W32), 212) / 4).to(DEV).requires_grad_()
    dsd = seeded((n, k * W32), 213).to(DEV)
    size = n * k * W32 * 4
    work = _native.lib().gcn_bn_linear_workspace_bytes(n, W32, W32, k)
    assert 0 < work < size

    def composition(z, w, batch):
        y = relu_batch_norm(z, batch=batch)
        return DenseMMFunction.apply(y.reshape(n * batch, W32), w).view(n, batch * W32)

    def measure(fn):
        zd.grad = wd.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        s = fn(zd, wd, batch=k)
        torch.cuda.synchronize()
        retained, peak_fwd = torch.cuda.memory_allocated() - base, torch.cuda.max_memory_allocated() - base
        live = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        s.backward(dsd)
        torch.cuda.synchronize()
        return retained, peak_fwd, torch.cuda.max_memory_allocated() - live

    measure(relu_batch_norm_linear)                                         # (first use)
    retained, peak_fwd, peak_bwd = measure(relu_batch_norm_linear)
    print(f"fused: retained {retained / mib:.1f} MiB, forward peak {peak_fwd / mib:.1f} MiB, backward peak "
          f"{peak_bwd / mib:.1f} MiB; s = {size / mib:.1f} MiB, W = {work / mib:.1f} MiB")
    assert retained <= size + mib
    assert peak_fwd <= size + work + mib
    assert peak_bwd <= size + work + mib
    measure(composition)
    retained_c, peak_c, peak_bwd_c = measure(composition)
    print(f"composition: retained {retained_c / mib:.1f} MiB, forward peak {peak_c / mib:.1f} MiB, backward peak "
          f"{peak_bwd_c / mib:.1f} MiB")
    assert retained_c > size + mib


# --------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_argument_errors():
    """All pointers are valid device memory of the stated size; every call returns before a launch."""
    from pygcn_amd import _native
    L = _native.lib()
    n, k = 37, 3
    z, ds, s, dz = (torch.zeros(n, k * W32, device=DEV) for _ in range(4))
    w, gw = torch.zeros(W32, W32, device=DEV), torch.zeros(W32, W32, device=DEV)
    mean, rstd = torch.zeros(k * W32, device=DEV), torch.ones(k * W32, device=DEV)
    coef = torch.zeros(4, k * W32, dtype=torch.float64, device=DEV)
    need = L.gcn_bn_linear_workspace_bytes(n, W32, W32, k)
    assert need == k * 2 * ROW
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def calls(n=n, fin=W32, fout=W32, k=k, zp=z.data_ptr(), wp=w.data_ptr(), dsp=ds.data_ptr(), cp=coef.data_ptr(),
              wsp=ws.data_ptr(), need=need, mp=mean.data_ptr()):
        return {
            "gcn_bn_linear_forward": lambda: L.gcn_bn_linear_forward(zp, wp, mp, rstd.data_ptr(), s.data_ptr(), n, fin,
                                                                     fout, k, 1, None),
            "gcn_bn_linear_backward_sums": lambda: L.gcn_bn_linear_backward_sums(
                dsp, zp, wp, mp, rstd.data_ptr(), n, fin, fout, k, 1, 1e-5, gw.data_ptr(), cp, wsp, need, None),
            "gcn_bn_linear_backward_apply": lambda: L.gcn_bn_linear_backward_apply(dsp, zp, wp, cp, dz.data_ptr(), n,
                                                                                   fin, fout, k, 1, None),
        }

    def expect(table, code, only=None):
        for name, call in table.items():
            if only is None or name in only:
                assert call() == code, name
                assert L.gcn_last_error().decode().startswith(name + ":"), (name, L.gcn_last_error())

    for bad in (dict(n=1), dict(n=0), dict(fin=24), dict(fout=24), dict(fin=64, fout=64), dict(k=0), dict(k=65536),
                dict(zp=None), dict(wp=None)):
        expect(calls(**bad), -1)                                           # GCN_E_BADARG
    expect(calls(mp=None), -1, ["gcn_bn_linear_forward", "gcn_bn_linear_backward_sums"])
    expect(calls(dsp=None), -1, ["gcn_bn_linear_backward_sums", "gcn_bn_linear_backward_apply"])
    expect(calls(cp=None), -1, ["gcn_bn_linear_backward_sums", "gcn_bn_linear_backward_apply"])
    expect(calls(zp=z.data_ptr() + 4), -2)                                 # GCN_E_ALIGN
    expect(calls(cp=coef.data_ptr() + 4), -2, ["gcn_bn_linear_backward_sums", "gcn_bn_linear_backward_apply"])
    expect(calls(wsp=ws.data_ptr() + 8), -2, ["gcn_bn_linear_backward_sums"])
    expect(calls(need=need - 1), -3, ["gcn_bn_linear_backward_sums"])      # GCN_E_WORKSPACE: one byte short
    expect(calls(wsp=None), -3, ["gcn_bn_linear_backward_sums"])
    torch.cuda.synchronize()
    for t in (s, dz, gw, coef):
        assert not t.any()                                                 # nothing was launched


# ------------------------------------------------------------------------------------------------ the models
@pytest.mark.parametrize("tag", ["a_", "b_", "c_"])
def test_the_evaluator_fixture_with_fused_norm(tag, monkeypatch):
    from pygcn_amd import CSRGraph, GCN_OVER_MLP
    g9 = load_golden("g9_evaluator.npz")
    state, x, _, d = g9_case(g9, tag)
    dims = [int(v) for v in g9["dims"]]
    model = GCN_OVER_MLP(dims[0], dims[1], dims[2], 0.0, dims[5], dims[2] + x.shape[2] - 1 - d, dims[3], dims[4],
                         dim_touched=d, fused_norm=True)
    model.load_state_dict(state, strict=True)
    model = model.to(DEV).train()
    graph = CSRGraph(torch.from_numpy(g9["rowptr"]).to(DEV), torch.from_numpy(g9["col"]).to(DEV),
                     torch.from_numpy(g9["val"]).to(DEV), (64, 64))
    xd = x.to(DEV).requires_grad_()
    spy = S.LaunchSpy(monkeypatch)
    out = model(xd, graph)
    out.sum().backward()
    torch.cuda.synchronize()
    names = spy.names()
    assert names.count("gcn_bn_linear_forward") == 2 and names.count("gcn_bn_linear_backward_sums") == 2
    assert names.count("gcn_bn_linear_backward_apply") == 2 and "gcn_bn_apply_batched" not in names
    assert_normwise(out.detach().cpu().numpy(), g9[tag + "out"], what=f"fused_norm {tag}out")
    assert_normwise(xd.grad[:, :, -1].cpu().numpy(), g9[tag + "dflag"], what=f"fused_norm {tag}dflag")
    for name, p in model.named_parameters():
        assert_normwise(p.grad.cpu().numpy(), g9[tag + "grad_" + name], what=f"fused_norm {tag}grad {name}")


def fused_relu_masks(model, wide, adj_dev, k):
    """The ReLU derivatives the device used on the fused route, per sample and layer: the calls
    GCNBatchNorm._fused_tail makes."""
    from pygcn_amd.functional import relu_batch_norm_linear
    n = wide.shape[0]
    z1 = model.gc1.forward_wide(wide, adj_dev, k)
    z2 = model.gc2.aggregate(relu_batch_norm_linear(z1, model.gc2.weight, batch=k), adj_dev, k)
    z3 = model.gc3.aggregate(relu_batch_norm_linear(z2, model.gc3.weight, batch=k), adj_dev, k)
    return [[(z.view(n, k, -1)[:, j] > 0).cpu() for z in (z1, z2, z3)] for j in range(k)]


@pytest.mark.parametrize("batched", [True, False])
def test_model_with_fused_norm_against_the_default_route_and_the_cpu(batched, monkeypatch):
    from pygcn_amd import GCNBatchNorm
    n, edges = B.CASES["random600x12"][:2]
    adj_cpu, adj_dev = B._graph(n, edges)
    k = 3 if batched else 1
    x = seeded((k, n, W32), 221)
    cot = seeded((k, n, W32), 222)
    torch.manual_seed(42)
    plain = GCNBatchNorm(W32, W32, W32, 0.5, 3)
    state = {name: v.detach().clone() for name, v in plain.state_dict().items()}
    fused = GCNBatchNorm(W32, W32, W32, 0.5, 3, fused_norm=True)
    fused.load_state_dict(state)
    plain, fused = plain.to(DEV).train(), fused.to(DEV).train()
    xin, cin = (x.to(DEV), cot.to(DEV)) if batched else (x[0].to(DEV), cot[0].to(DEV))
    spy = S.LaunchSpy(monkeypatch)
    out = fused(xin, adj_dev)
    out.backward(cin)
    assert spy.names().count("gcn_bn_linear_forward") == 2 and "gcn_bn_apply_batched" not in spy.names()
    want = plain(xin, adj_dev)
    want.backward(cin)
    wide = x.permute(1, 0, 2).reshape(n, k * W32).to(DEV)
    masks = fused_relu_masks(fused, wide, adj_dev, k)
    torch.cuda.synchronize()
    what = f"fused_norm {'[3, n, 32]' if batched else '[n, 32]'}"
    assert out.shape == want.shape
    assert_normwise(out.detach().cpu().numpy(), want.detach().cpu().numpy(), what=f"{what}: output vs the default")
    names = sorted(state)
    assert names == ["gc1.bias", "gc1.weight", "gc2.bias", "gc2.weight", "gc3.bias", "gc3.weight"]
    got = {name: p.grad.cpu().numpy() for name, p in fused.named_parameters()}
    for name, p in plain.named_parameters():
        assert_normwise(got[name], p.grad.cpu().numpy(), what=f"{what}: {name}.grad vs the default")
    for j in range(k):
        T.check_relu_masks(masks[j], state, x[j], adj_cpu)

    def cpu_step(dtype):
        params = {name: v.detach().clone().to(dtype).requires_grad_() for name, v in state.items()}
        outs = torch.stack([T.fork_forward(params, x[j].to(dtype), adj_cpu.to(dtype), masks[j])[0] for j in range(k)])
        outs.backward(cot.to(dtype))
        return outs.detach().numpy(), {name: p.grad.numpy() for name, p in params.items()}
    o32, g32 = cpu_step(torch.float32)
    o64, g64 = cpu_step(torch.float64)
    got_out = out.detach().cpu().numpy().reshape(k, n, W32)
    assert_parity(got_out, o32, o64, f"{what}: output")
    for name in names:
        assert_parity(got[name], g32[name], g64[name], f"{what}: {name}.grad")
