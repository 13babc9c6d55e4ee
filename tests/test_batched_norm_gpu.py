"""k samples side by side on the MI355X: the column-window form of the ReLU + BatchNorm sweeps
(gcn_bn_*_batched, pygcn_amd/csrc/gcn_norm.hip), `relu_batch_norm(batch=k)`, the batched GCNBatchNorm
(the loop of the fork's evaluator, reference pygcn/models.py:343-349, in one pass) and the masked mean
pool (its PoolLayer, :267-286).

A window's results are held BITWISE against the existing 2-D entry points on a contiguous copy of the
window; everything else against torch on the CPU as in tests/test_norm_gpu.py (float64 the arbiter,
float32 the reference arithmetic, conftest.assert_parity / assert_normwise at the project's 1e-5)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_norm_gpu as T
from conftest import assert_normwise, assert_parity
from test_norm_gpu import DEV, EPS, n_big, rows_of, seeded

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------- windows against the 2-D entry points
def sweeps_2d(z, g, gamma, beta, relu):
    """All eight results of the EXISTING 2-D entry points on contiguous [n, F] device tensors."""
    from pygcn_amd import _native
    from pygcn_amd.norm import _DTYPES
    n, nf = z.shape
    dt = _DTYPES[z.dtype]
    assert z.is_contiguous() and g.is_contiguous()
    need = _native.lib().gcn_bn_workspace_bytes(n, nf, dt)
    mean, var, rstd, sum_g, sum_gxhat = (torch.empty(nf, device=DEV) for _ in range(5))
    coef = torch.empty(4, nf, dtype=torch.float64, device=DEV)
    y, dz = torch.empty_like(z), torch.empty_like(z)
    _native.launch("gcn_bn_stats", DEV, dt, z.data_ptr(), n, nf, int(relu), EPS, mean.data_ptr(), var.data_ptr(),
                   rstd.data_ptr(), workspace=need)
    _native.launch("gcn_bn_apply", DEV, dt, z.data_ptr(), y.data_ptr(), n, nf, int(relu), mean.data_ptr(),
                   rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr())
    _native.launch("gcn_bn_backward_sums", DEV, dt, g.data_ptr(), z.data_ptr(), n, nf, int(relu), EPS,
                   mean.data_ptr(), sum_g.data_ptr(), sum_gxhat.data_ptr(), coef.data_ptr(), workspace=need)
    _native.launch("gcn_bn_backward_apply", DEV, dt, g.data_ptr(), z.data_ptr(), dz.data_ptr(), n, nf, int(relu),
                   gamma.data_ptr(), coef.data_ptr())
    return dict(mean=mean, var=var, rstd=rstd, y=y, sum_g=sum_g, sum_gxhat=sum_gxhat, coef=coef, dz=dz)


def sweeps_batched(z, g, gamma, beta, relu, k):
    from pygcn_amd.norm import bn_apply, bn_backward_apply, bn_backward_sums, bn_stats
    mean, var, rstd = bn_stats(z, relu, EPS, batch=k)
    y = bn_apply(z, mean, rstd, gamma, beta, relu, batch=k)
    sum_g, sum_gxhat, coef = bn_backward_sums(g, z, mean, relu, EPS, batch=k)
    dz = bn_backward_apply(g, z, coef, gamma, relu, batch=k)
    return dict(mean=mean, var=var, rstd=rstd, y=y, sum_g=sum_g, sum_gxhat=sum_gxhat, coef=coef, dz=dz)


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("nf,dtype", [(16, torch.float32), (256, torch.float32), (128, torch.bfloat16)])
@pytest.mark.parametrize("n_name", ["2", "37", "n_big"])
def test_windows_equal_the_2d_path_bitwise(n_name, nf, dtype, k):
    """Every output of every window is, bit for bit, what the 2-D entry point returns on
    z[:, j*F:(j+1)*F].contiguous() — so a window's result cannot depend on `batch` either.  k = 3 at
    F = 16 is 48 columns, k = 5 at F = 128 is 640: widths the 2-D shape rule rejects."""
    from pygcn_amd import _native
    from pygcn_amd.norm import _DTYPES
    n = rows_of(n_name, nf, dtype)
    z, g = seeded((n, k * nf), 71).to(dtype).to(DEV), seeded((n, k * nf), 72).to(dtype).to(DEV)
    gamma, beta = (1.0 + 0.5 * seeded((k * nf,), 73)).to(DEV), seeded((k * nf,), 74).to(DEV)
    got = sweeps_batched(z, g, gamma, beta, True, k)
    for j in range(k):
        w = slice(j * nf, (j + 1) * nf)
        ref = sweeps_2d(z[:, w].contiguous(), g[:, w].contiguous(), gamma[w].contiguous(), beta[w].contiguous(), True)
        for name, r in ref.items():
            a = got[name][:, w] if got[name].dim() == 2 else got[name][w]
            assert torch.equal(a, r), f"{name}, window {j} of {k} [{n}x{nf} {dtype}]"
    if n_name == "n_big":                       # dz may alias g: the same bits, over >= 3 blocks per window
        _native.launch("gcn_bn_backward_apply_batched", DEV, _DTYPES[dtype], g.data_ptr(), z.data_ptr(), g.data_ptr(),
                       n, nf, k, 1, gamma.data_ptr(), got["coef"].data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(g, got["dz"])


# ------------------------------------------------------------------------- autograd node against float64
def torch_loop(z, w, b, g, relu, k, dtype):
    """(y, dz, dweight, dbias): one BatchNorm applied to each sample's columns in turn, sharing weight and
    bias — torch on the CPU in `dtype`."""
    z = z.detach().clone().to(dtype).requires_grad_()
    w = w.detach().clone().to(dtype).requires_grad_() if w is not None else None
    b = b.detach().clone().to(dtype).requires_grad_() if b is not None else None
    x = torch.relu(z) if relu else z
    nf = z.shape[1] // k
    y = torch.cat([F.batch_norm(x[:, j * nf:(j + 1) * nf], None, None, w, b, True, 0.0, EPS) for j in range(k)], 1)
    y.backward(g.to(dtype))
    return y.detach(), z.grad, w.grad if w is not None else None, b.grad if b is not None else None


def hip_batched(z, w, b, g, relu, k):
    from pygcn_amd.functional import relu_batch_norm
    z = z.to(DEV).requires_grad_()
    w = w.to(DEV).requires_grad_() if w is not None else None
    b = b.to(DEV).requires_grad_() if b is not None else None
    y = relu_batch_norm(z, w, b, eps=EPS, relu=relu, batch=k)
    y.backward(g.to(DEV))
    torch.cuda.synchronize()
    return (y.detach().cpu(), z.grad.cpu(), w.grad.cpu() if w is not None else None,
            b.grad.cpu() if b is not None else None)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("n_name", ["2", "37", "n_big"])
def test_batched_node_fp32(n_name, affine, relu):
    nf, k = 16, 3
    n = rows_of(n_name, nf)
    z, g = seeded((n, k * nf), 81), seeded((n, k * nf), 82)
    w = 1.0 + 0.5 * seeded((nf,), 83) if affine else None
    b = seeded((nf,), 84) if affine else None
    got = hip_batched(z, w, b, g, relu, k)
    ref32 = torch_loop(z, w, b, g, relu, k, torch.float32)
    ref64 = torch_loop(z, w, b, g, relu, k, torch.float64)
    for name, a, r32, r64 in zip(("y", "dz", "dweight", "dbias"), got, ref32, ref64):
        if a is None:
            assert r32 is None
            continue
        assert a.dtype == torch.float32 and a.shape == r32.shape
        assert_parity(a.numpy(), r32.numpy(), r64.numpy(), f"{name} [{n}x({k}x{nf}), affine={affine}, relu={relu}]")


@pytest.mark.parametrize("n_name", ["37", "n_big"])
def test_batched_node_bf16(n_name):
    """bf16 storage, the gate of test_norm_gpu.test_forward_backward_bf16: fp32 arithmetic on the
    bf16-rounded inputs, 2^-8 relative for the one rounding of each stored element; the parameter
    gradients are fp32 sums and keep 1e-5."""
    nf, k = 128, 3
    n = rows_of(n_name, nf, torch.bfloat16)
    z, g = seeded((n, k * nf), 85).bfloat16(), seeded((n, k * nf), 86).bfloat16()
    w, b = 1.0 + 0.5 * seeded((nf,), 87), seeded((nf,), 88)
    got = hip_batched(z, w, b, g, True, k)
    assert got[0].dtype == got[1].dtype == torch.bfloat16
    ref32 = torch_loop(z.float(), w, b, g.float(), True, k, torch.float32)
    ref64 = torch_loop(z.float(), w, b, g.float(), True, k, torch.float64)
    for name, a, r64 in zip(("y", "dz"), got[:2], ref64[:2]):
        err = (a.double() - r64).abs()
        assert bool((err <= 2.0 ** -8 * r64.abs() + 1e-5 * float(r64.abs().max())).all()), name
    for name, a, r32, r64 in zip(("dweight", "dbias"), got[2:], ref32[2:], ref64[2:]):
        assert a.dtype == torch.float32
        assert_parity(a.numpy(), r32.numpy(), r64.numpy(), f"bf16 {name} [{n}x({k}x{nf})]")


def test_hip_route_runs_without_torch_batch_norm(monkeypatch):
    from pygcn_amd.norm import supported

    def refuse(*a, **kw):
        raise AssertionError("torch's batch_norm was called on a supported input")
    n, nf, k = 37, 16, 3
    z, g = seeded((n, k * nf), 91), seeded((n, k * nf), 92)
    w, b = 1.0 + 0.5 * seeded((nf,), 93), seeded((nf,), 94)
    zd = z.to(DEV)
    assert supported(zd, k) and not supported(zd) and not supported(z, k) and not supported(zd, 2)
    assert not supported(zd.t(), 1) and not supported(zd.double(), k)
    with monkeypatch.context() as m:
        m.setattr(torch.nn.functional, "batch_norm", refuse)
        got = hip_batched(z, w, b, g, True, k)
    ref = torch_loop(z, w, b, g, True, k, torch.float32)
    for name, a, r in zip(("y", "dz", "dweight", "dbias"), got, ref):
        assert_normwise(a.numpy(), r.numpy(), what=f"HIP route {name}")
    # a window width of 24 (2 x 24 = 48 columns) is outside the rule: the literal torch composition
    w24, b24 = 1.0 + 0.5 * seeded((24,), 95), seeded((24,), 96)
    assert not supported(zd, 2)
    got24 = hip_batched(z, w24, b24, g, True, 2)
    ref24 = torch_loop(z, w24, b24, g, True, 2, torch.float32)
    for name, a, r in zip(("y", "dz", "dweight", "dbias"), got24, ref24):
        assert_normwise(a.numpy(), r.numpy(), what=f"fallback {name}")


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_nan_and_inf_stay_in_their_window_and_column(poison, relu):
    """One NaN / +inf written into valid memory (nothing is provoked) at (n_big / 2, window 1, column 9):
    exactly that column of that window is non-finite in y and dz; column 9 of windows 0 and 2 is finite."""
    nf, k = 16, 3
    n = n_big(nf, torch.float32)
    z, g = seeded((n, k * nf), 101), seeded((n, k * nf), 102)
    w, b = 1.0 + 0.5 * seeded((nf,), 103), seeded((nf,), 104)
    col = 1 * nf + 9
    z[n // 2, col] = poison
    got = hip_batched(z, w, b, g, relu, k)
    ref = torch_loop(z, w, b, g, relu, k, torch.float32)
    for name, a, r in zip(("y", "dz", "dweight", "dbias"), got, ref):
        assert torch.equal(torch.isnan(a), torch.isnan(r)), f"{name}: isnan pattern differs from torch's"
        assert torch.equal(torch.isfinite(a), torch.isfinite(r)), name
    others = [c for c in range(k * nf) if c != col]
    for a in got[:2]:
        assert bool(torch.isfinite(a[:, others]).all()) and not bool(torch.isfinite(a[:, col]).all())
        assert bool(torch.isfinite(a[:, [9, 2 * nf + 9]]).all())
    keep = torch.isfinite(ref[0])
    assert_normwise(got[0][keep].numpy(), ref[0][keep].numpy(), what="y outside the poisoned column")


# ------------------------------------------------------------------------------ C-ABI argument errors
def test_c_abi_argument_errors():
    """All pointers are valid device memory of the stated size; every call returns before a launch."""
    from pygcn_amd import _native
    L = _native.lib()
    n, nf, k = 37, 16, 3
    z = torch.randn(n, k * nf, device=DEV)
    col = [torch.zeros(k * nf, device=DEV) for _ in range(5)]
    zp, (m, v, r, s0, s1) = z.data_ptr(), [c.data_ptr() for c in col]
    coef = torch.zeros(4, k * nf, dtype=torch.float64, device=DEV)
    cf = coef.data_ptr()
    mask = torch.ones(k, n, device=DEV)
    mk = mask.data_ptr()
    need = L.gcn_bn_batched_workspace_bytes(n, nf, k, 0)
    assert need == k * L.gcn_bn_workspace_bytes(n, nf, 0) and need >= L.gcn_pool_workspace_bytes(n, nf, k, 0) > 0
    pool_need = L.gcn_pool_workspace_bytes(n, nf, k, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    wp = ws.data_ptr()

    def bn_calls(n, nf, k, zp=zp, need=need, wp=wp):
        return {
            "gcn_bn_stats_batched": lambda: L.gcn_bn_stats_batched(0, zp, n, nf, k, 1, EPS, m, v, r, wp, need, None),
            "gcn_bn_apply_batched": lambda: L.gcn_bn_apply_batched(0, zp, zp, n, nf, k, 1, m, r, None, None, None),
            "gcn_bn_backward_sums_batched": lambda: L.gcn_bn_backward_sums_batched(0, zp, zp, n, nf, k, 1, EPS, m, s0, s1,
                                                                                   cf, wp, need, None),
            "gcn_bn_backward_apply_batched": lambda: L.gcn_bn_backward_apply_batched(0, zp, zp, zp, n, nf, k, 1, None, cf,
                                                                                     None),
        }

    def pool_calls(n, nf, k, zp=zp, need=pool_need, wp=wp):
        return {
            "gcn_masked_colsum": lambda: L.gcn_masked_colsum(0, zp, mk, n, nf, k, cf, wp, need, None),
            "gcn_masked_broadcast": lambda: L.gcn_masked_broadcast(0, mk, m, zp, n, nf, k, None),
        }

    def expect(table, code):
        for name, call in table.items():
            assert call() == code, name
            assert L.gcn_last_error().decode().startswith(name + ":"), (name, L.gcn_last_error())

    for calls in (bn_calls, pool_calls):
        expect(calls(n, nf, 0), -1)                # GCN_E_BADARG: batch = 0
        expect(calls(n, nf, 65536), -1)
        expect(calls(n, 24, 2), -1)                # GCN_E_BADARG: window width outside the shape rule
        expect(calls(n, 7, k), -1)
        expect(calls(n, nf, k, zp=None), -1)       # GCN_E_BADARG: NULL tensor
    expect(bn_calls(1, nf, k), -1)                 # GCN_E_BADARG: n_rows < 2 (BatchNorm only)
    expect(pool_calls(0, nf, k), -1)
    short = {**bn_calls(n, nf, k, need=need - 1), **pool_calls(n, nf, k, need=pool_need - 1)}
    reducing = ("gcn_bn_stats_batched", "gcn_bn_backward_sums_batched", "gcn_masked_colsum")
    expect({name: short[name] for name in reducing}, -3)         # GCN_E_WORKSPACE: one byte short
    none = {**bn_calls(n, nf, k, wp=None), **pool_calls(n, nf, k, wp=None)}
    expect({name: none[name] for name in reducing}, -3)          # GCN_E_WORKSPACE: NULL
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- pool
def pool_ref(h, mask, count, cot, dtype):
    """reference pygcn/models.py:272,279 restated: (h * mask[:, :, None]).sum(1) / count, and its gradient."""
    h = h.detach().clone().to(dtype).requires_grad_()
    out = (h * mask.to(dtype)[:, :, None]).sum(1) / count.to(dtype).reshape(-1, 1)
    out.backward(cot.to(dtype))
    return out.detach(), h.grad


def wide_view(h):
    """[k, N, C] values as the permuted view of contiguous [N, k*C] device storage (GCNBatchNorm's result)."""
    k, n, c = h.shape
    store = h.permute(1, 0, 2).reshape(n, k * c).contiguous().to(DEV)
    return store.view(n, k, c).permute(1, 0, 2)


def hip_pool(h, mask, count, cot):
    from pygcn_amd.functional import masked_mean_pool
    hd = wide_view(h).requires_grad_()
    out = masked_mean_pool(hd, mask.to(DEV), count.to(DEV) if count is not None else None)
    assert out.grad_fn.name().startswith("MaskedMeanPoolFunction"), out.grad_fn.name()
    out.backward(cot.to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu(), hd.grad.cpu()


def bernoulli_mask(k, n, seed, p=0.3):
    return torch.from_numpy((np.random.default_rng(seed).random((k, n)) < p).astype(np.float32))


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("c", [16, 256])
@pytest.mark.parametrize("n_name", ["1", "37", "n_big"])
def test_pool_forward_backward_fp32(n_name, c, k):
    n = rows_of(n_name, c)
    h, cot = seeded((k, n, c), 111), seeded((k, c), 112)
    mask = bernoulli_mask(k, n, 113)
    mask[:, 0] = 1.0                                  # (no empty sample here: see the all-zero test)
    count = (mask != 0).sum(1)
    got = hip_pool(h, mask, None, cot)
    ref32, ref64 = pool_ref(h, mask, count, cot, torch.float32), pool_ref(h, mask, count, cot, torch.float64)
    for name, a, r32, r64 in zip(("pooled", "dh"), got, ref32, ref64):
        assert a.dtype == torch.float32 and a.shape == r32.shape
        assert_parity(a.numpy(), r32.numpy(), r64.numpy(), f"{name} [{k}x{n}x{c}]")


@pytest.mark.parametrize("n_name", ["1", "n_big"])
def test_pool_forward_backward_bf16(n_name):
    """bf16 storage: the bf16 instantiations of the two pool sweeps.  The sums are exact products added in double,
    so pooled and dh are the float64 results on the bf16-rounded inputs with ONE rounding to bf16 each (dh: after
    the fp32 quotient g / count) — within one bf16 ulp, 2^-8 relative, of float64; a zero stays zero."""
    c, k = 128, 3
    n = rows_of(n_name, c, torch.bfloat16)
    h, cot = seeded((k, n, c), 131).bfloat16(), seeded((k, c), 132).bfloat16()
    mask = bernoulli_mask(k, n, 133)
    mask[:, 0] = 1.0
    count = (mask != 0).sum(1)
    got = hip_pool(h, mask, None, cot)
    ref64 = pool_ref(h.float(), mask, count, cot.float(), torch.float64)
    for name, a, r64 in zip(("pooled", "dh"), got, ref64):
        assert a.dtype == torch.bfloat16 and a.shape == r64.shape
        assert bool(((a.double() - r64).abs() <= 2.0 ** -8 * r64.abs()).all()), f"bf16 {name} [{k}x{n}x{c}]"


def test_pool_with_the_forks_count_and_an_empty_sample():
    """count = sample 0's vertex count for every sample (reference pygcn/models.py:279); a sample whose
    mask is all zero under its OWN count is 0 / 0: torch's NaN pattern."""
    k, c = 3, 16
    n = n_big(c, torch.float32)
    h, cot = seeded((k, n, c), 121), seeded((k, c), 122)
    mask = bernoulli_mask(k, n, 123)
    fork_count = (mask[0] != 0).sum()
    got = hip_pool(h, mask, fork_count, cot)
    ref32 = pool_ref(h, mask, fork_count, cot, torch.float32)
    ref64 = pool_ref(h, mask, fork_count, cot, torch.float64)
    for name, a, r32, r64 in zip(("pooled", "dh"), got, ref32, ref64):
        assert_parity(a.numpy(), r32.numpy(), r64.numpy(), f"fork's count: {name}")
    again = hip_pool(h, mask, fork_count, cot)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])         # bitwise reproducible
    mask[1] = 0.0
    own = (mask != 0).sum(1)
    got = hip_pool(h, mask, None, cot)
    ref = pool_ref(h, mask, own, cot, torch.float32)
    for name, a, r in zip(("pooled", "dh"), got, ref):
        assert torch.equal(torch.isnan(a), torch.isnan(r)) and torch.equal(torch.isinf(a), torch.isinf(r)), name
        keep = torch.isfinite(r)
        assert_normwise(a[keep].numpy(), r[keep].numpy(), what=f"empty sample: finite part of {name}")
    assert bool(torch.isnan(got[0][1]).all()) and bool(torch.isfinite(got[0][[0, 2]]).all())
    # the mask multiplies: a NaN under a zero mask stays NaN, in its sample and column only
    mask = bernoulli_mask(k, n, 124)
    row = int((mask[2] == 0).nonzero()[0])
    h[2, row, 5] = float("nan")
    pooled = hip_pool(h, mask, None, cot)[0]
    bad = torch.zeros(k, c, dtype=torch.bool)
    bad[2, 5] = True
    assert torch.equal(torch.isnan(pooled), bad)


def test_pool_layouts():
    """The permuted view gives, sample by sample, the bits of the contiguous [N, C] call (a window's sum
    does not depend on k); a [1, N, C] tensor is one sample; other layouts and C = 7 take the torch route."""
    from pygcn_amd.functional import masked_mean_pool
    k, c = 3, 16
    n = n_big(c, torch.float32)
    h, mask = seeded((k, n, c), 131), bernoulli_mask(k, n, 132)
    hd, md = wide_view(h), mask.to(DEV)
    whole = masked_mean_pool(hd.requires_grad_(), md)
    assert whole.grad_fn.name().startswith("MaskedMeanPoolFunction")
    for j in range(k):
        one = hd[j].detach().contiguous().requires_grad_()
        flat = masked_mean_pool(one, md[j])
        assert flat.grad_fn.name().startswith("MaskedMeanPoolFunction") and flat.shape == (1, c)
        assert torch.equal(flat[0], whole[j].detach())
        assert torch.equal(masked_mean_pool(one.detach()[None], md[j:j + 1]), flat.detach())
    plain = h.to(DEV).requires_grad_()            # contiguous [k, N, C]: not the wide storage
    out = masked_mean_pool(plain, md)
    assert not out.grad_fn.name().startswith("MaskedMeanPoolFunction")
    assert_normwise(out.detach().cpu().numpy(), whole.detach().cpu().numpy(), what="torch route, contiguous [k, N, C]")
    h7, cot7 = seeded((k, 37, 7), 133), seeded((k, 7), 134)
    m7 = bernoulli_mask(k, 37, 135)
    m7[:, 0] = 1.0
    h7d = wide_view(h7).requires_grad_()
    out7 = masked_mean_pool(h7d, m7.to(DEV))
    assert not out7.grad_fn.name().startswith("MaskedMeanPoolFunction")
    out7.backward(cot7.to(DEV))
    ref7 = pool_ref(h7, m7, (m7 != 0).sum(1), cot7, torch.float32)
    assert_normwise(out7.detach().cpu().numpy(), ref7[0].numpy(), what="C = 7 pooled")
    assert_normwise(h7d.grad.cpu().numpy(), ref7[1].numpy(), what="C = 7 dh")


# --------------------------------------------------------------------------------------------- model
def _graph(n, edges):
    from pygcn_amd import CSRGraph
    from pygcn_amd.utils import rmat_graph
    rowptr, col, val = rmat_graph(n, edges, seed=5, device="cpu")
    adj = torch.sparse_csr_tensor(rowptr.long(), col.long(), val, (n, n))
    return adj, CSRGraph(rowptr.to(DEV), col.to(DEV), val.to(DEV), (n, n))


CASES = {"random3000x256": (3000, 30000, (256, 256, 256), 3), "random600x12": (600, 4000, (12, 16, 7), 5)}


def batched_relu_masks(model, x, adj_dev):
    """The ReLU derivatives the device used on the BATCHED path, per sample and layer: the calls
    GCNBatchNorm._forward_batched makes (as test_norm_gpu.device_relu_masks does for the 2-D path)."""
    from pygcn_amd.functional import relu_batch_norm
    k, n, _ = x.shape
    z1 = model.gc1.forward_wide(x.permute(1, 0, 2).reshape(n, -1), adj_dev, k)
    z2 = model.gc2.forward_wide(relu_batch_norm(z1, batch=k), adj_dev, k)
    z3 = model.gc3.forward_wide(relu_batch_norm(z2, batch=k), adj_dev, k)
    return [[(z.view(n, k, -1)[:, j] > 0).cpu() for z in (z1, z2, z3)] for j in range(k)]


def cpu_evaluator_step(state, x, adj, mask, cot, dtype, masks):
    """reference pygcn/models.py:341-355 restated on the CPU up to the MLP: the GCN once per sample
    (:343-349), the masked mean pool with the count of sample 0 (PoolLayer, :272,279), a cotangent on the
    [k, C] result."""
    params = {name: v.detach().clone().to(dtype).requires_grad_() for name, v in state.items()}
    outs = [T.fork_forward(params, x[j].to(dtype), adj.to(dtype), masks[j])[0] for j in range(x.shape[0])]
    h = torch.stack(outs)
    pooled = (h * mask.to(dtype)[:, :, None]).sum(1) / len(torch.nonzero(mask[0], as_tuple=True)[0])
    pooled.backward(cot.to(dtype))
    return pooled.detach().numpy(), {name: p.grad.numpy() for name, p in params.items()}


@pytest.mark.parametrize("case", list(CASES))
def test_batched_model_and_evaluator_step(case):
    from pygcn_amd import GCNBatchNorm
    from pygcn_amd.functional import masked_mean_pool
    n, edges, dims, k = CASES[case]
    adj_cpu, adj_dev = _graph(n, edges)
    x = seeded((k, n, dims[0]), 61)
    torch.manual_seed(42)
    model = GCNBatchNorm(*dims, dropout=0.5, NN=3)
    state = {name: v.detach().clone() for name, v in model.state_dict().items()}
    model = model.to(DEV).train()
    xd = x.to(DEV)
    mask = bernoulli_mask(k, n, 62)
    cot = seeded((k, dims[2]), 63)

    # forward: the batched pass against the device's own per-sample loop (the products sum in other orders)
    out = model(xd, adj_dev)
    assert out.shape == (k, n, dims[2])
    with torch.no_grad():
        loop = torch.stack([model(xd[j], adj_dev) for j in range(k)])
    assert_normwise(out.detach().cpu().numpy(), loop.cpu().numpy(), what=f"{case}: batched forward vs the loop")

    # the evaluator's step
    pooled = masked_mean_pool(out, mask.to(DEV), count=(mask[0] != 0).sum().to(DEV))
    assert pooled.grad_fn.name().startswith("MaskedMeanPoolFunction") == (dims[2] % 4 == 0)
    pooled.backward(cot.to(DEV))
    masks = batched_relu_masks(model, xd, adj_dev)
    torch.cuda.synchronize()
    for j in range(k):
        T.check_relu_masks(masks[j], state, x[j], adj_cpu)
    p32, grads32 = cpu_evaluator_step(state, x, adj_cpu, mask, cot, torch.float32, masks)
    p64, grads64 = cpu_evaluator_step(state, x, adj_cpu, mask, cot, torch.float64, masks)
    assert_parity(pooled.detach().cpu().numpy(), p32, p64, f"{case}: pooled output")
    assert sorted(grads32) == ["gc1.bias", "gc1.weight", "gc2.bias", "gc2.weight", "gc3.bias", "gc3.weight"]
    for name in grads32:
        mod, par = name.split(".")
        got = getattr(getattr(model, mod), par).grad.cpu().numpy()
        assert_parity(got, grads32[name], grads64[name], f"{case}: {name}.grad")

    # a 2-D input through the same object: today's path, the bits of a model that never saw a batch
    torch.manual_seed(42)
    fresh = GCNBatchNorm(*dims, dropout=0.5, NN=3).to(DEV).train()
    with torch.no_grad():
        assert torch.equal(model(xd[0], adj_dev), fresh(xd[0], adj_dev))


def test_dense_adjacency_matches_the_sparse_one():
    from pygcn_amd import GCNBatchNorm
    n, edges, dims, k = CASES["random600x12"]
    adj_cpu, adj_dev = _graph(n, edges)
    xd = seeded((k, n, dims[0]), 61).to(DEV)
    torch.manual_seed(42)
    model = GCNBatchNorm(*dims, dropout=0.5).to(DEV).train()
    with torch.no_grad():
        sparse = model(xd, adj_dev)
        dense = model(xd, adj_cpu.to_dense().to(DEV))
    assert dense.shape == (k, n, dims[2])
    assert_normwise(dense.cpu().numpy(), sparse.cpu().numpy(), what="dense [N, N] adjacency vs CSR")
