"""ReLU + BatchNorm sweeps (pygcn_amd/csrc/gcn_norm.hip, pygcn_amd/norm.py) and the fork's live 3-layer
model (pygcn_amd.models.GCNBatchNorm; reference pygcn/models.py:17-71) on the MI355X.

The reference of every comparison is torch on the CPU, computed here: `F.batch_norm(F.relu(z), ...)` in
float64 is the arbiter, the same in float32 the reference arithmetic; both go through
conftest.assert_parity / assert_normwise at the project's 1e-5.  bf16 storage follows the project's
convention (tests/test_gemm_gpu.py): float32 arithmetic on the bf16-rounded inputs, 2^-8 relative for
the final rounding of each stored element."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import inputs as gin
from conftest import GOLDEN, _record, assert_normwise, assert_parity

pytestmark = pytest.mark.gpu

EPS = 1e-5
DEV = torch.device("cuda:0")


def n_big(nf, dtype):
    """The smallest row count whose sweep spans >= 3 blocks with a ragged last one, from the
    documented formula of gcn_bn_workspace_bytes (include/gcn_spmm.h): B * 4 * F * sizeof(double)
    bytes for B blocks, block b sweeping rows [b * R, min((b + 1) * R, n)), R = ceil(n / B) — so a
    retune of the slab size moves this shape with it."""
    from pygcn_amd import _native
    from pygcn_amd.norm import _DTYPES
    for n in range(2, 1 << 22):
        blocks = _native.lib().gcn_bn_workspace_bytes(n, nf, _DTYPES[dtype]) // (4 * nf * 8)
        rows = -(-n // blocks)
        if blocks >= 3 and (blocks - 1) * rows < n and n % rows != 0:
            return n
    raise AssertionError("no multi-block shape below 2^22 rows")


def rows_of(name, nf, dtype=torch.float32):
    return n_big(nf, dtype) if name == "n_big" else int(name)


def seeded(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def torch_step(z, w, b, g, relu, dtype):
    """(y, dz, dgamma, dbeta, mean, var, rstd) of torch's composition on the CPU in `dtype`."""
    z = z.detach().clone().to(dtype).requires_grad_()
    w = w.detach().clone().to(dtype).requires_grad_() if w is not None else None
    b = b.detach().clone().to(dtype).requires_grad_() if b is not None else None
    x = torch.relu(z) if relu else z
    y = F.batch_norm(x, None, None, w, b, True, 0.0, EPS)
    y.backward(g.to(dtype))
    xd = x.detach()
    var = xd.var(0, unbiased=False)
    return (y.detach(), z.grad, w.grad if w is not None else None, b.grad if b is not None else None,
            xd.mean(0), var, 1.0 / torch.sqrt(var + EPS))


def hip_step(z, w, b, g, relu):
    from pygcn_amd.functional import relu_batch_norm
    z = z.to(DEV).requires_grad_()
    w = w.to(DEV).requires_grad_() if w is not None else None
    b = b.to(DEV).requires_grad_() if b is not None else None
    y = relu_batch_norm(z, w, b, eps=EPS, relu=relu)
    y.backward(g.to(DEV))
    torch.cuda.synchronize()
    return (y.detach().cpu(), z.grad.cpu(), w.grad.cpu() if w is not None else None,
            b.grad.cpu() if b is not None else None)


# ---------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("nf", [16, 256])
@pytest.mark.parametrize("n_name", ["2", "37", "n_big"])
def test_statistics_match_float64(n_name, nf, relu):
    from pygcn_amd.norm import bn_stats
    n = rows_of(n_name, nf)
    z = seeded((n, nf), 11)
    got = [t.cpu().numpy() for t in bn_stats(z.to(DEV), relu, EPS)]
    ref32 = torch_step(z, None, None, z, relu, torch.float32)[4:]
    ref64 = torch_step(z, None, None, z, relu, torch.float64)[4:]
    for name, a, r32, r64 in zip(("mean", "var", "rstd"), got, ref32, ref64):
        assert_parity(a, r32.numpy(), r64.numpy(), f"{name} [{n}x{nf}, relu={relu}]")


@pytest.mark.parametrize("nf", [16, 256])
@pytest.mark.parametrize("n_name", ["37", "n_big"])
def test_variance_of_a_column_far_from_zero(n_name, nf):
    """z = 1000 + N(0,1): sum x^2 / n - mean^2 cancels six digits — in fp32 sums nothing of the variance
    is left (9e-2 relative on the CPU emulation of the kernel's order); the double sums keep it.
    Only the statistics are judged on this input: y inherits the rounding of mean to fp32, in torch's
    own float32 result as well."""
    from pygcn_amd.norm import bn_stats
    n = rows_of(n_name, nf)
    z = 1000.0 + seeded((n, nf), 12)
    mean, var, rstd = (t.cpu().numpy().astype(np.float64) for t in bn_stats(z.to(DEV), False, EPS))
    z64 = z.double()
    var64 = z64.var(0, unbiased=False).numpy()
    rstd64 = 1.0 / np.sqrt(var64 + EPS)
    assert (np.abs(var - var64) <= 1e-5 * var64).all(), (np.abs(var - var64) / var64).max()
    assert (np.abs(rstd - rstd64) <= 1e-5 * rstd64).all()
    assert_normwise(mean, z64.mean(0).numpy(), what="mean of the offset column")


# ---------------------------------------------------------------------------- forward and backward
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("nf", [16, 256])
@pytest.mark.parametrize("n_name", ["2", "37", "n_big"])
def test_forward_backward_fp32(n_name, nf, affine, relu):
    """y, dz, dgamma, dbeta through the autograd node against torch on the CPU, float64 the arbiter.

    n = 2 with relu=False is the hard case for dz: over two rows xhat = +-1, so
    dz = gamma * rstd * (g - mean g - xhat * mean(g xhat)) cancels to eps / (var + eps) of its terms, and
    any fp32 rounding of mean, rstd or the sums is multiplied by the inverse of that — torch's own
    float32 evaluation is 3e-5 of max|dz| from float64 at 2 x 16.  The backward sweeps work in double
    (gcn_norm.hip, file header) and meet the float64 gate there as well."""
    n = rows_of(n_name, nf)
    z, g = seeded((n, nf), 21), seeded((n, nf), 22)
    w = 1.0 + 0.5 * seeded((nf,), 23) if affine else None
    b = seeded((nf,), 24) if affine else None
    got = hip_step(z, w, b, g, relu)
    ref32 = torch_step(z, w, b, g, relu, torch.float32)
    ref64 = torch_step(z, w, b, g, relu, torch.float64)
    for name, a, r32, r64 in zip(("y", "dz", "dgamma", "dbeta"), got, ref32, ref64):
        if a is None:
            assert r32 is None
            continue
        assert a.dtype == torch.float32
        assert_parity(a.numpy(), r32.numpy(), r64.numpy(), f"{name} [{n}x{nf}, affine={affine}, relu={relu}]")


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("n_name", ["37", "n_big"])
def test_forward_backward_bf16(n_name, affine, relu):
    """bf16 storage (config C5), F = 128: fp32 arithmetic on the bf16-rounded inputs, one rounding in
    the store of y and dz; the parameter gradients are fp32 sums and keep the 1e-5 gate."""
    nf = 128
    n = rows_of(n_name, nf, torch.bfloat16)
    z, g = seeded((n, nf), 31).bfloat16(), seeded((n, nf), 32).bfloat16()
    w = 1.0 + 0.5 * seeded((nf,), 33) if affine else None
    b = seeded((nf,), 34) if affine else None
    got = hip_step(z, w, b, g, relu)
    assert got[0].dtype == got[1].dtype == torch.bfloat16
    ref32 = torch_step(z.float(), w, b, g.float(), relu, torch.float32)
    ref64 = torch_step(z.float(), w, b, g.float(), relu, torch.float64)
    for name, a, r64 in zip(("y", "dz"), got[:2], ref64[:2]):
        err = (a.double() - r64).abs()
        assert bool((err <= 2.0 ** -8 * r64.abs() + 1e-5 * float(r64.abs().max())).all()), name
    if affine:
        for name, a, r32, r64 in zip(("dgamma", "dbeta"), got[2:], ref32[2:4], ref64[2:4]):
            assert a.dtype == torch.float32
            assert_parity(a.numpy(), r32.numpy(), r64.numpy(), f"bf16 {name} [{n}x{nf}, relu={relu}]")


@pytest.mark.parametrize("which", ["weight", "bias"])
def test_weight_alone_and_bias_alone(which):
    """gamma and beta are separate NULL branches in the kernels and in the autograd node."""
    n, nf = 37, 16
    z, g = seeded((n, nf), 25), seeded((n, nf), 26)
    w = 1.0 + 0.5 * seeded((nf,), 27) if which == "weight" else None
    b = seeded((nf,), 28) if which == "bias" else None
    got = hip_step(z, w, b, g, True)
    ref32 = torch_step(z, w, b, g, True, torch.float32)
    ref64 = torch_step(z, w, b, g, True, torch.float64)
    assert (got[2] is None) == (w is None) and (got[3] is None) == (b is None)
    for name, a, r32, r64 in zip(("y", "dz", "dgamma", "dbeta"), got, ref32, ref64):
        if a is not None:
            assert_parity(a.numpy(), r32.numpy(), r64.numpy(), f"{which} alone: {name}")


@pytest.mark.parametrize("dtype,nf", [(torch.float32, 16), (torch.bfloat16, 128)])
def test_backward_apply_in_place(dtype, nf):
    """dz may alias g (include/gcn_spmm.h): the same bits as the out-of-place call, over >= 3 blocks."""
    from pygcn_amd import _native
    from pygcn_amd.norm import _DTYPES, bn_backward_apply, bn_backward_sums, bn_stats
    n = n_big(nf, dtype)
    z, g = seeded((n, nf), 35).to(dtype).to(DEV), seeded((n, nf), 36).to(dtype).to(DEV)
    gamma = (1.0 + 0.5 * seeded((nf,), 37)).to(DEV)
    mean, _, _ = bn_stats(z, True, EPS)
    _, _, coef = bn_backward_sums(g, z, mean, True, EPS)
    apart = bn_backward_apply(g, z, coef, gamma, True)
    _native.launch("gcn_bn_backward_apply", z.device, _DTYPES[dtype], g.data_ptr(), z.data_ptr(), g.data_ptr(),
                   n, nf, 1, gamma.data_ptr(), coef.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(g, apart)


# --------------------------------------------------------------------------------------- edge cases
def _edge_input(n, nf):
    z, g = seeded((n, nf), 41), seeded((n, nf), 42)
    w, b = 1.0 + 0.5 * seeded((nf,), 43), seeded((nf,), 44)
    return z, g, w, b


def test_dead_relu_unit():
    """A column with z <= 0 everywhere: var = 0, rstd = eps^-1/2, y = beta, dz = 0."""
    from pygcn_amd.norm import bn_stats
    n, nf = n_big(16, torch.float32), 16
    z, g, w, b = _edge_input(n, nf)
    z[:, 5] = -z[:, 5].abs()
    z[0, 5] = 0.0
    got = hip_step(z, w, b, g, True)
    ref32 = torch_step(z, w, b, g, True, torch.float32)
    ref64 = torch_step(z, w, b, g, True, torch.float64)
    _, var, rstd = (t.cpu() for t in bn_stats(z.to(DEV), True, EPS))
    assert float(var[5]) == 0.0 and abs(float(rstd[5]) - EPS ** -0.5) <= 1e-5 * EPS ** -0.5
    assert torch.equal(got[0][:, 5], b[5].expand(n)) and not got[1][:, 5].any()
    for name, a, r32, r64 in zip(("y", "dz", "dgamma", "dbeta"), got, ref32, ref64):
        assert_parity(a.numpy(), r32.numpy(), r64.numpy(), f"dead unit: {name}")
    assert float(got[2][5]) == float(ref32[2][5]) == 0.0


def test_constant_column_without_relu():
    n, nf = n_big(16, torch.float32), 16
    z, g, w, b = _edge_input(n, nf)
    z[:, 3] = 3.7
    got = hip_step(z, w, b, g, False)
    ref32 = torch_step(z, w, b, g, False, torch.float32)
    ref64 = torch_step(z, w, b, g, False, torch.float64)
    for name, a, r32, r64 in zip(("y", "dz", "dgamma", "dbeta"), got, ref32, ref64):
        assert_parity(a.numpy(), r32.numpy(), r64.numpy(), f"constant column: {name}")
    assert torch.equal(got[0][:, 3], b[3].expand(n))


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_nan_and_inf_stay_in_their_column(poison, relu):
    """One NaN / +inf (valid memory, nothing is provoked): exactly that column of y and dz is
    non-finite, with torch's isnan pattern (under ReLU torch's mask zeroes dz where z <= 0)."""
    n, nf = n_big(16, torch.float32), 16
    z, g, w, b = _edge_input(n, nf)
    z[n // 2, 9] = poison
    got = hip_step(z, w, b, g, relu)
    ref = torch_step(z, w, b, g, relu, torch.float32)
    others = [c for c in range(nf) if c != 9]
    for name, a, r in zip(("y", "dz", "dgamma", "dbeta"), got, ref):
        assert torch.equal(torch.isnan(a), torch.isnan(r)), f"{name}: isnan pattern differs from torch's"
        assert torch.equal(torch.isfinite(a), torch.isfinite(r)), name
        keep = torch.isfinite(r)
        assert_normwise(a[keep].numpy(), r[keep].numpy(), what=f"{name} outside the poisoned column")
    for a in got[:2]:
        assert bool(torch.isfinite(a[:, others]).all()) and not bool(torch.isfinite(a[:, 9]).all())


def test_a_single_row_raises_like_torch():
    from pygcn_amd.functional import relu_batch_norm
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        relu_batch_norm(torch.zeros(1, 16, device=DEV))


# ------------------------------------------------------------------------------ determinism, routes
def test_two_runs_are_bitwise_equal():
    n, nf = 4099, 256
    z, g, w, b = _edge_input(n, nf)
    first, second = hip_step(z, w, b, g, True), hip_step(z, w, b, g, True)
    for a, c in zip(first, second):
        assert torch.equal(a, c)


def test_hip_route_runs_without_torch_batch_norm(monkeypatch):
    from pygcn_amd.functional import relu_batch_norm
    from pygcn_amd.norm import supported

    def refuse(*a, **k):
        raise AssertionError("torch's batch_norm was called on a supported input")
    z, g, w, b = _edge_input(37, 16)
    assert supported(z.to(DEV)) and not supported(z) and not supported(z.to(DEV).t())
    assert not supported(z.to(DEV).double()) and not supported(z.to(DEV)[:, :7].contiguous())
    with monkeypatch.context() as m:
        m.setattr(torch.nn.functional, "batch_norm", refuse)
        got = hip_step(z, w, b, g, True)
    ref = torch_step(z, w, b, g, True, torch.float32)
    assert_normwise(got[0].numpy(), ref[0].numpy(), what="y on the HIP route")
    # F = 7 is outside the shape rule: the literal torch composition, on the device
    z7, g7 = z[:, :7].contiguous(), g[:, :7].contiguous()
    got7 = hip_step(z7, w[:7].clone(), b[:7].clone(), g7, True)
    ref7 = torch_step(z7, w[:7].clone(), b[:7].clone(), g7, True, torch.float32)
    for name, a, r in zip(("y", "dz", "dgamma", "dbeta"), got7, ref7):
        assert_normwise(a.numpy(), r.numpy(), what=f"fallback {name}")


# ------------------------------------------------------------------------------ C-ABI argument errors
def test_c_abi_argument_errors():
    from pygcn_amd import _native
    L = _native.lib()
    n, nf = 37, 16
    z = torch.randn(n, nf, device=DEV)
    col = [torch.zeros(nf, device=DEV) for _ in range(5)]
    zp, (m, v, r, s0, s1) = z.data_ptr(), [c.data_ptr() for c in col]
    coef = torch.zeros(4, nf, dtype=torch.float64, device=DEV)
    cf = coef.data_ptr()
    need = L.gcn_bn_workspace_bytes(n, nf, 0)
    assert need == ((n + 63) // 64) * 4 * nf * 8
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    wp = ws.data_ptr()
    for bad in ((n, 7), (n, 24), (1, nf), (n, 2048)):
        assert L.gcn_bn_workspace_bytes(bad[0], bad[1], 0) == 0
    assert L.gcn_bn_workspace_bytes(n, nf, 5) == 0

    def calls(n, nf, zp=zp, m=m, cf=cf, need=need, wp=wp):
        return {
            "gcn_bn_stats": lambda: L.gcn_bn_stats(0, zp, n, nf, 1, EPS, m, v, r, wp, need, None),
            "gcn_bn_apply": lambda: L.gcn_bn_apply(0, zp, zp, n, nf, 1, m, r, None, None, None),
            "gcn_bn_backward_sums": lambda: L.gcn_bn_backward_sums(0, zp, zp, n, nf, 1, EPS, m, s0, s1, cf, wp, need, None),
            "gcn_bn_backward_apply": lambda: L.gcn_bn_backward_apply(0, zp, zp, zp, n, nf, 1, None, cf, None),
        }

    def expect(table, code):
        for name, call in table.items():
            assert call() == code, name
            assert L.gcn_last_error().decode().startswith(name + ":"), (name, L.gcn_last_error())

    expect(calls(n, 7), -1)                    # GCN_E_BADARG: F outside the shape rule
    expect(calls(1, nf), -1)                   # GCN_E_BADARG: n_rows < 2
    expect(calls(n, nf, zp=None), -1)          # GCN_E_BADARG: NULL tensor
    expect(calls(n, nf, m=None, cf=None), -1)  # GCN_E_BADARG: NULL column vector
    short = calls(n, nf, need=need - 1)
    expect({k: short[k] for k in ("gcn_bn_stats", "gcn_bn_backward_sums")}, -3)      # GCN_E_WORKSPACE
    none = calls(n, nf, wp=None)
    expect({k: none[k] for k in ("gcn_bn_stats", "gcn_bn_backward_sums")}, -3)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------- model
class ReluWithMask(torch.autograd.Function):
    """F.relu whose derivative is the given mask (see device_relu_masks)."""

    @staticmethod
    def forward(ctx, z, mask):
        ctx.save_for_backward(mask)
        return torch.relu(z)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0].to(g.dtype), None


def fork_forward(params, x, adj, masks=None):
    """reference pygcn/models.py:49,53,56 restated on the CPU (the fork's own forward calls .cuda()).
    Returns the output and the three pre-activations."""
    pre = []

    def gc(x, i):
        pre.append(torch.sparse.mm(adj, x @ params[f"gc{i}.weight"]) + params[f"gc{i}.bias"])
        return pre[-1]

    def relu(z):
        return F.relu(z) if masks is None else ReluWithMask.apply(z, masks[len(pre) - 1])

    def apply_bn(x):
        return nn.BatchNorm1d(x.size()[1]).to(x.dtype)(x)
    x = apply_bn(relu(gc(x, 1)))
    x = apply_bn(relu(gc(x, 2)))
    return relu(gc(x, 3)), pre


def device_relu_masks(model, x, adj_dev):
    """The ReLU derivatives the DEVICE used, layer by layer: the calls GCNBatchNorm.forward makes, on
    deterministic kernels, with autograd on as in the step itself (a layer whose input needs no
    gradient may associate its two products the other way round)."""
    from pygcn_amd.functional import relu_batch_norm
    z1 = model.gc1(x, adj_dev)
    z2 = model.gc2(relu_batch_norm(z1), adj_dev)
    z3 = model.gc3(relu_batch_norm(z2), adj_dev)
    return [(z > 0).cpu() for z in (z1, z2, z3)]


def check_relu_masks(masks, state, x, adj_cpu, tol=1e-5):
    """A pre-activation within rounding of zero can sit on the other side of the ReLU on the CPU:
    invisible in the forward pass, but it switches one term of a weight / bias gradient on or off, and
    one term of a cancelling sum over 3000 vertices is 1e-2 of it (the float32 and float64 CPU
    evaluations of this very model differ by that much at one such element).  The derivative of ReLU
    at 0 is a convention, not arithmetic — as in tests/_sampling.py device_relu_mask, the comparison is
    made well-posed by handing the reference the device's masks AFTER asserting that they differ from
    the float64 reference's only where its own pre-activation is within `tol` of zero, and on fewer
    than 1e-4 of the elements.  The count of each layer goes into the suite's ledger; measured on the
    MI355X: 0 in all three layers, on Cora and on the random graph."""
    with torch.no_grad():
        _, pre = fork_forward({k: v.double() for k, v in state.items()}, x.double(), adj_cpu.to(torch.float64))
    for i, (mask, z) in enumerate(zip(masks, pre)):
        flips = mask != (z > 0)
        _record(f"layer {i + 1}: share of ReLU derivatives that differ from float64's", int(flips.sum()),
                flips.numel(), 1e-4)
        if flips.any():
            assert float(z[flips].abs().max()) <= tol * float(z.abs().max()), "masks differ away from the ReLU boundary"
        assert float(flips.float().mean()) < 1e-4


def _cpu_model_step(state, x, adj, cot, dtype, masks):
    params = {k: v.detach().clone().to(dtype).requires_grad_() for k, v in state.items()}
    out, _ = fork_forward(params, x.to(dtype), adj.to(dtype), masks)
    out.backward(cot.to(dtype))
    return out.detach().numpy(), {k: p.grad.numpy() for k, p in params.items()}


def _model_case(name):
    from pygcn_amd import CSRGraph
    from pygcn_amd.utils import load_data, rmat_graph
    if name == "cora":
        adj = load_data(os.path.join(GOLDEN, "cora_graph.npz"))[0].coalesce()
        return adj, adj.to(DEV), torch.from_numpy(gin.cora_features()), (1433, 16, 7)
    n = 3000
    rowptr, col, val = rmat_graph(n, 30000, seed=5, device="cpu")
    adj = torch.sparse_csr_tensor(rowptr.long(), col.long(), val, (n, n))
    return adj, CSRGraph(rowptr.to(DEV), col.to(DEV), val.to(DEV), (n, n)), seeded((n, 256), 51), (256, 256, 256)


@pytest.mark.parametrize("case", ["cora", "random3000"])
def test_model_matches_the_fork_forward_on_the_cpu(case, monkeypatch):
    from pygcn_amd import GCNBatchNorm
    adj_cpu, adj_dev, x, dims = _model_case(case)
    torch.manual_seed(42)
    model = GCNBatchNorm(*dims, dropout=0.5, NN=3)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    cot = seeded((x.shape[0], dims[2]), 52)
    model = model.to(DEV).train()
    xd = x.to(DEV)
    with monkeypatch.context() as m:          # the normalisation runs on the HIP route
        m.setattr(torch.nn.functional, "batch_norm", None)
        out = model(xd, adj_dev)
        out.backward(cot.to(DEV))
        train_out = out.detach().clone()
        model.eval()                          # a fresh BatchNorm1d per call: batch statistics in eval too
        assert torch.equal(model(xd, adj_dev).detach(), train_out)
        masks = device_relu_masks(model, xd, adj_dev)
    torch.cuda.synchronize()
    check_relu_masks(masks, state, x, adj_cpu)
    out32, grads32 = _cpu_model_step(state, x, adj_cpu, cot, torch.float32, masks)
    out64, grads64 = _cpu_model_step(state, x, adj_cpu, cot, torch.float64, masks)
    assert_parity(train_out.cpu().numpy(), out32, out64, f"{case}: output")
    assert sorted(grads32) == ["gc1.bias", "gc1.weight", "gc2.bias", "gc2.weight", "gc3.bias", "gc3.weight"]
    for k in grads32:
        mod, name = k.split(".")
        got = getattr(getattr(model, mod), name).grad.cpu().numpy()
        assert_parity(got, grads32[k], grads64[k], f"{case}: {k}.grad")
