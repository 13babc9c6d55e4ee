"""The input side of the fork's evaluator GCN_OVER_MLP (reference pygcn/models.py:333-355): its input is ONE
tensor x [k, N, F] (reference pygcn/gnn-over-mlp.py:219-237, F = 9 or 17) of which the GCN reads the columns
[:d] (d = dim_touched, :345), the columns [d:F-1] are pooled as they are (:351), and the last column is the 0/1
vertex flag PoolLayer multiplies by and whose non-zero count it divides by (:272, :279).

    wide[n, j*d + c] = x[j, n, c], c < d         the [N, k*d] layout GraphConvolution.forward_wide takes
    mask[j, n]       = m(j, n)                   the [k, N] layout masked_mean_pool reads
    esum[j, c - d]   = sum_n m(j, n) * x[j, n, c], d <= c < F-1
    nonzero[j]       = #{n : m(j, n) != 0}

with m = `flag` when it is given and x[:, :, -1] otherwise.  Two full-height HIP sweeps
(pygcn_amd/csrc/gcn_eval.hip) behind ONE autograd node: gcn_eval_ingest reads x once and writes all four,
gcn_eval_ingest_backward reads x and the three gradients once and writes dx (and the flag's gradient) once.
Nothing of size [k, N, C + F - d] — the fork's `torch.cat` (:351) — exists, and nothing synchronises with the
host: the count stays on the device.
"""
import torch

from . import _native


def supported(x, d, flag=None):
    """True when the HIP sweeps take the call: a contiguous fp32 [k, N, F] tensor on the HIP device inside the
    shape rule of gcn_eval_workspace_bytes (2 <= F <= 64, 0 <= d <= F - 1, k <= 65535, N >= 1), and `flag`, if
    given, fp32 on the same device."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 3 and x.dtype == torch.float32
            and x.is_contiguous() and x.numel() > 0):
        return False
    if flag is not None and not (flag.device == x.device and flag.dtype == torch.float32):
        return False
    k, n, f = x.shape
    return _native.lib().gcn_eval_workspace_bytes(n, f, d, k) != 0


def ingest(x, d, flag=None):
    """(wide [N, k*d], mask [k, N], esum double [k*e], nonzero int64 [k]) of the contiguous fp32 `x` [k, N, F]
    and the contiguous fp32 `flag` [k, N] or None: one launch of gcn_eval_ingest and its finish."""
    k, n, f = x.shape
    wide = torch.empty((n, k * d), dtype=torch.float32, device=x.device)
    mask = torch.empty((k, n), dtype=torch.float32, device=x.device)
    esum = torch.empty(k * (f - 1 - d), dtype=torch.float64, device=x.device)
    nonzero = torch.empty(k, dtype=torch.int64, device=x.device)
    _native.launch("gcn_eval_ingest", x.device, x.data_ptr(), flag.data_ptr() if flag is not None else None, n, f, d,
                   k, wide.data_ptr(), mask.data_ptr(), esum.data_ptr(), nonzero.data_ptr(),
                   workspace=_native.lib().gcn_eval_workspace_bytes(n, f, d, k))
    return wide, mask, esum, nonzero


def ingest_backward(x, d, flag, d_wide, d_mask, d_esum, need_dx=True, need_dflag=False):
    """(dx [k, N, F] or None, dflag [k, N] or None): one launch of gcn_eval_ingest_backward.  The gradients are
    contiguous fp32 tensors ([N, k*d], [k, N], [k, e]) or None, which is zero."""
    k, n, f = x.shape
    dx = torch.empty_like(x) if need_dx else None
    dflag = torch.empty((k, n), dtype=torch.float32, device=x.device) if need_dflag else None
    ptr = lambda t: t.data_ptr() if t is not None else None     # noqa: E731
    _native.launch("gcn_eval_ingest_backward", x.device, x.data_ptr(), ptr(flag), ptr(d_wide), ptr(d_mask),
                   ptr(d_esum), n, f, d, k, ptr(dx), ptr(dflag))
    return dx, dflag


class EvaluatorIngestFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flag, d):
        k, n, f = x.shape
        flag_kn = flag.detach().reshape(k, n).contiguous() if flag is not None else None
        wide, mask, esum, nonzero = ingest(x, d, flag_kn)
        ctx.d = d
        ctx.flag_shape = flag.shape if flag is not None else None
        ctx.save_for_backward(x, flag_kn)
        ctx.set_materialize_grads(False)
        # (without a gradient for x, `wide` is a constant: layer 1 of the GCN then forms no input gradient)
        ctx.mark_non_differentiable(*((nonzero,) if ctx.needs_input_grad[0] else (nonzero, wide)))
        return wide, mask, esum.view(k, f - 1 - d).float(), nonzero

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_wide, g_mask, g_esum, g_nonzero):
        x, flag_kn = ctx.saved_tensors
        need_dx, need_dflag = ctx.needs_input_grad[0], flag_kn is not None and ctx.needs_input_grad[1]
        if not (need_dx or need_dflag):
            return None, None, None
        as32 = lambda g: g.to(torch.float32).contiguous() if g is not None else None     # noqa: E731
        dx, dflag = ingest_backward(x, ctx.d, flag_kn, as32(g_wide) if need_dx else None, as32(g_mask), as32(g_esum),
                                    need_dx, need_dflag)
        return dx, dflag.view(ctx.flag_shape) if need_dflag else None, None


def _flag_kn(x, flag):
    k, n = x.shape[0], x.shape[1]
    if tuple(flag.shape) != (k, n) and not (k == 1 and tuple(flag.shape) in ((n,), (n, 1))):
        raise RuntimeError(f"evaluator_ingest: flag {tuple(flag.shape)} does not go with x {tuple(x.shape)}: "
                           "expected [k, N] (for k = 1 also [N] or [N, 1])")
    return flag


def evaluator_ingest(x, dim_touched, flag=None):
    """`(wide, mask, esum, nonzero)` of the evaluator's input x [k, N, F] (module docstring), d = dim_touched:

        wide    = x[:, :, :d].permute(1, 0, 2).reshape(N, k * d)
        mask    = x[:, :, -1], or `flag` as [k, N] when it is given
        esum    = (x[:, :, d:-1] * mask[:, :, None]).sum(1)          [k, F - 1 - d], x's dtype
        nonzero = (mask != 0).sum(1)                                 int64 [k]; a NaN counts, as torch.nonzero

    `flag`: [k, N], and for k = 1 also [N] or [N, 1] (what `Generator` returns) — the device-friendly form of the
    fork's `cat(..., vac_flag)` (reference pygcn/policy-generator.py:398): the data columns of x stay constant
    and the flag arrives on its own; the last column of x is then not read.  Gradients go to `x`, if it requires
    one, and to `flag`, if it is given and requires one; `nonzero` has none.

    On the HIP device, for a contiguous fp32 x with 2 <= F <= 64 (and an fp32 flag), this is one autograd node
    over two HIP sweeps (pygcn_amd/csrc/gcn_eval.hip: esum is summed in double in a fixed order and rounded
    once); CPU tensors, other dtypes, a non-contiguous x and other shapes take the torch composition above."""
    if x.dim() != 3:
        raise RuntimeError(f"evaluator_ingest: x must be [k, N, F], got {tuple(x.shape)}")
    k, n, f = x.shape
    d = int(dim_touched)
    if f < 1 or not 0 <= d <= f - 1:
        raise RuntimeError(f"evaluator_ingest: dim_touched = {d} does not go with {f} columns, the last one the flag")
    if flag is not None:
        flag = _flag_kn(x, flag)
    if supported(x, d, flag):
        return EvaluatorIngestFunction.apply(x, flag, d)
    wide = x[:, :, :d].permute(1, 0, 2).reshape(n, k * d)
    mask = flag.reshape(k, n).to(x.dtype) if flag is not None else x[:, :, f - 1]
    esum = (x[:, :, d:f - 1] * mask.unsqueeze(2)).sum(1)
    return wide, mask, esum, (mask != 0).sum(1)
