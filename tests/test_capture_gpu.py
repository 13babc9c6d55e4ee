"""Every launching entry point and every training step under hipGraph capture and replay (tests/_capture.py).

Part A — one case per kernel family (the table CAPTURED of tests/test_capture_cpu.py): static inputs, a callable
through the Python wrapper, a refill that writes new contents of the same shape in place.  run_case holds, bit for bit:
the replay against the eager call on the same contents; after a refill (the second one scaled by 64) the replay
against the eager call on the new contents, and different from the first; and one eager call between capture and
first replay against the eager call before the capture.  Every replay starts from NaN-filled outputs.  The kernels
use integer atomics and atomicMax only and no case goes through a torch op that is not run-to-run deterministic, so
all comparisons with eager runs are exact.

Part B — training steps (zero_grad, forward, loss, backward, update) replayed 4 times from a saved state against 4
eager steps, bitwise with dropout 0, and against a float64 torch evaluation of the same steps at the project's 1e-5;
with dropout 0.5 every replay against the eager function at the seed the replay left in the device seed tensor.

What may change between replays and what may not is INTEGRATION.md §2, "The capture contract"."""
import numpy as np
import pytest
import torch

import _agglin_ref as AR
import _f64 as F64
from _capture import any_differs, assert_bitwise, bits_equal, capture, snapshot
from conftest import assert_normwise, load_golden
from test_capture_cpu import CAPTURED
from test_select_gpu import LaunchSpy, g7_model, n_big

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASE_NAMES = set()
SEEN = {}                 # case -> entry points launched inside its captures


def case(name):
    """Marks a test as (a variant of) the capture case `name` of the table CAPTURED."""
    def mark(fn):
        CASE_NAMES.add(name)
        fn.case_name = name
        return fn
    return mark


@pytest.fixture
def spy(monkeypatch):
    return LaunchSpy(monkeypatch)


def rnd(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


class Inputs:
    """Static device tensors with the recipe of their contents: add(name, maker) allocates maker(0, 1.0) on the
    device; refill(s) writes maker(s, 64 if s else 1) into every tensor IN PLACE."""

    def __init__(self):
        self.t, self.makers = {}, {}

    def add(self, name, maker):
        self.makers[name] = maker
        self.t[name] = maker(0, 1.0).to(DEV).contiguous()
        return self.t[name]

    def normal(self, name, shape, seed, dtype=torch.float32):
        return self.add(name, lambda s, scale: rnd(shape, seed + 101 * s, scale, dtype))

    def refill(self, s):
        with torch.no_grad():
            for name, maker in self.makers.items():
                self.t[name].copy_(maker(s, 64.0 if s else 1.0).to(self.t[name].dtype))


def run_case(name, spy, fn, refill):
    """The four assertions of a case (module docstring).  Returns the entry points its capture launched."""
    refill(0)
    want0 = snapshot(fn())
    assert want0 and all(t.numel() for t in want0), f"{name}: the callable returned nothing to compare"
    cap = capture(fn, spy)
    launched = set(cap.launched)
    assert launched <= set(CAPTURED), f"{name}: the capture launched {sorted(launched - set(CAPTURED))}, which " \
                                      "tests/test_capture_cpu.py lists as not capturable"
    SEEN.setdefault(name, set()).update(launched)
    assert_bitwise(snapshot(fn()), want0, f"{name}: eager call after the capture, before any replay")
    got0 = cap.replay()
    assert_bitwise(got0, want0, f"{name}: first replay")
    refill(1)
    got1 = cap.replay()
    want1 = snapshot(fn())
    assert_bitwise(got1, want1, f"{name}: replay after the in-place refill")
    assert any_differs(got1, got0), f"{name}: the refill changed no output"
    again = cap.replay()
    assert_bitwise(again, want1, f"{name}: a second replay on the same contents")
    torch.cuda.synchronize()
    return launched


def skewed_graph(n=1500, avg=6, seed=91, hub=(4, 600), sort=False):
    """The 1500-row skewed CSR of test_spmm_gpu's dropout replay test: Poisson(6) rows and one 600-entry hub row, so
    the long-row reduce kernel is inside the graph."""
    from pygcn_amd import CSRGraph
    rng = np.random.default_rng(seed)
    deg = rng.poisson(avg, size=n)
    deg[hub[0]] = hub[1]
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = rng.integers(0, n, size=int(rowptr[-1])).astype(np.int32)
    if sort:
        for r in range(n):
            col[rowptr[r]:rowptr[r + 1]] = np.sort(col[rowptr[r]:rowptr[r + 1]])
    val = (1.0 - rng.random(int(rowptr[-1]))).astype(np.float32)
    return CSRGraph(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(val).to(DEV), (n, n))


@pytest.fixture(scope="module")
def graph():
    g = skewed_graph()
    g.plan()
    return g


@pytest.fixture
def scheme_of():
    """set(name): switches the GEMM scheme inside a test; restored afterwards."""
    from pygcn_amd import spmm as S
    before = S.gemm_scheme()
    yield S.set_gemm_scheme
    S.set_gemm_scheme(before)


# ================================================================================================= A. entry points
@case("spmm_c_abi")
@pytest.mark.parametrize("F", [7, 64, 256])
def test_spmm_c_abi(spy, graph, F):
    """gcn_spmm_csr, the entry point without the epilogue struct (no Python wrapper launches it): plain, bias + ReLU."""
    from pygcn_amd import _native
    inp = Inputs()
    B, bias = inp.normal("B", (1500, F), 1), inp.normal("bias", (F,), 2)
    plan = graph.plan(torch.float32)
    need = _native.lib().gcn_spmm_workspace_bytes(plan, F)

    def fn():
        outs = []
        for b, relu in ((None, 0), (bias, 1)):
            out = torch.empty((1500, F), device=DEV)
            _native.launch("gcn_spmm_csr", DEV, plan, _native.GCN_DTYPE_F32, B.data_ptr(), B.stride(0), out.data_ptr(),
                           out.stride(0), F, b.data_ptr() if b is not None else None, relu, workspace=need)
            outs.append(out)
        return outs
    run_case("spmm_c_abi", spy, fn, inp.refill)


SPMM_OPTIONS = [("plain", 7, "f32"), ("plain", 64, "f32"), ("plain", 256, "f32"), ("plain", 64, "bf16"),
                ("plain", 256, "bf16"), ("bias", 64, "f32"), ("relu", 64, "f32"), ("relu", 256, "bf16"),
                ("dropout", 7, "f32"), ("dropout", 64, "f32"), ("dropout", 256, "f32"), ("dropout", 64, "bf16"),
                ("log_softmax", 7, "f32"), ("log_softmax", 64, "f32"), ("log_softmax", 256, "f32"),
                ("row_flags", 64, "f32"), ("skip_zero_rows", 64, "f32"), ("c_absmax", 256, "f32"),
                ("two_blocks", 64, "f32"), ("b_hint", 256, "f32")]


@case("spmm_epilogue")
@pytest.mark.parametrize("option,F,dt", SPMM_OPTIONS, ids=[f"{o}-{f}-{d}" for o, f, d in SPMM_OPTIONS])
def test_spmm_epilogue(spy, graph, option, F, dt):
    from pygcn_amd import spmm_csr
    from pygcn_amd.spmm import row_bitmap
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    inp = Inputs()
    B, bias = inp.normal("B", (1500, F), 3, dtype), inp.normal("bias", (F,), 4)
    seed_t = inp.add("seed", lambda s, scale: torch.tensor([123456789012345 + 977 * s], dtype=torch.int64))
    n = 1500
    if option == "b_hint":          # an operand with 7 rows in 8 zero: below the share at which the hint is honoured
        keep = (torch.arange(n) % 8 == 3).to(torch.float32).view(n, 1)
        inp.makers["B"] = lambda s, scale: rnd((n, F), 3 + 101 * s, scale) * keep

    def fn():
        if option == "plain":
            return spmm_csr(graph, B)
        if option == "bias":
            return spmm_csr(graph, B, bias=bias)
        if option == "relu":
            return spmm_csr(graph, B, bias=bias, relu=True)
        if option == "dropout":
            return spmm_csr(graph, B, bias=bias, relu=True, dropout_p=0.5, seed=seed_t)
        if option == "log_softmax":
            return spmm_csr(graph, B, bias=bias, log_softmax=True)
        if option in ("row_flags", "skip_zero_rows"):
            flags = torch.zeros(n, dtype=torch.uint8, device=DEV)
            out = spmm_csr(graph, B, relu=True, c_flags=flags, skip_zero_rows=option == "skip_zero_rows")
            if option == "skip_zero_rows":      # only the flagged rows of the result are defined
                out = torch.where(flags.bool().view(n, 1), out, torch.zeros_like(out))
            return out, flags
        if option == "c_absmax":
            top = torch.zeros(1, device=DEV)
            return spmm_csr(graph, B, bias=bias, relu=True, c_absmax=top), top
        if option == "two_blocks":
            return spmm_csr(graph, B[:1000], B2=B[1000:])
        if option == "b_hint":
            return spmm_csr(graph, B, b_hint=row_bitmap(B))
        raise AssertionError(option)
    launched = run_case("spmm_epilogue", spy, fn, inp.refill)
    assert launched == {"gcn_spmm_csr_ep"}
    if option == "dropout":         # the replayed mask is the mask of the tensor's value as a host seed
        eager = spmm_csr(graph, B, bias=bias, relu=True, dropout_p=0.5, seed=int(seed_t.item()))
        assert bits_equal(eager, fn())


@case("packed_rows")
def test_packed_rows(spy, graph):
    """rows_pack512 / rows_pack384 with their products: the activation is relu(normal - 0.7), 24 % non-zero, with
    every 16th row dense so that rows overflow their slots and are gathered from the matrix itself."""
    from pygcn_amd import spmm_csr
    from pygcn_amd.spmm import rows_pack384, rows_pack512
    inp = Inputs()
    dense_rows = (torch.arange(1500) % 16 == 5).view(1500, 1)

    def maker(s, scale):
        h = rnd((1500, 256), 5 + 101 * s)
        return torch.where(dense_rows, h.abs() + 0.1, torch.relu(h - 0.7)) * scale
    h = inp.add("h", maker)

    def fn():
        return spmm_csr(graph, packed=rows_pack512(h)), spmm_csr(graph, packed=rows_pack384(h))
    launched = run_case("packed_rows", spy, fn, inp.refill)
    assert launched == {"gcn_rows_pack512", "gcn_spmm_csr_packed", "gcn_rows_pack384", "gcn_spmm_csr_packed384"}
    assert bits_equal(fn()[0], spmm_csr(graph, h)) and bits_equal(fn()[1], spmm_csr(graph, h))


@case("sddmm")
@pytest.mark.parametrize("F,dt", [(7, "f32"), (64, "f32"), (256, "f32"), (64, "bf16")])
def test_sddmm(spy, graph, F, dt):
    from pygcn_amd.spmm import sddmm_csr
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    inp = Inputs()
    G, B = inp.normal("G", (1500, F), 6, dtype), inp.normal("B", (1500, F), 7, dtype)
    run_case("sddmm", spy, lambda: sddmm_csr(graph, G, B), inp.refill)


@case("backward_sweeps")
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_backward_sweeps(spy, dt):
    """The four backward sweeps on 3001 rows of width 64 (skip_zero_rows included: every 5th row of `out` is zero)."""
    from pygcn_amd.spmm import backward_with_colsum, nll_log_softmax_backward, relu_dropout_backward, unpack_row_flags
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    n, F = 3001, 64
    inp = Inputs()
    live = (torch.arange(n) % 5 != 2).view(n, 1)
    grad = inp.normal("grad", (n, F), 8, dtype)
    out = inp.add("out", lambda s, scale: (torch.relu(rnd((n, F), 9 + 101 * s, scale)) * live).to(dtype))
    logp = inp.add("logp", lambda s, scale: torch.log_softmax(rnd((n, F), 10 + 101 * s, scale ** 0.25), 1).to(dtype))
    target = inp.add("target", lambda s, scale: torch.randint(0, F, (n,), generator=torch.Generator().manual_seed(s)))
    coef = inp.add("coef", lambda s, scale: torch.tensor([-scale / n]))

    def fn():
        plain = relu_dropout_backward(grad, out, 2.0)
        gp, colsum, hint = backward_with_colsum(grad.clone(), out, scale=2.0)
        gs, colsum_s, hint_s = backward_with_colsum(grad.clone(), out, scale=2.0, skip_zero_rows=True)
        gs = torch.where(unpack_row_flags(hint_s[0], n).view(n, 1), gs, torch.zeros_like(gs))   # the others: undefined
        unmasked = backward_with_colsum(grad.clone())[1]
        gl, colsum_l, hint_l = backward_with_colsum(grad.clone(), logp, log_softmax=True)
        gn, colsum_n = nll_log_softmax_backward(logp, target, coef)
        return plain, gp, colsum, hint, gs, colsum_s, hint_s, unmasked, gl, colsum_l, hint_l, gn, colsum_n
    launched = run_case("backward_sweeps", spy, fn, inp.refill)
    assert launched == {"gcn_relu_dropout_backward", "gcn_relu_dropout_backward_colsum",
                        "gcn_log_softmax_backward_colsum", "gcn_nll_log_softmax_backward_colsum"}


M_GEMM = 1024 + 37          # several 128-row tiles and a ragged last one


@case("gemm_c_abi")
def test_gemm_c_abi(spy):
    """gcn_gemm_xw256_f32, round 1's three-part kernel (no Python wrapper launches it)."""
    from pygcn_amd import _native
    inp = Inputs()
    X, W = inp.normal("X", (M_GEMM, 256), 11), inp.normal("W", (256, 256), 12)

    def fn():
        Y = torch.empty((M_GEMM, 256), device=DEV)
        _native.launch("gcn_gemm_xw256_f32", DEV, X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), Y.data_ptr(),
                       Y.stride(0), M_GEMM, workspace=_native.lib().gcn_gemm_xw256_workspace_bytes())
        return Y
    run_case("gemm_c_abi", spy, fn, inp.refill)


@case("gemm_xw256")
@pytest.mark.parametrize("form", ["plain", "forward_epilogue", "backward_mask", "gathered_rows", "first_in_graph"])
def test_gemm_xw256(spy, gemm_scheme, form):
    """gemm_xw256 under both schemes.  Under "h2" no bound is handed over: the reduction pass over X is part of the
    graph, so the replay after the x64 refill scales by the new maximum.  "first_in_graph": the call with no bound
    is the first launch of the graph (no zero fill of a y_absmax before it), behind the NaN fills of the replay:
    where torch's split reduction kept its capture-time result (profiles/capture_coverage.md, finding 4)."""
    from pygcn_amd.gemm import gemm_keep_bits_usable, gemm_xw256
    inp = Inputs()
    X, W, bias = inp.normal("X", (M_GEMM, 256), 13), inp.normal("W", (256, 256), 14), inp.normal("bias", (256,), 15)
    mask_src = inp.normal("mask_src", (M_GEMM, 256), 16)
    seed_t = inp.add("seed", lambda s, scale: torch.tensor([-987654321987 - 31 * s], dtype=torch.int64))
    rows = torch.from_numpy(np.random.default_rng(3).permutation(M_GEMM)[:600].astype(np.int32)).to(DEV)

    def fn():
        if form == "plain":
            top = torch.zeros(1, device=DEV)
            return gemm_xw256(X, W, y_absmax=top), top
        if form == "forward_epilogue":
            bits = torch.empty((M_GEMM, 8), dtype=torch.int32, device=DEV) if gemm_keep_bits_usable(X, None, 0.5) else None
            top = torch.zeros(1, device=DEV)
            Y = gemm_xw256(X, W, y_absmax=top, bias=bias, relu=True, dropout_p=0.5, seed=seed_t, keep_bits_out=bits)
            return Y, top, bits
        if form == "backward_mask":
            return gemm_xw256(X, W, mask_src=mask_src, mask_scale=2.0)
        if form == "first_in_graph":
            return gemm_xw256(X, W)
        return gemm_xw256(X, W, rows=rows)
    first = fn()
    assert (first[0] if isinstance(first, tuple) else first) is not None, "gemm_xw256 declined the operands"
    launched = run_case("gemm_xw256", spy, fn, inp.refill)
    assert launched == {"gcn_gemm_xw256_f32_h2" if gemm_scheme == "h2" else "gcn_gemm_xw256_f32_b3"}
    if form == "forward_epilogue":
        eager = gemm_xw256(X, W, bias=bias, relu=True, dropout_p=0.5, seed=int(seed_t.item()))
        assert bits_equal(eager, fn()[0])


@case("gemm_log_softmax")
def test_gemm_log_softmax(spy):
    from pygcn_amd.gemm import gemm_xw256_log_softmax
    inp = Inputs()
    X, bias = inp.normal("X", (M_GEMM, 256), 17), inp.normal("bias", (256,), 19)
    W = inp.add("W", lambda s, scale: rnd((256, 256), 18 + 101 * s, scale ** 0.25 / 16))
    assert gemm_xw256_log_softmax(X, W, bias) is not None
    launched = run_case("gemm_log_softmax", spy, lambda: gemm_xw256_log_softmax(X, W, bias), inp.refill)
    assert launched == {"gcn_gemm_xw256_f32_b3_logsoftmax"}


@case("gemm_bf16")
@pytest.mark.parametrize("K,N", [(128, 128), (128, 256), (256, 128)])
def test_gemm_bf16(spy, K, N):
    from pygcn_amd.gemm import gemm_bf16
    bf = torch.bfloat16
    inp = Inputs()
    X, W, bias = inp.normal("X", (M_GEMM, K), 20, bf), inp.normal("W", (K, N), 21, bf), inp.normal("bias", (N,), 22, bf)
    mask_src = inp.normal("mask_src", (M_GEMM, N), 23, bf)
    seed_t = inp.add("seed", lambda s, scale: torch.tensor([55555 + s], dtype=torch.int64))

    def fn():
        outs = (gemm_bf16(X, W), gemm_bf16(X, W, bias=bias, relu=True, dropout_p=0.5, seed=seed_t),
                gemm_bf16(X, W, mask_src=mask_src, mask_scale=2.0))
        assert all(o is not None for o in outs), "gemm_bf16 declined the operands"
        return outs
    launched = run_case("gemm_bf16", spy, fn, inp.refill)
    assert launched == {"gcn_gemm_xw_bf16"}


@case("weight_grad")
@pytest.mark.parametrize("form", ["b3", "b3_colsum", "h2", "bf16"])
def test_weight_grad(spy, scheme_of, form):
    """The three atg256 forms and atg_bf16, over all rows and over row lists.  Under "h2" the bounds are reduction
    passes recorded in the graph."""
    from pygcn_amd.gemm import weight_grad_rows
    scheme_of("h2" if form == "h2" else "bf16x3")
    dtype, width = (torch.bfloat16, 128) if form == "bf16" else (torch.float32, 256)
    inp = Inputs()
    A, G = inp.normal("A", (M_GEMM, width), 24, dtype), inp.normal("G", (M_GEMM, width), 25, dtype)
    rng = np.random.default_rng(4)
    ra = torch.from_numpy(rng.permutation(M_GEMM)[:333].astype(np.int32)).to(DEV)
    rg = torch.from_numpy(rng.permutation(M_GEMM)[:333].astype(np.int32)).to(DEV)

    def fn():
        kw = {"colsum_g": True} if form == "b3_colsum" else {}
        outs = weight_grad_rows(A, G, **kw), weight_grad_rows(A, G, ra, rg, **kw)
        assert all(o is not None for o in outs), "weight_grad_rows declined the operands"
        return outs
    launched = run_case("weight_grad", spy, fn, inp.refill)
    assert launched == {{"b3": "gcn_gemm_atg256_f32_b3", "b3_colsum": "gcn_gemm_atg256_f32_b3_colsum",
                         "h2": "gcn_gemm_atg256_f32", "bf16": "gcn_gemm_atg_bf16"}[form]}


def _bn_inputs(n, width, dtype):
    inp = Inputs()
    z, g = inp.normal("z", (n, width), 26, dtype), inp.normal("g", (n, width), 27, dtype)
    gamma, beta = inp.normal("gamma", (width,), 28), inp.normal("beta", (width,), 29)
    return inp, z, g, gamma, beta


@case("bn_sweeps")
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bn_sweeps(spy, dt):
    """The four 2-D ReLU + BatchNorm sweeps (pygcn_amd/norm.py launches the batched forms only)."""
    from pygcn_amd import _native
    from pygcn_amd.norm import _DTYPES
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    n, nf, eps = 3001, 32, 1e-5
    inp, z, g, gamma, beta = _bn_inputs(n, nf, dtype)
    code = _DTYPES[dtype]
    need = _native.lib().gcn_bn_workspace_bytes(n, nf, code)

    def fn():
        mean, var, rstd, sum_g, sum_gxhat = (torch.empty(nf, device=DEV) for _ in range(5))
        coef = torch.empty(4, nf, dtype=torch.float64, device=DEV)
        y, dz = torch.empty_like(z), torch.empty_like(z)
        _native.launch("gcn_bn_stats", DEV, code, z.data_ptr(), n, nf, 1, eps, mean.data_ptr(), var.data_ptr(),
                       rstd.data_ptr(), workspace=need)
        _native.launch("gcn_bn_apply", DEV, code, z.data_ptr(), y.data_ptr(), n, nf, 1, mean.data_ptr(),
                       rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr())
        _native.launch("gcn_bn_backward_sums", DEV, code, g.data_ptr(), z.data_ptr(), n, nf, 1, eps,
                       mean.data_ptr(), sum_g.data_ptr(), sum_gxhat.data_ptr(), coef.data_ptr(), workspace=need)
        _native.launch("gcn_bn_backward_apply", DEV, code, g.data_ptr(), z.data_ptr(), dz.data_ptr(), n, nf, 1,
                       gamma.data_ptr(), coef.data_ptr())
        return mean, var, rstd, y, sum_g, sum_gxhat, coef, dz
    launched = run_case("bn_sweeps", spy, fn, inp.refill)
    assert launched == {"gcn_bn_stats", "gcn_bn_apply", "gcn_bn_backward_sums", "gcn_bn_backward_apply"}


@case("bn_sweeps_batched")
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bn_sweeps_batched(spy, dt):
    from pygcn_amd.norm import bn_apply, bn_backward_apply, bn_backward_sums, bn_stats
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    n, nf, k = 3001, 32, 3
    inp, z, g, gamma, beta = _bn_inputs(n, k * nf, dtype)

    def fn():
        mean, var, rstd = bn_stats(z, True, 1e-5, batch=k)
        y = bn_apply(z, mean, rstd, gamma, beta, True, batch=k)
        sum_g, sum_gxhat, coef = bn_backward_sums(g, z, mean, True, 1e-5, batch=k)
        return mean, var, rstd, y, sum_g, sum_gxhat, coef, bn_backward_apply(g, z, coef, gamma, True, batch=k)
    launched = run_case("bn_sweeps_batched", spy, fn, inp.refill)
    assert launched == {"gcn_bn_stats_batched", "gcn_bn_apply_batched", "gcn_bn_backward_sums_batched",
                        "gcn_bn_backward_apply_batched"}


def _bernoulli(k, n, seed):
    return (torch.rand((k, n), generator=torch.Generator().manual_seed(seed)) < 0.4).to(torch.float32)


@case("masked_pool")
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_masked_pool(spy, dt):
    from pygcn_amd.pool import masked_broadcast, masked_colsum
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    n, k, c = 3001, 3, 16
    inp = Inputs()
    h, coef = inp.normal("h", (n, k * c), 30, dtype), inp.normal("coef", (k * c,), 31)
    mask = inp.add("mask", lambda s, scale: _bernoulli(k, n, 32 + s))

    def fn():
        return masked_colsum(h, mask, n, k, c), masked_broadcast(mask, coef, n, k, c, dtype)
    launched = run_case("masked_pool", spy, fn, inp.refill)
    assert launched == {"gcn_masked_colsum", "gcn_masked_broadcast"}


@case("attention")
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_attention(spy, dt):
    from pygcn_amd.attention import attn_backward, attn_normalize, attn_scores
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    n, k, c = 3001, 3, 16
    inp = Inputs()
    h, ds = inp.normal("h", (n, k * c), 33, dtype), inp.normal("ds", (k, n), 35)
    key = inp.add("key", lambda s, scale: rnd((k * c,), 34 + 101 * s, 0.3))      # (scores stay inside exp's range)

    def fn():
        scores, stats = attn_scores(h, key, n, k, c)
        attn = attn_normalize(scores, stats, out=torch.empty_like(scores))
        return scores, stats, attn, attn_backward(h, ds, key, n, k, c)
    launched = run_case("attention", spy, fn, inp.refill)
    assert launched == {"gcn_attn_scores", "gcn_attn_normalize", "gcn_attn_backward"}


@case("select")
def test_select(spy):
    """The radix select, the index rule, the flag and the race keys on three windows of n_big() rows (>= 3 blocks, a
    ragged last one); the race keys from a host seed and from a device seed."""
    from pygcn_amd.select import flag_above, kth_largest, race_keys, topk_indices
    k, n, kth = 3, n_big(), 100
    inp = Inputs()
    p = inp.add("p", lambda s, scale: rnd((k, n), 36 + 101 * s, scale).abs())
    seed_t = inp.add("seed", lambda s, scale: torch.tensor([424242 + 7 * s], dtype=torch.int64))

    def fn():
        keys_host = race_keys(p, 99)
        keys = race_keys(p, seed_t)
        thr, cnt = kth_largest(keys, kth)
        return keys_host, keys, thr, cnt, topk_indices(keys, kth, thr, cnt), flag_above(keys, thr)
    launched = run_case("select", spy, fn, inp.refill)
    assert launched == {"gcn_race_keys", "gcn_race_keys_dev", "gcn_select_kth", "gcn_select_indices", "gcn_topk_flag"}
    assert bits_equal(race_keys(p, seed_t), race_keys(p, int(seed_t.item())))     # the device seed IS that host seed
    with pytest.raises(RuntimeError, match="tensor seed"):
        race_keys(p, seed_t.int())


@case("eval_ingest")
def test_eval_ingest(spy):
    from pygcn_amd.evaluator import ingest, ingest_backward
    k, n, f, d = 3, 3001, 17, 8
    inp = Inputs()
    x = inp.normal("x", (k, n, f), 37)
    flag = inp.add("flag", lambda s, scale: _bernoulli(k, n, 38 + s) * scale)
    d_wide, d_mask = inp.normal("d_wide", (n, k * d), 39), inp.normal("d_mask", (k, n), 40)
    d_esum = inp.normal("d_esum", (k, f - 1 - d), 41)

    def fn():
        return (ingest(x, d, flag), ingest(x, d, None),
                ingest_backward(x, d, flag, d_wide, d_mask, d_esum, need_dx=True, need_dflag=True))
    launched = run_case("eval_ingest", spy, fn, inp.refill)
    assert launched == {"gcn_eval_ingest", "gcn_eval_ingest_backward"}


class _ThreeLinears(torch.nn.Module):
    def __init__(self, fin, h1, h2):
        super().__init__()
        self.linear1, self.linear2, self.linear3 = (torch.nn.Linear(fin, h1), torch.nn.Linear(h1, h2),
                                                    torch.nn.Linear(h2, 1))


@case("vertex_mlp")
@pytest.mark.parametrize("batch_norm", [False, True])
def test_vertex_mlp(spy, batch_norm):
    from pygcn_amd.functional import vertex_mlp
    n, c, f, d = 3001, 16, 12, 4
    torch.manual_seed(3)
    mlp = _ThreeLinears(c + f - d, 32, 16).to(DEV)
    params = list(mlp.parameters())
    inp = Inputs()
    h, x, g = inp.normal("h", (n, c), 42).requires_grad_(), inp.normal("x", (n, f), 43), inp.normal("g", (n, 1), 44)
    for i, prm in enumerate(params):          # the refill moves the parameters too (by 1/8, not by 64)
        start = prm.detach().cpu().clone()
        inp.makers[f"p{i}"] = lambda s, scale, start=start: start * (1.0 + 0.125 * s)
        inp.t[f"p{i}"] = prm.data

    def fn():
        scores, m1, m2 = vertex_mlp(h, x, d, mlp, batch_norm, return_masks=True)
        return scores, m1, m2, torch.autograd.grad(scores, [h] + params, g)
    launched = run_case("vertex_mlp", spy, fn, inp.refill)
    assert launched == {"gcn_vmlp_forward", "gcn_vmlp_backward"}


@case("dropout_rows")
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_dropout_rows(spy, dt):
    from pygcn_amd.spmm import dropout_rows
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    m, F = 1037, 256
    inp = Inputs()
    src = inp.normal("src", (m, F), 45, dtype)
    seed_t = inp.add("seed", lambda s, scale: torch.tensor([2 ** 40 + 13 * s], dtype=torch.int64))
    rows = torch.from_numpy(np.random.default_rng(5).integers(0, 20000, m)).to(DEV)

    def fn():
        return dropout_rows(src.clone(), rows, 0.5, seed_t), dropout_rows(src.clone(), None, 0.25, seed_t, row_base=77)
    launched = run_case("dropout_rows", spy, fn, inp.refill)
    assert launched == {"gcn_dropout_rows"}
    assert bits_equal(fn()[0], dropout_rows(src.clone(), rows, 0.5, int(seed_t.item())))


@case("bn_linear")
def test_bn_linear(spy):
    from pygcn_amd.functional import relu_batch_norm_linear
    n, k = 3001, 3
    inp = Inputs()
    z, w = inp.normal("z", (n, k * 32), 46).requires_grad_(), inp.normal("w", (32, 32), 47).requires_grad_()
    ds = inp.normal("ds", (n, k * 32), 48)

    def fn():
        s = relu_batch_norm_linear(z, w, batch=k)
        return s, torch.autograd.grad(s, [z, w], ds)
    launched = run_case("bn_linear", spy, fn, inp.refill)
    assert {"gcn_bn_linear_forward", "gcn_bn_linear_backward_sums", "gcn_bn_linear_backward_apply"} <= launched


@case("agg_linear")
@pytest.mark.parametrize("fin,k", [(8, 1), (16, 3)])
def test_agg_linear(spy, fin, k):
    """aggregate_linear at R.n_three_blocks rows (the backward sweep spans >= 3 blocks, the last one ragged) on the
    hub-and-empty-row matrix of tests/_agglin_ref.py."""
    from pygcn_amd import CSRGraph, _native
    from pygcn_amd.functional import aggregate_linear
    n = AR.n_three_blocks(_native.lib().gcn_agg_linear_partial_rows, fin, k)
    rowptr, col, val = AR.random_csr(n, 7)
    g = CSRGraph(rowptr.to(DEV), col.to(DEV), val.to(DEV), (n, n))
    inp = Inputs()
    x, cot = inp.normal("x", (n, k * fin), 49), inp.normal("cot", (n, k * 32), 52)
    w, b = inp.normal("w", (fin, 32), 50).requires_grad_(), inp.normal("b", (32,), 51).requires_grad_()

    def fn():
        y = aggregate_linear(x, g, w, b, batch=k, relu=True)
        return y, torch.autograd.grad(y, [w, b], cot)
    launched = run_case("agg_linear", spy, fn, inp.refill)
    assert {"gcn_agg_linear_forward", "gcn_agg_linear_backward"} <= launched


@case("gather")
def test_gather(spy):
    """gcn_gather_f32 (CSRGraph._share_verified launches it behind a host read): indices outside the source give 0."""
    from pygcn_amd import _native
    n_src, n = 5000, 7001
    inp = Inputs()
    src = inp.normal("src", (n_src,), 53)
    index = inp.add("index", lambda s, scale: torch.randint(-3, n_src + 3, (n,), dtype=torch.int32,
                                                            generator=torch.Generator().manual_seed(s)))

    def fn():
        out = torch.empty(n, device=DEV)
        _native.launch("gcn_gather_f32", DEV, src.data_ptr(), index.data_ptr(), n, n_src, out.data_ptr())
        return out
    run_case("gather", spy, fn, inp.refill)
    ref = torch.where((index >= 0) & (index < n_src), src[index.clamp(0, n_src - 1).long()], torch.zeros(n, device=DEV))
    assert bits_equal(fn(), ref)


@case("normalize_in_place")
@pytest.mark.parametrize("which", ["row", "sym"])
def test_normalize_in_place(spy, which):
    """row_normalize_ / sym_normalize_ write graph.val through its address: the callable copies the static values in
    first, so every replay normalises the current contents."""
    g = skewed_graph(seed=92)
    inp = Inputs()
    vals = inp.add("vals", lambda s, scale: (torch.rand(g.nnz, generator=torch.Generator().manual_seed(60 + s)) + 0.1)
                   * scale)

    def fn():
        g.val.copy_(vals)
        return (g.row_normalize_() if which == "row" else g.sym_normalize_()).val.clone()
    launched = run_case("normalize_in_place", spy, fn, inp.refill)      # (both are scale-free: the refill draws anew)
    assert launched == {"gcn_row_normalize_device" if which == "row" else "gcn_sym_normalize_device"}


@case("rows_unpack")
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_rows_unpack(spy, dt):
    """The receiving side of the compressed halo exchange: fixed shapes (the values arrive in a buffer sized by the
    sender), offsets from the receiver's own scan."""
    from pygcn_amd.spmm import rows_pack, rows_unpack
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    m, F = 1037, 64
    keep = torch.rand((m, F), generator=torch.Generator().manual_seed(6)) < 0.3          # the pattern stays, the
    bits, _, vals0 = rows_pack((rnd((m, F), 54) * keep).to(dtype).to(DEV))               # values are refilled
    inp = Inputs()
    vals = inp.add("vals", lambda s, scale: (rnd((vals0.numel(),), 55 + 101 * s, scale).abs() + 0.5).to(dtype))
    launched = run_case("rows_unpack", spy, lambda: rows_unpack(bits, vals, F), inp.refill)
    assert launched == {"gcn_bits_row_counts", "gcn_rows_unpack"}
    assert bool(((rows_unpack(bits, vals, F) != 0).cpu() == keep).all())


@case("transpose")
def test_transpose(spy):
    """CSRGraph.t() allocates from nnz, which the handle knows: the radix sort is capturable.  A fresh handle per call
    (t() is cached per handle); the values are the refilled data."""
    from pygcn_amd import CSRGraph
    g = skewed_graph(seed=93)
    inp = Inputs()
    vals = inp.normal("vals", (g.nnz,), 56)

    def fn():
        t = CSRGraph(g.rowptr, g.col, vals, g.shape, validate=False).t()
        return t.rowptr, t.col, t.val
    launched = run_case("transpose", spy, fn, inp.refill)
    assert launched == {"gcn_csr_transpose_device"}


@case("mirror")
def test_mirror(spy):
    """The mirror search of share_transpose(): positions and the four counters have fixed shapes; the host read of
    the counters comes after it in _share_verified and is not part of the captured call."""
    from pygcn_amd import CSRGraph
    n = 1500
    rng = np.random.default_rng(8)
    pairs = rng.integers(0, n, size=(6000, 2))
    both = np.unique(np.concatenate([pairs, pairs[:, ::-1], np.stack([np.arange(n)] * 2, 1)]), axis=0)    # symmetric, sorted
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(both[:, 0], minlength=n))]).astype(np.int32)
    g = CSRGraph(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(both[:, 1].astype(np.int32)).to(DEV),
                 torch.ones(len(both), device=DEV), (n, n))
    inp = Inputs()
    vals = inp.normal("vals", (g.nnz,), 57)

    def fn():
        g.val.copy_(vals)
        mirror, counts = g._mirror_counts()
        return mirror, counts, g.val[mirror.long()]
    launched = run_case("mirror", spy, fn, inp.refill)
    assert launched == {"gcn_csr_mirror_device"}
    assert fn()[1].tolist()[:3] == [0, 0, 0]            # sorted, unique, pattern-symmetric


# =============================================================================================== B. training steps
def rmat(n, edges, seed):
    from pygcn_amd import CSRGraph
    from pygcn_amd.utils import rmat_graph
    rowptr, col, val = rmat_graph(n, edges, seed=seed, device="cpu")
    g = CSRGraph(rowptr.to(DEV), col.to(DEV), val.to(DEV), (n, n))
    return g, (rowptr.to(DEV), col.to(DEV), val.to(DEV))


def steps64(state0, csr, x, y, idx, steps, make_opt):
    """`steps` training steps of the 2-layer model in float64 from `state0`: (losses, final parameters).  The sparse
    products are tests/_f64.py's (plain torch ops on the original arrays; autograd differentiates them in B)."""
    p = {k: v.detach().double().clone().requires_grad_() for k, v in state0.items()}
    opt = make_opt(list(p.values()))
    x64, losses = x.double(), []
    for _ in range(steps):
        opt.zero_grad()
        h = torch.relu(F64.spmm64(*csr, x64 @ p["gc1.weight"]) + p["gc1.bias"])
        logp = torch.log_softmax(F64.spmm64(*csr, h @ p["gc2.weight"]) + p["gc2.bias"], 1)
        loss = torch.nn.functional.nll_loss(logp[idx] if idx is not None else logp, y[idx] if idx is not None else y)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return losses, {k: v.detach() for k, v in p.items()}


class PlainSGD:
    """p.add_(p.grad, alpha=-lr), as the captured steps write it."""

    def __init__(self, params, lr):
        self.params, self.lr = list(params), lr

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def step(self):
        with torch.no_grad():
            for p in self.params:
                p.add_(p.grad, alpha=-self.lr)


def load_state(model, state, opt=None):
    """Parameters (and the optimiser's moments and step counts) back to the saved start, IN PLACE."""
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(state[k])
        if isinstance(opt, torch.optim.Optimizer):
            for st in opt.state.values():
                for t in st.values():
                    if isinstance(t, torch.Tensor):
                        t.zero_()


def check_training_step(spy, make_model, make_opt, make_opt64, forward_loss, x, y, idx, csr, refill, steps=4):
    """The protocol of part B for a 2-layer GCN at dropout 0.  forward_loss(model) -> loss."""
    torch.manual_seed(1)
    captured_model, eager_model = make_model(), make_model()
    state0 = {k: v.detach().clone() for k, v in captured_model.state_dict().items()}
    load_state(eager_model, state0)
    opt_c, opt_e = make_opt(captured_model.parameters()), make_opt(eager_model.parameters())

    def step_of(model, opt):
        def step():
            opt.zero_grad()
            loss = forward_loss(model)
            loss.backward()
            opt.step()
            return loss.detach()
        return step
    cap = capture(step_of(captured_model, opt_c), spy)
    assert set(cap.launched) <= set(CAPTURED), sorted(set(cap.launched) - set(CAPTURED))
    load_state(captured_model, state0, opt_c)            # (the warm-up steps moved parameters and moments)
    eager_step = step_of(eager_model, opt_e)
    losses = []
    for k in range(steps):
        got = cap.replay()[0]
        want = eager_step()
        assert bits_equal(got, want), f"loss of step {k}: replay {float(got)!r}, eager {float(want)!r}"
        for (name, a), b in zip(captured_model.state_dict().items(), eager_model.state_dict().values()):
            assert_bitwise([a], [b], f"{name} after step {k}")
        losses.append(float(got))
    losses64, final64 = steps64(state0, csr, x, y, idx, steps, make_opt64)
    print("losses", losses, "float64", losses64)
    assert_normwise(np.array(losses), np.array(losses64), what="loss trajectory of the replays vs float64")
    for name, v in captured_model.state_dict().items():
        assert_normwise(v.cpu().numpy(), final64[name].cpu().numpy(), what=f"{name} after {steps} replays vs float64")
    refill()
    got, want = cap.replay()[0], eager_step()
    assert bits_equal(got, want), f"loss after the refill: replay {float(got)!r}, eager {float(want)!r}"
    assert float(got) != losses[-1]
    for (name, a), b in zip(captured_model.state_dict().items(), eager_model.state_dict().values()):
        assert_bitwise([a], [b], f"{name} after the refill")
    torch.cuda.synchronize()
    return cap


def refill_of(x, y, seed, nclass):
    def refill():
        x.copy_(rnd(tuple(x.shape), seed, 64.0))
        y.copy_(torch.randint(0, nclass, tuple(y.shape), generator=torch.Generator().manual_seed(seed)))
    return refill


# The learning rate of tools/cora_epoch.py.  It also keeps the float64 comparison of the final parameters inside what
# the project promises: a gradient within 1e-5 of its float64 value (the contract of every gradient test) moves the
# parameters by lr * 4 steps * 1e-5 * max|grad|, which stays below 1e-5 * max|parameter| while 4 * lr * max|grad| <=
# max|parameter| (0.04 * max|grad| against 0.15 for the 256-wide weights).
LR = 0.01


def test_gcn_layer_by_layer_step_with_adam(spy, gemm_scheme):
    """n = 600, 48 -> 64 -> 16, Adam(capturable=True) as in tools/cora_epoch.py: below ROWGRAD_MIN_ROWS the model is
    the plain composition of two layer nodes."""
    from pygcn_amd import GCN
    n, dims = 600, (48, 64, 16)
    g, csr = rmat(n, 6000, 31)
    x, y = rnd((n, dims[0]), 70).to(DEV), torch.randint(0, dims[2], (n,), generator=torch.Generator().manual_seed(1)).to(DEV)
    idx = torch.arange(0, n, 3, device=DEV)

    def forward_loss(model):
        return torch.nn.functional.nll_loss(model(x, g)[idx], y[idx])
    check_training_step(spy, lambda: GCN(*dims, dropout=0.0).to(DEV).train(),
                        lambda ps: torch.optim.Adam(ps, lr=0.01, capturable=True),
                        lambda ps: torch.optim.Adam(ps, lr=0.01), forward_loss, x, y, idx, csr,
                        refill_of(x, y, 71, dims[2]))


N_ONE_NODE = 16384 + 37        # ROWGRAD_MIN_ROWS and a ragged tail


@pytest.fixture(scope="module")
def big():
    """The R-MAT graph of the one-node steps, about 10 entries per row."""
    from pygcn_amd.tuning import ROWGRAD_MIN_ROWS
    assert N_ONE_NODE == ROWGRAD_MIN_ROWS + 37
    g, csr = rmat(N_ONE_NODE, 10 * N_ONE_NODE, 32)
    g.plan(), g.t().plan()
    idx = torch.from_numpy(np.sort(np.random.default_rng(6).permutation(N_ONE_NODE)[:N_ONE_NODE // 10])).to(DEV)
    return g, csr, idx


def one_node_problem(dims, seed):
    x = rnd((N_ONE_NODE, dims[0]), seed).to(DEV)
    y = torch.randint(0, dims[2], (N_ONE_NODE,), generator=torch.Generator().manual_seed(seed)).to(DEV)
    return x, y


def forward_loss_of(form, x, y, g, idx, **kw):
    from pygcn_amd import functional as PF

    def forward_loss(model):
        if form == "rows":
            return torch.nn.functional.nll_loss(model(x, g, rows=idx, **kw), y[idx])
        if form == "select":                     # upstream's lines: the RowSelectable route
            return torch.nn.functional.nll_loss(model(x, g)[idx], y[idx])
        return PF.nll_loss(model(x, g), y)       # a loss over all vertices (the structural gradient)
    return forward_loss


@pytest.mark.parametrize("form", ["rows", "select", "all"])
@pytest.mark.parametrize("dims", [(48, 64, 16), (256, 256, 256)], ids=["48x64x16", "256x256x256"])
def test_gcn_one_node_step(spy, gemm_scheme, big, dims, form):
    """The one-node path at n = 16384 + 37 with plain SGD, in its three call forms.  256 -> 256 -> 256 takes the
    reassociated layer 1 and the keep bits; under "h2" the x64 refill of x must move the bound of max|X| that
    gemm.absmax_cached hands to the scaled GEMMs.

    Before gemm._absmax_staged these three "h2" cases replayed a plausible wrong loss after the refill (6.022947
    against 127.643677 eager): the graph began with torch's split one-output reduction of max|X|, and once any kernel
    (the NaN fill of the static loss) preceded the replay on the launching stream, that reduction left the
    capture-time bound in place (profiles/capture_coverage.md, finding 4)."""
    from pygcn_amd import GCN
    g, csr, idx = big
    x, y = one_node_problem(dims, 72)
    cap = check_training_step(spy, lambda: GCN(*dims, dropout=0.0).to(DEV).train(), lambda ps: PlainSGD(ps, LR),
                              lambda ps: torch.optim.SGD(ps, lr=LR), forward_loss_of(form, x, y, g, idx), x, y,
                              None if form == "all" else idx, csr, refill_of(x, y, 73, dims[2]))
    assert "gcn_spmm_csr_ep" in cap.launched


def test_restricted_forward_step(spy, gemm_scheme, big):
    from pygcn_amd import GCN
    g, csr, idx = big
    dims = (256, 256, 256)
    x, y = one_node_problem(dims, 74)
    check_training_step(spy, lambda: GCN(*dims, dropout=0.0).to(DEV).train(), lambda ps: PlainSGD(ps, LR),
                        lambda ps: torch.optim.SGD(ps, lr=LR),
                        forward_loss_of("rows", x, y, g, idx, restrict_forward=True), x, y, idx, csr,
                        refill_of(x, y, 75, dims[2]))


def test_input_product_cache_step(spy, gemm_scheme, big):
    """set_input_product_cache(True): a capture taken after the warm-up must still contain layer 1's sparse product,
    or a replay on refilled features returns the old Â·X.  Under "h2" the cached product and the cached bound of
    max|X| are both bypassed in the same capture."""
    from pygcn_amd import GCN, fused
    g, csr, idx = big
    dims = (256, 256, 256)
    x, y = one_node_problem(dims, 76)
    fused.set_input_product_cache(True)
    try:
        check_training_step(spy, lambda: GCN(*dims, dropout=0.0).to(DEV).train(), lambda ps: PlainSGD(ps, LR),
                            lambda ps: torch.optim.SGD(ps, lr=LR), forward_loss_of("rows", x, y, g, idx), x, y, idx, csr,
                            refill_of(x, y, 77, dims[2]))
    finally:
        fused.set_input_product_cache(False)
        g._input_product = None


@pytest.mark.parametrize("restricted", [False, True], ids=["full", "restricted"])
def test_dropout_step_replays_at_the_device_seed(spy, monkeypatch, gemm_scheme, big, restricted):
    """The 256-wide one-node step with dropout 0.5.  "bf16x3": the packed layer 2, the GEMM-store dropout, the keep
    bits; "h2": the dense layer 2 behind gcn_gemm_xw256_f32_h2 with the dropout in its store, its seed read on the
    device and its bounds formed in the graph; the restricted pass: dropout_rows with the device seed.  After each replay the device seed tensor holds the seed
    that replay used: the eager function at that value as a HOST seed, from the parameters the replay started from,
    gives the same output rows and the same four parameter gradients bit for bit.  Two replays mask differently."""
    from pygcn_amd import GCN, fused
    from pygcn_amd import spmm as S
    g, _, idx = big
    dims = (256, 256, 256)
    x, y = one_node_problem(dims, 78)
    torch.manual_seed(2)
    model, twin = GCN(*dims, dropout=0.5).to(DEV).train(), GCN(*dims, dropout=0.5).to(DEV).train()
    opt = PlainSGD(model.parameters(), LR)
    hidden = []
    real_forward = fused._gcn2_forward
    monkeypatch.setattr(fused, "_gcn2_forward", lambda *a, **kw: (lambda r: (hidden.append(r[1]), r)[1])(real_forward(*a, **kw)))

    def step():
        opt.zero_grad()
        out = model(x, g, rows=idx, restrict_forward=restricted)
        loss = torch.nn.functional.nll_loss(out, y[idx])
        loss.backward()
        grads = [p.grad.clone() for p in model.parameters()]
        opt.step()
        return out.detach(), loss.detach(), grads
    cap = capture(step, spy)
    h1 = hidden[-1]                                     # layer 1's output of the captured pass: the graph's memory
    seed_t = S._device_seeds[DEV.index]
    gemm = "gcn_gemm_xw256_f32_h2" if gemm_scheme == "h2" else "gcn_gemm_xw256_f32_b3"
    packed = {"gcn_rows_pack384", "gcn_spmm_csr_packed384", "gcn_gemm_xw256_f32_b3_logsoftmax"}
    wanted = {gemm} | ({"gcn_dropout_rows"} if restricted else packed if gemm_scheme == "bf16x3" else set())
    assert wanted <= set(cap.launched), sorted(set(cap.launched))
    if restricted or gemm_scheme == "h2":           # the packed route: the full pass under the default scheme only
        assert not packed & set(cap.launched), sorted(set(cap.launched))
    masks, seeds = [], []
    for k in range(3):
        before = {name: v.detach().clone() for name, v in model.state_dict().items()}
        out, loss, *grads = cap.replay()
        masks.append((h1 != 0).clone())
        seed = int(seed_t.item())
        seeds.append(seed)
        load_state(twin, before)
        twin.zero_grad()
        fn = fused.gcn2_rows_restricted if restricted else (lambda *a: fused.gcn2_rows(*a)[0])
        want = fn(x, twin.gc1, twin.gc2, g, idx, 0.5, seed)
        torch.nn.functional.nll_loss(want, y[idx]).backward()
        assert_bitwise([out], [want.detach()], f"replay {k}: output rows against the eager call at seed {seed}")
        assert_bitwise(grads, [p.grad for p in twin.parameters()], f"replay {k}: parameter gradients at seed {seed}")
        if k == 1:
            x.copy_(rnd(tuple(x.shape), 79, 64.0))      # the last replay runs on refilled features
    assert len(set(seeds)) == 3
    share = float((masks[0] != masks[1]).sum()) / float((masks[0] | masks[1]).sum())
    assert share > 0.25, f"two replays kept the same elements ({share:.3f} of the kept ones differ)"
    torch.cuda.synchronize()


def test_gcn_batch_norm_forward_backward(spy):
    """GCNBatchNorm, k = 3 samples side by side, random600x12 of tests/test_batched_norm_gpu.py."""
    import test_batched_norm_gpu as BN
    from pygcn_amd import GCNBatchNorm
    n, edges, dims, _ = BN.CASES["random600x12"]
    _, g = BN._graph(n, edges)
    torch.manual_seed(42)
    model = GCNBatchNorm(*dims, dropout=0.0, NN=3).to(DEV).train()
    params = list(model.parameters())
    inp = Inputs()
    x, cot = inp.normal("x", (3, n, dims[0]), 80), inp.normal("cot", (3, n, dims[2]), 81)

    def fn():
        out = model(x, g)
        return out, torch.autograd.grad(out, params, cot)
    launched = run_case("GCNBatchNorm", spy, fn, inp.refill)
    SEEN.pop("GCNBatchNorm")
    assert "gcn_bn_stats_batched" in launched and "gcn_bn_backward_apply_batched" in launched


def test_evaluator_forward_backward(spy):
    """GCN_OVER_MLP on fixture g9 (sample set a_): output, the flag's gradient, every parameter gradient."""
    from pygcn_amd import CSRGraph, GCN_OVER_MLP
    from test_evaluator_cpu import g9_case
    g9 = load_golden("g9_evaluator.npz")
    state, x0, _, d = g9_case(g9, "a_")
    dims = [int(v) for v in g9["dims"]]
    model = GCN_OVER_MLP(dims[0], dims[1], dims[2], 0.0, dims[5], dims[2] + x0.shape[2] - 1 - d, dims[3], dims[4],
                         dim_touched=d)
    model.load_state_dict(state, strict=True)
    model = model.to(DEV).train()
    params = list(model.parameters())
    graph = CSRGraph(torch.from_numpy(g9["rowptr"]).to(DEV), torch.from_numpy(g9["col"]).to(DEV),
                     torch.from_numpy(g9["val"]).to(DEV), (64, 64))
    inp = Inputs()

    def maker(s, scale):            # the fixture's samples; the refill scales the features, not the 0/1 flag column
        t = x0.clone() if s == 0 else x0.flip(0).clone()
        t[:, :, :-1] *= scale
        return t
    x = inp.add("x", maker).requires_grad_()

    def fn():
        out = model(x, graph)
        return out, torch.autograd.grad(out.sum(), [x] + params)
    launched = run_case("GCN_OVER_MLP", spy, fn, inp.refill)
    SEEN.pop("GCN_OVER_MLP")
    assert {"gcn_eval_ingest", "gcn_eval_ingest_backward"} <= launched


def test_soft_generator_policy_step_draws_anew_on_every_replay(spy):
    """SoftGenerator.select_action + saved_log_probs[-1].backward() on g7.  The draw inside the graph reads the
    device seed that the capture advances (select.sample_without_replacement, C-ABI gcn_race_keys_dev): replay k
    picks the vertices of the eager call with seed = the tensor's value after replay k, and two replays pick
    different sets.  Eagerly torch.manual_seed still reproduces a run (test_select_gpu)."""
    from pygcn_amd import spmm as S
    model, x, graph, nn_ = g7_model()
    params = list(model.parameters())

    def step():
        del model.saved_log_probs[:]
        for p in params:
            p.grad = None
        vac_flag, idx = model.select_action(x, graph)
        lp = model.saved_log_probs[-1]
        lp.backward()
        return vac_flag, idx, lp.detach(), [p.grad for p in params]
    cap = capture(step, spy)
    assert "gcn_race_keys_dev" in cap.launched and "gcn_race_keys" not in cap.launched
    seed_t = S._device_seeds[DEV.index]
    picks = []
    for k in range(3):
        vac_flag, idx, lp, *grads = cap.replay()
        seed = int(seed_t.item())
        del model.saved_log_probs[:]
        for p in params:
            p.grad = None
        want_flag, want_idx = model.select_action(x, graph, seed=seed)
        model.saved_log_probs[-1].backward()
        assert_bitwise([vac_flag, idx, lp], [want_flag, want_idx, model.saved_log_probs[-1].detach()],
                       f"replay {k}: the picks against the eager call at seed {seed}")
        assert_bitwise(grads, [p.grad for p in params], f"replay {k}: parameter gradients")
        assert int(vac_flag.sum()) == nn_
        picks.append(set(idx.tolist()))
    assert picks[0] != picks[1] and picks[1] != picks[2], "every replay drew the same vertices"
    torch.cuda.synchronize()


def test_capture_without_a_device_seed_is_a_named_error():
    """The one limit by design: the device seed tensor is created by the first EAGER dropout launch (or draw), so a
    capture of a dropout step with no eager step before it raises by name instead of freezing a host seed."""
    from pygcn_amd import spmm as S
    from pygcn_amd.functional import sample_without_replacement
    p = torch.rand(2, 500, device=DEV)
    kept = dict(S._device_seeds)
    S._device_seeds.clear()
    try:
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="before capturing it into a hipGraph"):
            with torch.cuda.graph(graph):
                sample_without_replacement(p, 10)
    finally:
        S._device_seeds.update(kept)
    torch.cuda.synchronize()


# ==================================================================================================== the table
def test_zz_the_cases_launched_exactly_the_captured_table():
    """The union of the entry points the cases of part A launched inside their captures is the table CAPTURED, and
    each case launched at least the entry points the table gives it.  (Run on its own, or with a selection of cases,
    it holds the cases that ran.)"""
    assert SEEN, "no capture case ran before this test"
    for name, launched in SEEN.items():
        mine = {ep for ep, c in CAPTURED.items() if c == name}
        assert mine <= launched, f"{name} did not launch {sorted(mine - launched)}"
    if set(SEEN) == CASE_NAMES:
        union = set().union(*SEEN.values())
        assert union == set(CAPTURED), f"never captured: {sorted(set(CAPTURED) - union)}"
        assert CASE_NAMES == set(CAPTURED.values())
