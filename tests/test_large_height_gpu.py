"""The kernels at the heights the project is graded at (C4: 10⁷ x 256 fp32, C5: 5·10⁷ x 128 bf16),
each run once at full height through its pygcn_amd.spmm wrapper and held against a float64 product
of the same inputs (tests/_f64.py) with the gates of the small-size tests — so that no output row
past element 2³¹ (or 2³²) of an operand goes unchecked.

Dense outputs are checked on: rows 0-127, 128-row windows straddling elements 2³¹ and 2³² of the
operand, the last 300 rows (the ragged last tile) and 2 000 random rows.  Reductions (weight
gradients, column sums) are checked whole."""
import pytest
import torch

import _f64
from conftest import assert_normwise

pytestmark = pytest.mark.gpu

M32 = (1 << 24) + 37            # fp32 [M, 256]: 2^32 + 9472 elements
M16 = (1 << 25) + 37            # bf16 [M, 128]: past 2^32 elements


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_between_tests():
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f"  peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def keep(oracle):
    return oracle.dropout_keep


def checked_rows(M, F, gen, device):
    """int64 row ids: first 128, windows across elements 2^31 and 2^32, last 300, 2000 random."""
    parts = [torch.arange(0, 128)]
    for el in (1 << 31, 1 << 32):
        r = el // F
        if r < M:
            parts.append(torch.arange(max(r - 64, 0), min(r + 64, M)))
    parts.append(torch.arange(M - 300, M))
    parts = [p.to(device) for p in parts]
    parts.append(torch.randint(0, M, (2000,), generator=gen, device=device))
    return torch.unique(torch.cat(parts))


def _row_gate(got, ref, rel, what):
    """per-row max|got - ref| <= rel * max|ref row| (rows span orders of magnitude)."""
    err = (got.double() - ref).abs().amax(1)
    scale = ref.abs().amax(1)
    worst = float((err / scale.clamp_min(1e-300)).max())
    assert bool((err <= rel * scale).all()), f"{what}: worst row err/scale {worst:.3e} > {rel:g}"
    return worst


def _ledger(what, worst, gate):
    from conftest import _record
    _record(what, worst, 1.0, gate)


def _scaled_rows(M, K, gen, device):
    X = torch.randn(M, K, generator=gen, device=device)
    X.mul_(torch.pow(10.0, 4 * torch.rand(M, 1, generator=gen, device=device) - 2))
    return X


def _popcount_rows(bits):
    return sum(((bits >> k) & 1).sum(1) for k in range(32))


def _pack_keep_bits(pos):
    """bool [m, 256] -> int32 [m, 8] in the lane order of gemm_xw256_s16_kernel's keep bits
    (gcn_gemm.hip, `kb` / `write_keep_bits`): lane q of a row writes words 2q, 2q + 1; bit 4·(cb & 7) + j of
    word 2q + (cb >> 3) is column 16·cb + 4q + j (cb = 0..15, j = 0..3)."""
    w = torch.arange(8, device=pos.device).view(8, 1)
    b = torch.arange(32, device=pos.device).view(1, 32)
    col = 16 * (8 * (w & 1) + (b >> 2)) + 4 * (w >> 1) + (b & 3)            # [8, 32]
    assert torch.equal(col.flatten().sort().values, torch.arange(256, device=pos.device))
    words = (pos[:, col].to(torch.int64) << b).sum(-1)                       # [m, 8] as uint32 values
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def test_fp32_gemm_full_height(dev, keep):
    """gemm_xw256 (default scheme, contiguous rows: gemm_xw256_s16_kernel) at M = 2^24 + 37: plain; the
    forward epilogue bias + ReLU + dropout 1/2 with keep bits; the grad_input form masked from those bits."""
    from pygcn_amd import gemm as S
    assert S.gemm_scheme() == "bf16x3"
    gen = torch.Generator(device=dev).manual_seed(2024)
    X = _scaled_rows(M32, 256, gen, dev)
    W = torch.randn(256, 256, generator=gen, device=dev)
    bias = torch.randn(256, generator=gen, device=dev) * 0.5
    rows = checked_rows(M32, 256, gen, dev)
    pre = X[rows].double() @ W.double()

    Y = S.gemm_xw256(X, W)
    assert Y is not None and Y.shape == (M32, 256)
    _ledger("fp32 GEMM plain, checked rows", _row_gate(Y[rows], pre, 2e-6, "plain"), 2e-6)
    del Y

    seed = 0x1234_5678_9ABC_DEF1
    bits = torch.full((M32, 8), -1, dtype=torch.int32, device=dev)
    H = S.gemm_xw256(X, W, bias=bias, relu=True, dropout_p=0.5, seed=seed, keep_bits_out=bits)
    pre_b = pre + bias.double()
    kp = torch.from_numpy(keep(seed, rows.cpu().numpy(), 256, 0.5)).to(dev)
    want = torch.where(kp & (pre_b > 0), 2.0 * pre_b, torch.zeros_like(pre_b))
    scale = pre_b.abs().amax(1, keepdim=True)
    err = (H[rows].double() - want).abs().amax(1, keepdim=True)
    worst = float((err / scale).max())
    assert bool((err <= 2 * 2e-6 * scale).all()), f"epilogue: {worst:.3e}"
    _ledger("fp32 GEMM bias+relu+dropout, checked rows (vs 2 max|pre|)", worst / 2, 2e-6)
    # keep decisions: off the ReLU boundary, the device keeps exactly the oracle's elements
    clear = pre_b.abs() > 2e-6 * scale
    assert torch.equal((H[rows] > 0)[clear], ((pre_b > 0) & kp)[clear])
    # keep bits: exactly the packed `H > 0` on the checked rows, one per positive output over the whole tensor
    assert torch.equal(bits[rows], _pack_keep_bits(H[rows] > 0))
    assert int(_popcount_rows(bits).sum()) == int((H > 0).sum())

    # grad_input form: mask from the bits == mask from the activations, and against float64
    W2 = torch.randn(256, 256, generator=gen, device=dev)
    want_src = S.gemm_xw256(X, W2, mask_src=H, mask_scale=2.0)
    Hd = H[rows].clone()
    H.fill_(float("nan"))                     # with bits, the activations are not read
    got = S.gemm_xw256(X, W2, mask_src=H, mask_scale=2.0, mask_bits=bits)
    del H
    assert torch.equal(got, want_src)
    del want_src
    g64 = X[rows].double() @ W2.double()
    ref = torch.where(Hd > 0, 2.0 * g64, torch.zeros_like(g64))
    err = (got[rows].double() - ref).abs().amax(1)
    worst = float((err / (2 * g64.abs().amax(1))).max())
    assert worst <= 2e-6, f"masked grad_input: {worst:.3e}"
    _ledger("fp32 GEMM mask_src + mask_bits, checked rows", worst, 2e-6)


@pytest.mark.parametrize("scheme", ["bf16x3", "h2"])
def test_fp32_gemm_row_list_and_h2_full_height(dev, scheme):
    """gemm_xw256 through a list of 10^6 random rows of a 2^24 + 37-row operand (round 3's listed-row
    pipeline; every output row checked), and the contiguous launch at full height under each scheme."""
    from pygcn_amd import gemm as S
    gen = torch.Generator(device=dev).manual_seed(77)
    X = _scaled_rows(M32, 256, gen, dev)
    W = torch.randn(256, 256, generator=gen, device=dev)
    lst = torch.randint(0, M32, (1_000_000,), generator=gen, device=dev)
    lst[:4] = torch.tensor([M32 - 1, 1 << 23, 1 << 24, (1 << 24) - 1], device=dev)
    assert int(lst.max()) == M32 - 1
    tol = 2e-6 if scheme == "bf16x3" else 4e-6
    before = S.gemm_scheme()
    S.set_gemm_scheme(scheme)
    try:
        Yl = S.gemm_xw256(X, W, rows=lst.to(torch.int32))
        ref = _f64.mm64(X.index_select(0, lst), W)
        _ledger(f"fp32 GEMM {scheme} row list, all 10^6 rows", _row_gate(Yl, ref, tol, "row list"), tol)
        del Yl, ref
        if scheme == "h2":
            rows = checked_rows(M32, 256, gen, dev)
            Y = S.gemm_xw256(X, W)
            _ledger("fp32 GEMM h2 plain, checked rows",
                    _row_gate(Y[rows], X[rows].double() @ W.double(), tol, "h2 plain"), tol)
    finally:
        S.set_gemm_scheme(before)


def test_bf16_gemm_full_height(dev, keep):
    """gemm_bf16 128 -> 128 at M = 2^25 + 37 (more than 2^32 elements): plain, the forward epilogue at
    p = 1/2, and the mask_src backward — against float64 on the same bf16 values."""
    from pygcn_amd.gemm import gemm_bf16
    gen = torch.Generator(device=dev).manual_seed(2025)
    X = torch.randn(M16, 128, generator=gen, device=dev).bfloat16()
    W = (torch.randn(128, 128, generator=gen, device=dev) * 0.2).bfloat16()
    bias = (torch.randn(128, generator=gen, device=dev) * 0.5).bfloat16()
    rows = checked_rows(M16, 128, gen, dev)
    pre = X[rows].double() @ W.double()

    def gate(got, ref, what):
        err = (got.double() - ref).abs()
        big = float(ref.abs().max())
        ok = err <= 2.0 ** -8 * ref.abs() + 1e-5 * big
        worst = float(((err - 2.0 ** -8 * ref.abs()).clamp_min(0)).max()) / big
        assert bool(ok.all()), f"{what}: {worst:.3e}"
        _ledger(f"bf16 GEMM {what}, checked rows (excess over 2^-8 |ref|)", worst, 1e-5)

    Y = gemm_bf16(X, W)
    assert Y is not None and Y.shape == (M16, 128)
    gate(Y[rows], pre, "plain")
    del Y
    seed = 987654321
    H = gemm_bf16(X, W, bias=bias, relu=True, dropout_p=0.5, seed=seed)
    pre_b = pre + bias.double()
    kp = torch.from_numpy(keep(seed, rows.cpu().numpy(), 128, 0.5)).to(dev)
    gate(H[rows], torch.where(kp & (pre_b > 0), 2.0 * pre_b, torch.zeros_like(pre_b)), "bias+relu+dropout")
    clear = pre_b.abs() > 1e-5 * float(pre_b.abs().max())
    assert torch.equal((H[rows] > 0)[clear], ((pre_b > 0) & kp)[clear])
    W2 = (torch.randn(128, 128, generator=gen, device=dev) * 0.2).bfloat16()
    got = gemm_bf16(X, W2, mask_src=H, mask_scale=2.0)
    g64 = X[rows].double() @ W2.double()
    gate(got[rows], torch.where(H[rows] > 0, 2.0 * g64, torch.zeros_like(g64)), "mask_src backward")


def _wgrad_gate(got, ref, summ, what):
    err = float((got.double() - ref).abs().max())
    s = float(summ.max())
    assert err <= 3e-7 * s, f"{what}: {err / s:.3e} of the summands"
    _ledger(what + " (err / max summands)", err / s, 3e-7)


def _colsum_check(cs, ref, f32, what):
    """A bias gradient against its float64 sum: fp32 normwise at the contract's 1e-5; bf16 (the result
    is rounded to bf16 once) elementwise 2^-8·|ref| + 1e-5·max|ref|, the bf16 GEMM gate."""
    if f32:
        assert_normwise(cs.cpu(), ref.cpu().numpy(), 1e-5, what)
        return
    err = (cs.double() - ref).abs()
    big = float(ref.abs().max())
    worst = float((err - 2.0 ** -8 * ref.abs()).clamp_min(0).max()) / big
    assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-5 * big).all()), f"{what}: {worst:.3e}"
    _ledger(what + " (excess over 2^-8 |ref|)", worst, 1e-5)


def _colsum_gate(cs, ref, absref, rel, what):
    """The weight-gradient kernels' side result: the gate of their small-size test (of max Σ|.|)."""
    err = float((cs.double() - ref).abs().max())
    s = float(absref.max())
    assert err <= rel * s, f"{what}: {err / s:.3e} of max Σ|.|"
    _ledger(what + " (err / max Σ|.|)", err / s, rel)


def test_fp32_weight_gradient_full_height(dev):
    """weight_grad_rows (atg256 b3 with the column sums) over all 10^7 + 13 rows, no list."""
    from pygcn_amd import gemm as S
    assert S.gemm_scheme() == "bf16x3"
    n = 10_000_013
    gen = torch.Generator(device=dev).manual_seed(31)
    A = torch.randn(n, 256, generator=gen, device=dev)
    G = torch.randn(n, 256, generator=gen, device=dev) * 0.01 + 0.003
    got, cs = S.weight_grad_rows(A, G, colsum_g=True)
    ref, summ = _f64.tn64(A, G, absolute=True)
    _wgrad_gate(got, ref, summ, "atg256 b3, 10^7+13 rows")
    s, sa = _f64.colsum64(G)
    _colsum_gate(cs, s, sa, 2e-7, "atg256 b3 colsum_g, 10^7+13 rows")


@pytest.mark.parametrize("scheme", ["bf16x3", "h2"])
def test_fp32_weight_gradient_row_lists_full_height(dev, scheme):
    """weight_grad_rows over lists of 5·10^6 rows into 1.6·10^7-row operands (gathers past element 2^31)."""
    from pygcn_amd import gemm as S
    n, m = 16_000_000, 5_000_000
    gen = torch.Generator(device=dev).manual_seed(32)
    A = torch.randn(n, 256, generator=gen, device=dev) * 3
    G = torch.randn(n, 256, generator=gen, device=dev) * 0.01 + 0.003
    ra = torch.randint(0, n, (m,), generator=gen, device=dev)
    ra[:2] = torch.tensor([n - 1, 1 << 23], device=dev)
    rg = torch.randperm(n, generator=gen, device=dev)[:m]
    rg[0] = n - 1
    before = S.gemm_scheme()
    S.set_gemm_scheme(scheme)
    try:
        res = S.weight_grad_rows(A, G, ra.to(torch.int32), rg.to(torch.int32), colsum_g=scheme == "bf16x3")
    finally:
        S.set_gemm_scheme(before)
    got, cs = res if scheme == "bf16x3" else (res, None)
    ref, summ = _f64.tn64(A, G, ra, rg, absolute=True)
    _wgrad_gate(got, ref, summ, f"atg256 {scheme}, lists of 5·10^6 rows")
    if cs is not None:
        s, sa = _f64.colsum64(G.index_select(0, rg))
        _colsum_gate(cs, s, sa, 2e-7, "atg256 b3 colsum_g over a list")


def test_bf16_weight_gradient_full_height(dev):
    """weight_grad_rows for bf16 [5·10^7, 128] operands (atg_bf16): fp32 accumulation, one rounding to bf16."""
    from pygcn_amd.gemm import weight_grad_rows
    n = 50_000_000
    gen = torch.Generator(device=dev).manual_seed(33)
    A = torch.randn(n, 128, generator=gen, device=dev).bfloat16()
    G = (torch.randn(n, 128, generator=gen, device=dev) * 0.01 + 0.003).bfloat16()
    got = weight_grad_rows(A, G)
    assert got is not None and got.dtype == torch.bfloat16
    ref = _f64.tn64(A, G)
    err, s = float((got.double() - ref).abs().max()), float(ref.abs().max())
    assert err <= 2.0 ** -8 * s, f"{err / s:.3e}"
    _ledger("atg bf16, 5·10^7 rows (err / max|ref|)", err / s, 2.0 ** -8)


@pytest.mark.parametrize("F,dtype,n", [(256, torch.float32, M32), (128, torch.bfloat16, 50_000_000)])
def test_backward_passes_full_height(dev, F, dtype, n):
    """backward_with_colsum (masked, unmasked, log_softmax), relu_dropout_backward and
    nll_log_softmax_backward (with ignored rows) at full height: grad_pre bit-exact where the small
    tests ask for it, column sums against float64 sums (_colsum_check).  The gradients have column
    means that do not cancel (as a bias gradient's), so the sums grow like n and the gate rejects a
    sum that misses or misreads a slab of rows."""
    from pygcn_amd.spmm import backward_with_colsum, nll_log_softmax_backward, relu_dropout_backward
    f32 = dtype == torch.float32
    gen = torch.Generator(device=dev).manual_seed(F)
    mu = 0.003 * (1.0 + torch.arange(F, device=dev) / F)            # (column means: sums that do not cancel)
    go = (torch.randn(n, F, generator=gen, device=dev) * 0.01 + mu).to(dtype)
    out = torch.randn(n, F, generator=gen, device=dev).to(dtype)
    go[::3] = 0
    rows = checked_rows(n, F, gen, dev)
    scale = 1.5 if f32 else 2.0
    # (bf16: the pass sums the STORED, rounded grad_pre values — so does the reference)
    stored = (lambda t: t) if f32 else (lambda t: t.to(dtype).double())      # noqa: E731

    # masked (the ReLU / dropout backward) and the standalone pass
    gp, cs, _ = backward_with_colsum(go, out, scale)
    want = torch.where(out > 0, go * scale, torch.zeros_like(go))
    assert torch.equal(gp, want)
    del gp
    assert torch.equal(relu_dropout_backward(go, out, scale), want)
    _colsum_check(cs, _f64.colsum64(want)[0], f32, f"colsum masked {dtype}")
    del want
    # unmasked
    gq, cq, _ = backward_with_colsum(go, None, 1.0)
    assert gq is go
    _colsum_check(cq, _f64.colsum64(go)[0], f32, f"colsum unmasked {dtype}")
    del out

    # log_softmax backward: rows of a loss gradient (5 % non-zero), log-probabilities
    logp = torch.empty(n, F, dtype=dtype, device=dev)
    for r in range(0, n, 1 << 22):
        logp[r:r + (1 << 22)] = torch.log_softmax(2.0 * torch.randn(min(1 << 22, n - r), F, generator=gen,
                                                                    device=dev), 1).to(dtype)
    go.mul_((torch.rand(n, 1, generator=gen, device=dev) < 0.05).to(dtype))
    gl, cl, _ = backward_with_colsum(go, logp, log_softmax=True)

    def lsm64(g, lp):
        g, lp = g.double(), lp.double()
        return g - lp.exp() * g.sum(1, keepdim=True)
    ref = lsm64(go[rows], logp[rows])
    tol = 1e-5 if f32 else 2.0 ** -6
    err = float((gl[rows].double() - ref).abs().max()) / float(ref.abs().max())
    assert err <= tol, f"log_softmax backward: {err:.3e}"
    _ledger(f"log_softmax backward {dtype}, checked rows", err, tol)
    del gl
    s = torch.zeros(F, dtype=torch.float64, device=dev)
    for r in range(0, n, 1 << 20):
        s += stored(lsm64(go[r:r + (1 << 20)], logp[r:r + (1 << 20)])).sum(0)
    _colsum_check(cl, s, f32, f"colsum log_softmax {dtype}")
    del go

    # NLL over all rows with ignored (-100) rows: coef·(onehot(target) − exp(logp))
    target = torch.randint(0, F // 4, (n,), generator=gen, device=dev)   # (a quarter of the classes: no cancelling)
    target[::7] = -100
    coef = torch.full((1,), -1.0 / n, device=dev)
    gn, cn = nll_log_softmax_backward(logp, target, coef)

    def nll64(lp, t):
        g = -lp.double().exp()
        g.scatter_add_(1, t.clamp_min(0).view(-1, 1), torch.ones(t.numel(), 1, dtype=torch.float64, device=dev))
        return g.mul_((t >= 0).double().unsqueeze(1) * float(coef))
    ref = nll64(logp[rows], target[rows])
    tol = 1e-5 if f32 else 2.0 ** -7
    err = float((gn[rows].double() - ref).abs().max()) / float(ref.abs().max())
    assert err <= tol, f"nll backward: {err:.3e}"
    assert not gn[rows][target[rows] < 0].any()
    _ledger(f"nll log_softmax backward {dtype}, checked rows", err, tol)
    s = torch.zeros(F, dtype=torch.float64, device=dev)
    for r in range(0, n, 1 << 20):
        s += stored(nll64(logp[r:r + (1 << 20)], target[r:r + (1 << 20)])).sum(0)
    _colsum_check(cn, s, f32, f"colsum nll {dtype}")
