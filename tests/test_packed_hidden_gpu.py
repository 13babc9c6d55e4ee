"""Layer 2 of the training-mode forward pass as (Â·h1)·W2 over PACKED hidden rows (pygcn_amd/fused.py
set_packed_hidden): the pack kernel against the NumPy reference of the format (tests/_pack512_ref.py), the packed
SpMM against the dense launch on the same operand (bit for bit), the GEMM's log_softmax epilogue against float64,
and a training step on both routes."""
import numpy as np
import pytest
import torch

import _pack512_ref as ref512
from conftest import assert_normwise

pytestmark = pytest.mark.gpu

ROUTES = 1e-5          # route against route, as tests/test_fused_gpu.py
TOL = 1e-5             # the log_softmax gate of tests/test_spmm_gpu.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _sparse_rows(m, density, seed):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((m, 256)).astype(np.float32)
    if density < 1.0:
        h[rng.random((m, 256)) >= density] = 0.0
    return h


def _check_pack(h, dev):
    """Device slots of `h` against the reference: every word the format defines, the overflow marks, and the
    expansion back to `h` bit for bit (rows that overflowed: the stored part)."""
    from pygcn_amd.spmm import rows_pack512
    want, written, want_ovf = ref512.pack(h)
    packed = rows_pack512(torch.from_numpy(h).to(dev))
    got = packed.slots.cpu().numpy().view(np.uint32)
    assert got.shape == want.shape
    assert np.array_equal(got[written], want[written]), "a defined word differs"
    back, ovf = ref512.expand(np.where(written, got, 0))
    assert np.array_equal(ovf, want_ovf), "overflow marks"
    bits, hb = back.view(np.uint32), h.view(np.uint32)
    assert np.array_equal(bits[~ovf], hb[~ovf]), "expansion of a row that fits"
    ref_back, _ = ref512.expand(want)
    assert np.array_equal(bits[ovf], ref_back.view(np.uint32)[ovf]), "stored part of an overflowed row"
    return want_ovf


@pytest.mark.parametrize("density", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("m", [1, 15, 16, 17, 129, 257])
def test_pack_is_exact(dev, m, density):
    ovf = _check_pack(_sparse_rows(m, density, 1000 * m + int(100 * density)), dev)
    if density == 1.0:
        assert ovf.all()
    if density == 0.0:
        assert not ovf.any()


def test_pack_at_the_capacity_edge_and_special_values(dev):
    h, names = ref512.special_rows()
    ovf = _check_pack(h, dev)
    marked = {names[k] for k in ("quarter 1 one over", "quarter 2 all set", "all -0.0")}
    assert set(np.flatnonzero(ovf)) == marked
    # -0.0, NaN and the infinities are stored values: the slot gives the row back bit for bit
    _, written, _ = ref512.pack(h)
    from pygcn_amd.spmm import rows_pack512
    got = rows_pack512(torch.from_numpy(h).to(dev)).slots.cpu().numpy().view(np.uint32)
    back, _ = ref512.expand(np.where(written, got, 0))
    r = names["special values"]
    assert np.array_equal(back.view(np.uint32)[r], h.view(np.uint32)[r])
    assert np.signbit(back[r, 1]) and back[r, 1] == 0 and np.isnan(back[r, 17])
    assert back[r, 35] == np.inf and back[r, 255] == -np.inf


# ------------------------------------------------------------------ packed SpMM against the dense launch
def _edge_csr(n, seed, hot_col, long_len):
    """[n, n] CSR: row 0 empty, rows 1..4 with 1, 63, 64 and 65 entries, row 5 with `long_len`, the rest 0..12;
    every non-empty row references `hot_col`."""
    rng = np.random.default_rng(seed)
    deg = np.minimum(rng.poisson(4, n), 12) + 1
    deg[:6] = [0, 1, 63, 64, 65, long_len]
    deg[n // 2] = 0
    rows = []
    for d in deg:
        if d == 0:
            rows.append(np.zeros(0, np.int32))
            continue
        others = rng.permutation(np.setdiff1d(np.arange(n), [hot_col]))[: d - 1]
        rows.append(np.sort(np.concatenate([[hot_col], others])).astype(np.int32))
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    val = (1.0 - rng.random(col.size)).astype(np.float32)
    return rowptr, col, val


def _hidden(n, seed, overflow_rows=()):
    """relu + dropout-like rows (25 % non-zero); `overflow_rows` get a quarter with 40 non-zeros."""
    h = np.abs(_sparse_rows(n, 0.25, seed))
    rng = np.random.default_rng(seed + 1)
    for k, r in enumerate(overflow_rows):
        h[r, ref512.quarter_columns(k % 4)[rng.permutation(64)[:40]]] = rng.random(40).astype(np.float32) + 0.5
    return h


@pytest.mark.parametrize("n,is64,hot_overflows", [(300, False, True), (303, True, False), (301, False, False)])
def test_packed_spmm_is_the_dense_launch_bit_for_bit(dev, n, is64, hot_overflows):
    """The same products in the same order: torch.equal with spmm_csr on the dense rows — rows of 0, 1, 63, 64
    and 65 entries, one row above long_thresh (chunks + spmm_long_reduce_kernel), a column every row gathers,
    gathered rows whose slot overflowed (their values come from the dense row, in place: the order of the sum
    does not change, so they too are held to torch.equal), n with and without a multiple of 4, int64 rowptr."""
    from pygcn_amd import CSRGraph, spmm_csr
    from pygcn_amd.spmm import rows_pack512
    hot = 7
    rowptr, col, val = _edge_csr(n, n, hot, long_len=100)
    g = CSRGraph(torch.from_numpy(rowptr if is64 else rowptr.astype(np.int32)).to(dev), torch.from_numpy(col).to(dev),
                 torch.from_numpy(val).to(dev), (n, n), long_thresh=32)
    assert g.plan(torch.float32).n_long >= 4                     # rows 2..5 are chunked at long_thresh = 32
    over = ([hot] if hot_overflows else []) + [20, 150, n - 1]
    h = _hidden(n, n + 5, over)
    _, _, ovf = ref512.pack(h)
    assert set(np.flatnonzero(ovf)) >= set(over)
    gathered = np.zeros(n, bool)
    gathered[col] = True
    assert (gathered & ovf).any(), "no gathered overflow row"
    if hot_overflows:
        assert ovf[hot]                                           # every non-empty row gathers an overflowed slot
    H = torch.from_numpy(h).to(dev)
    dense = spmm_csr(g, H)
    packed = spmm_csr(g, packed=rows_pack512(H))
    assert torch.equal(dense, packed)
    assert torch.equal(packed[0], torch.zeros(256, device=dev))  # the empty row
    # the default schedule too (long_thresh 256: row 5 is an ordinary row of a 64-entry tile and a half)
    g2 = CSRGraph(g.rowptr, g.col, g.val, (n, n))
    assert torch.equal(spmm_csr(g2, H), spmm_csr(g2, packed=rows_pack512(H)))
    with pytest.raises(RuntimeError, match="plain product"):
        spmm_csr(g, packed=rows_pack512(H), relu=True)


def test_packed_spmm_passes_special_values_through(dev):
    """NaN / inf / -0.0 in a gathered row reach the same output elements as in the dense launch."""
    from pygcn_amd import CSRGraph, spmm_csr
    from pygcn_amd.spmm import rows_pack512
    n = 80
    rowptr, col, val = _edge_csr(n, 3, 7, long_len=20)
    g = CSRGraph(torch.from_numpy(rowptr.astype(np.int32)).to(dev), torch.from_numpy(col).to(dev),
                 torch.from_numpy(val).to(dev), (n, n))
    h = _hidden(n, 9)
    h[7, [0, 100]] = [np.inf, -0.0]
    h[11, 200] = np.nan
    H = torch.from_numpy(h).to(dev)
    a, b = spmm_csr(g, H), spmm_csr(g, packed=rows_pack512(H))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ the GEMM's log_softmax epilogue
@pytest.mark.parametrize("M", [1, 127, 128, 129, 300])
def test_gemm_log_softmax_epilogue_matches_fp64(dev, M):
    """log_softmax(X·W + b) from the GEMM's store against float64.  Gates: the per-row bound tests/test_gemm_gpu.py
    holds the three-part product to (2e-6 of the row's largest logit; bias add exact in that test) — logsumexp is
    1-Lipschitz in the max norm, so such an input error moves an output by at most twice that — plus 4e-6 absolute
    for the hardware exp2 / log2 (256 terms of relative error 2^-22, one log2 of a value <= 256, roundings of the
    subtraction), and the gates of tests/test_spmm_gpu.py's log_softmax test: normwise TOL and |logsumexp| < 1e-5.
    Rows: one dominant logit, all logits equal, and a NaN row that must stay NaN in that row only."""
    from pygcn_amd.gemm import gemm_xw256_log_softmax
    gen = torch.Generator(device=dev).manual_seed(M)
    X = torch.randn(M, 256, generator=gen, device=dev) * 0.3
    W = torch.randn(256, 256, generator=gen, device=dev)
    bias = torch.randn(256, generator=gen, device=dev)
    dominant, equal, nan_row = (0, None, None) if M == 1 else (0, 1, M - 1)
    X[dominant] = 40.0 * W[:, 5] / (W[:, 5] @ W[:, 5])            # logit 5 = 40 + b, the others O(1)
    if equal is not None:
        X[equal] = 0.0                                            # logits = bias: all equal in the call without bias
    Xn = X.clone()
    if nan_row is not None:
        Xn[nan_row, 3] = float("nan")
    for b in (bias, None):
        got = gemm_xw256_log_softmax(Xn, W, b)
        assert got is not None and got.shape == (M, 256)
        z = X.double() @ W.double() + (b.double() if b is not None else 0.0)
        want = torch.log_softmax(z, 1)
        keep = torch.ones(M, dtype=torch.bool, device=dev)
        if nan_row is not None:
            assert bool(torch.isnan(got[nan_row]).all()), "the NaN row"
            keep[nan_row] = False
        assert bool(torch.isfinite(got[keep]).all()), "NaN outside its row"
        err = (got.double() - want).abs().amax(1)
        bound = 2 * 2e-6 * z.abs().amax(1) + 4e-6
        worst = float((err / bound)[keep].max())
        print(f"M={M} bias={b is not None}: worst err / bound = {worst:.3f}")
        assert worst <= 1.0
        assert_normwise(got[keep].cpu(), want[keep].cpu().numpy(), TOL, "GEMM log_softmax")
        assert float(torch.logsumexp(got[keep].double(), 1).abs().max()) < 1e-5
        if b is None and equal is not None:
            assert float((got[equal] + np.log(256.0)).abs().max()) <= 4e-6
        assert float(got[dominant, 5]) > -1e-6 and int(got[dominant].argmax()) == 5
        again = gemm_xw256_log_softmax(Xn, W, b)                              # fixed order, no atomics: the same bits
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))


def test_gemm_log_softmax_declines_what_it_cannot_take(dev):
    from pygcn_amd import spmm as S
    from pygcn_amd.gemm import gemm_xw256_log_softmax
    X, W = torch.randn(8, 256, device=dev), torch.randn(256, 256, device=dev)
    assert gemm_xw256_log_softmax(X[:, :128], W[:128]) is None
    assert gemm_xw256_log_softmax(X, W, torch.randn(256, device=dev).double()) is None
    before = S.gemm_scheme()
    S.set_gemm_scheme("h2")
    try:
        assert gemm_xw256_log_softmax(X, W) is None
    finally:
        S.set_gemm_scheme(before)


# ------------------------------------------------------------------ a training step on both routes
def test_training_step_on_both_routes(dev, monkeypatch):
    """n = 2000, 256 -> 256 -> 256, dropout 1/2, the same seed: log-probabilities and all five gradients of the
    packed route inside the route-against-route gate of tests/test_fused_gpu.py, identical keep bits; eval mode
    and dropout 0 take the dense route."""
    from pygcn_amd import GCN, CSRGraph, fused
    from pygcn_amd.utils import rmat_graph
    n = 2000
    rowptr, col, val = rmat_graph(n, 20000, seed=31, device="cpu")
    g = CSRGraph(rowptr.to(dev), col.to(dev), val.to(dev), (n, n))
    gen = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.randn(n, 256, generator=gen, device=dev)
    idx = torch.randperm(n, generator=gen, device=dev)[:300]
    y = torch.randint(0, 256, (300,), generator=gen, device=dev)
    torch.manual_seed(4)
    model = GCN(256, 256, 256, dropout=0.5).to(dev)
    calls, bits = [], []
    inner, layer_gemm = fused._layer2_packed, fused._gemm.layer_gemm
    monkeypatch.setattr(fused, "_layer2_packed", lambda *a: (calls.append(1), inner(*a))[1])

    def spy(*a, **k):
        out = layer_gemm(*a, **k)
        if k.get("keep_bits_out") is not None:
            bits.append(k["keep_bits_out"])
        return out
    monkeypatch.setattr(fused._gemm, "layer_gemm", spy)

    before = fused.packed_hidden()

    def step(packed, train=True, p=0.5):
        fused.set_packed_hidden(packed)
        try:
            model.train(train)
            model.dropout = p
            model.zero_grad()
            x = x0.clone().requires_grad_(True)
            torch.manual_seed(11)
            out, full = model(x, g, rows=idx, keep_full=True)
            torch.nn.functional.nll_loss(out, y).backward()
            return [full.detach(), out.detach(), x.grad] + [q.grad.clone() for q in model.parameters()]
        finally:
            fused.set_packed_hidden(before)
            model.dropout = 0.5
    dense = step(False)
    assert not calls and len(bits) == 1
    packed = step(True)
    assert len(calls) == 1 and len(bits) == 2
    assert torch.equal(bits[0], bits[1]), "keep bits differ between the routes"
    names = ["log-probabilities", "selected rows", "grad_x", "gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias"]
    assert len(dense) == len(packed) == len(names)
    for a, b, what in zip(packed, dense, names):
        assert bool(torch.isfinite(a).all()), what
        assert_normwise(a.cpu(), b.cpu().numpy(), ROUTES, "packed vs dense route: " + what)
    step(True, train=False)
    step(True, p=0.0)
    assert len(calls) == 1, "eval mode / dropout 0 took the packed route"
