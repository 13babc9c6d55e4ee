"""Full-size (BASELINE config C4: 10^7 vertices / 10^8 sampled edges, F = 256) checks of the HIP
path through properties that do not need a full-size CPU product:

  * Â is row-normalized, so Â · 1 = 1;  Âᵀ · 1 = the column sums of Â (fp64 bincount);
  * linearity: Â·(αB1 + B2) = α·Â·B1 + Â·B2;
  * sampled rows — uniformly random ones plus the longest rows (which take the chunked long-row
    path) — recomputed by the CPU oracle from their own stored entries.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import assert_normwise, assert_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c4():
    assert torch.cuda.is_available()
    from pygcn_amd import CSRGraph
    from pygcn_amd.utils import rmat_graph
    dev = torch.device("cuda:0")
    n, e = 10_000_000, 100_000_000
    rowptr, col, val = rmat_graph(n, e, seed=42, perm_seed=43, device=dev)
    g = CSRGraph(rowptr, col, val, (n, n))
    yield g, n
    del g
    torch.cuda.empty_cache()


def test_row_and_column_sums(c4):
    from pygcn_amd import spmm_csr
    g, n = c4
    ones = torch.ones(n, 256, device=g.device)
    out = spmm_csr(g, ones)
    assert float((out - 1).abs().max()) <= 1e-5          # rows of D^-1(A+I) sum to 1
    del out
    colsum = torch.zeros(n, dtype=torch.float64, device=g.device).index_add_(
        0, g.col.long(), g.val.double())
    out_t = spmm_csr(g.t(), ones)
    err = (out_t[:, 0].double() - colsum).abs().max().item()
    assert err <= 1e-5 * colsum.max().item()
    assert torch.equal(out_t[:, 0], out_t[:, 255])       # every feature column sees the same sum


def test_linearity(c4):
    from pygcn_amd import spmm_csr
    g, n = c4
    gen = torch.Generator(device=g.device).manual_seed(7)
    b1 = torch.randn(n, 256, generator=gen, device=g.device)
    b2 = torch.randn(n, 256, generator=gen, device=g.device)
    lhs = spmm_csr(g, 0.75 * b1 + b2)
    rhs = spmm_csr(g, b1).mul_(0.75).add_(spmm_csr(g, b2))
    scale = float(rhs.abs().max())
    assert float((lhs - rhs).abs().max()) <= 1e-5 * scale


def test_sampled_rows_against_oracle(c4, oracle):
    from pygcn_amd import spmm_csr
    g, n = c4
    gen = torch.Generator(device=g.device).manual_seed(8)
    B = torch.randn(n, 256, generator=gen, device=g.device)
    out = spmm_csr(g, B)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
    top = torch.topk(deg, 40).indices                      # hubs: tens of chunks each
    rnd = torch.randint(0, n, (3000,), generator=gen, device=g.device)
    rows = torch.unique(torch.cat([top, rnd, torch.tensor([0, n - 1], device=g.device)]))
    assert int(deg[top].max()) > 20000
    # gather the sampled rows' entries and the B rows they reference; remap to a small problem
    starts, ends = g.rowptr[rows].long(), g.rowptr[rows + 1].long()
    lens = ends - starts
    idx = torch.repeat_interleave(starts - torch.cumsum(lens, 0) + lens, lens) + torch.arange(
        int(lens.sum()), device=g.device)
    cols, vals = g.col[idx].long(), g.val[idx]
    ucols, inv = torch.unique(cols, return_inverse=True)
    rp = torch.zeros(len(rows) + 1, dtype=torch.int64, device=g.device)
    torch.cumsum(lens, 0, out=rp[1:])
    ref = oracle.spmm_csr(rp.cpu().numpy(), inv.cpu().numpy().astype(np.int32),
                          vals.cpu().numpy(), B[ucols].cpu().numpy())
    assert_normwise(out[rows].cpu(), ref, 1e-5, "sampled rows incl. hubs")


def test_sampled_rows_of_the_transpose_product_against_oracle(c4, oracle):
    """Âᵀ·G with a random G at full size — the backward product of a dense-gradient epoch —
    against the oracle on >= 3 000 sampled rows of CSR(Âᵀ) incl. its 40 heaviest (the hub COLUMNS
    of Â: tens of thousands of entries each, the chunked long-row path)."""
    from pygcn_amd import spmm_csr
    from _sampling import heavy_and_random_rows, sampled_rows_reference
    g, n = c4
    gt = g.t()
    gen = torch.Generator(device=g.device).manual_seed(18)
    G = torch.randn(n, 256, generator=gen, device=g.device)
    out = spmm_csr(gt, G)
    rows, heaviest = heavy_and_random_rows(gt, 40, 3000, gen)
    assert heaviest > 20000
    # Rows of Âᵀ are not normalized: a hub column sums 10⁴–10⁵ terms to magnitudes ~10², and the
    # float32 CPU chain loses ~1e-5 there by itself.  Arbiter: float64 accumulation of the same
    # float32 products; the HIP result must be within the contract's 1e-5 of it, and within 1e-5 +
    # (the float32 oracle's own measured distance from float64) of the float32 oracle
    # (conftest.assert_parity).
    got = out[rows].cpu().numpy()
    ref64 = sampled_rows_reference(oracle, gt, G, rows, f64=True)
    ref32 = sampled_rows_reference(oracle, gt, G, rows)
    assert_parity(got, ref32, ref64, "C4 transpose product: sampled rows incl. the heaviest columns")


def test_transpose_block_equals_the_full_transpose_product(c4):
    """The [|R2|, |R|] block of Âᵀ the one-node backward pass multiplies (cut from the rows R of
    CSR(Â)) against the full cached CSR(Âᵀ) on an operand that is zero outside R: the same rows,
    and nothing outside R2."""
    from pygcn_amd import fused, spmm_csr
    g, n = c4
    dev = g.device
    rows = torch.arange(n * 140 // 2708, device=dev)                 # the bench's idx_train share
    rs = fused.row_sets(g, rows)
    assert rs.at_block.shape == (rs.n2, rs.n_u) and rs.n_u == rows.numel()
    gen = torch.Generator(device=dev).manual_seed(11)
    gp = torch.randn(rs.n_u, 256, generator=gen, device=dev)
    small = spmm_csr(rs.at_block, gp)
    operand = torch.zeros(n, 256, device=dev)
    operand[rows] = gp
    full = spmm_csr(g.t(), operand)
    del operand
    scale = float(full.abs().max())
    assert float((full.index_select(0, rs.rows2) - small).abs().max()) <= 1e-5 * scale
    outside = torch.ones(n, dtype=torch.bool, device=dev)
    outside[rs.rows2] = False
    assert float(full[outside].abs().max()) == 0.0                   # R2 is exactly where it can be non-zero


def test_training_step_routes_agree(c4):
    """One training step of the 2-layer model at C4 by two routes through the HIP kernels:
    `model(x, adj, rows=idx)` (one autograd node: transpose block, gather-fused weight gradients,
    masks in the GEMM stores) and upstream's unchanged lines `model(x, adj)[idx]` (one node per
    layer: dense gradient through autograd, row bitmaps found at run time, row-restricted
    launches).  Same forward kernels, different backward routes: loss, selected rows and all four
    parameter gradients must agree."""
    from pygcn_amd import GCN
    g, n = c4
    dev = g.device
    gen = torch.Generator(device=dev).manual_seed(44)
    x = torch.randn(n, 256, generator=gen, device=dev)
    labels = torch.randint(0, 256, (n,), generator=gen, device=dev)
    idx = torch.arange(n * 140 // 2708, device=dev)
    torch.manual_seed(42)
    model = GCN(256, 256, 256, dropout=0.0).to(dev)
    model.train()
    out_rows = model(x, g, rows=idx)
    loss = torch.nn.functional.nll_loss(out_rows, labels[idx])
    loss.backward()
    fused_grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    sel = out_rows.detach().clone()
    model.zero_grad(set_to_none=True)
    del out_rows, loss
    full = model(x, g)
    loss2 = torch.nn.functional.nll_loss(full[idx], labels[idx])
    loss2.backward()
    assert torch.equal(full.detach()[idx], sel)                      # (the same forward kernels)
    del full
    for k, p in model.named_parameters():
        a, b = fused_grads[k].double(), p.grad.double()
        assert torch.isfinite(a).all() and float(b.abs().max()) > 0
        err = float((a - b).abs().max())
        # (two float32 routes, each within the contract's 1e-5 of exact arithmetic)
        assert err <= 1e-5 * float(b.abs().max()), f"{k}: {err:.3e} vs {float(b.abs().max()):.3e}"


def _gcn2_node(t):
    """The model's one autograd node (pygcn_amd/fused.py: GCN2Function / GCN2RowsFunction) behind `t`."""
    fn = t.grad_fn
    while fn is not None and "GCN2" not in type(fn).__name__:
        fn = fn.next_functions[0][0]
    assert fn is not None, "no one-node model function in the graph"
    return fn


def _c4_device_step(g, x, labels, idx, sample, route, dropout, scheme):
    """One training step of GCN(256, 256, 256) at C4 by `route` under GEMM scheme `scheme`.  Returns
    the step's loss, its log-probabilities at `sample` (rows of idx for the rows route), the four
    gradients, the hidden
    activation h1 the device computed (saved by the model's node) and the dropout seeds drawn."""
    from pygcn_amd import GCN, spmm as S
    from pygcn_amd.functional import nll_loss
    dev = g.device
    torch.manual_seed(42)
    model = GCN(256, 256, 256, dropout=dropout).to(dev)
    model.train()
    seeds, draw = [], S.next_dropout_seed

    def recording(device=None):
        seeds.append(draw(device))
        return seeds[-1]
    S.next_dropout_seed = recording
    before = S.gemm_scheme()
    S.set_gemm_scheme(scheme)
    try:
        if route == "rows":
            out = model(x, g, rows=idx)
            loss = torch.nn.functional.nll_loss(out, labels[idx])
            logp = out.detach()[sample]
        else:
            full = model(x, g)
            out = full if route == "all-vertices" else full[idx]
            loss = nll_loss(full, labels) if route == "all-vertices" else \
                torch.nn.functional.nll_loss(out, labels[idx])
            logp = full.detach()[sample]
        h1 = _gcn2_node(out).saved_tensors[3]
        loss.backward()
    finally:
        S.next_dropout_seed = draw
        S.set_gemm_scheme(before)
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    params = {k: p.detach().clone() for k, p in model.named_parameters()}
    return float(loss), logp, grads, params, h1, seeds


def _rows_chunks(n, chunk=1 << 20):
    return ((s, min(s + chunk, n)) for s in range(0, n, chunk))


def test_c4_training_step_against_float64(c4, oracle):
    """One training step of the 2-layer model at full C4 (10⁷ x 256) by four routes — `model(x, g,
    rows=idx)`, upstream's `model(x, g)[idx]`, the dense loss over all vertices
    (pygcn_amd.functional.nll_loss), the rows route with dropout 1/2 and the rows route under the
    scaled two-part fp16 GEMM scheme ("h2") — against the same step in
    float64 (tests/_f64.py: no project kernel) from the same fp32 x, weights and biases, at the
    contract's 1e-5 normwise: log-probabilities on sampled rows (incl. rows past element 2³¹ and the
    last row), the loss, all four parameter gradients.

    The ReLU / dropout mask is the device's (h1 != 0): over 2.56·10⁹ hidden units some
    pre-activations lie within rounding of zero, where the ReLU derivative is a convention — after
    asserting that the device's h1 differs from the float64 ReLU only there, that at p = 1/2 its
    zeros are (pre > 0) ∧ oracle.dropout_keep(seed, …) on sampled rows, that half the units are kept,
    and that the kept values are 2·relu(pre)."""
    import _f64
    from conftest import _record
    g, n = c4
    dev = g.device
    gen = torch.Generator(device=dev).manual_seed(44)
    x = torch.randn(n, 256, generator=gen, device=dev)
    labels = torch.randint(0, 256, (n,), generator=gen, device=dev)
    idx = torch.arange(n * 140 // 2708, device=dev)
    sample = torch.unique(torch.cat([torch.arange(64, device=dev), torch.arange(8_388_544, 8_388_672, device=dev),
                                     torch.randint(0, n, (2000,), generator=gen, device=dev),
                                     torch.tensor([n - 1], device=dev)]))
    sample_idx = torch.unique(torch.cat([idx[:64], idx[-64:], idx[torch.randint(0, idx.numel(), (2000,),
                                                                                 generator=gen, device=dev)]]))
    routes = [("rows", 0.0, "bf16x3"), ("upstream-lines", 0.0, "bf16x3"), ("all-vertices", 0.0, "bf16x3"),
              ("rows", 0.5, "bf16x3"), ("rows", 0.0, "h2")]
    dev_res = {}
    h1_plain = h1_drop = h1_h2 = seed = None
    for route, p, scheme in routes:
        loss, logp, grads, params, h1, seeds = _c4_device_step(
            g, x, labels, idx, sample_idx if route == "rows" else sample, route, p, scheme)
        dev_res[(route, p, scheme)] = (loss, logp, grads, params)
        if scheme == "h2":                           # (other GEMMs: its own mask)
            h1_h2 = h1
        elif p == 0.0:
            if h1_plain is None:
                h1_plain = h1
            else:                                    # (the same forward kernels on every route)
                assert torch.equal(h1, h1_plain)
        else:
            assert len(seeds) == 1
            h1_drop, seed = h1, seeds[0]
        del h1
        torch.cuda.empty_cache()
    params = dev_res[("rows", 0.0, "bf16x3")][3]
    for r in dev_res.values():
        assert all(torch.equal(r[3][k], params[k]) for k in params)
    W1, b1, W2, b2 = (params[k] for k in ("gc1.weight", "gc1.bias", "gc2.weight", "gc2.bias"))
    failures = []

    def check(got, ref, what):
        got, ref = got.double(), ref.double()
        scale, err = float(ref.abs().max()), float((got - ref).abs().max())
        _record(what, err, scale, 1e-5)
        if not err <= 1e-5 * scale:
            failures.append(f"{what}: max|d| = {err:.3e} > 1e-5 * {scale:.3e}")

    rp, col, val = g.rowptr, g.col, g.val

    def forward64(h1_dev, p):
        """pre1 (float64) -> a1 = the device's mask applied to 1/(1-p)·pre1, in place; the mask; pre1
        at the sampled rows."""
        pre1 = _f64.spmm64(rp, col, val, _f64.mm64(x, W1))
        pre1 += b1.double()
        pre_sampled = pre1[sample]
        top = float(pre1.abs().max())
        mask = h1_dev != 0
        scale = 2.0 if p > 0 else 1.0
        n_pos = n_kept = 0
        worst = 0.0
        for s, e in _rows_chunks(n):
            pc, hc, mc = pre1[s:e], h1_dev[s:e], mask[s:e]
            pos = pc > 0
            flips = mc & ~pos if p > 0 else mc != pos
            if bool(flips.any()):                    # on the device's side of the ReLU only within rounding of 0
                assert float(pc[flips].abs().max()) <= 1e-5 * top, "mask differs away from the ReLU boundary"
            n_pos += int(pos.sum())
            n_kept += int(mc.sum())
            worst = max(worst, float((hc.double() - scale * pc).abs()[mc].max()) if bool(mc.any()) else 0.0)
            pc.mul_(mc.double() * scale)             # a1: the device's mask, float64 values
        assert worst <= 1e-5 * scale * top, f"h1 vs {scale:g}·relu(pre64): {worst:.3e}"
        _record(f"C4 h1 vs {scale:g}·relu(pre64) on kept units (p={p:g})", worst, scale * top, 1e-5)
        if p > 0:
            frac = n_kept / n_pos
            assert abs(frac - 0.5) <= 1e-3, f"kept fraction {frac:.5f}"
        else:
            assert n_kept >= n_pos * (1 - 1e-6)
        return pre1, mask, pre_sampled

    def check_dropout_rows(pre1_rows, h1_rows, rows):
        kp = torch.from_numpy(oracle.dropout_keep(seed, rows.cpu().numpy(), 256, 0.5)).to(dev)
        top = float(pre1_rows.abs().max())
        clear = pre1_rows.abs() > 1e-5 * top
        assert torch.equal((h1_rows != 0)[clear], ((pre1_rows > 0) & kp)[clear])

    def logits64(a1):
        pre2 = _f64.spmm64(rp, col, val, _f64.mm64(a1, W2))
        pre2 += b2.double()
        for s, e in _rows_chunks(n):
            pre2[s:e] -= torch.logsumexp(pre2[s:e], 1, keepdim=True)
        return pre2                                   # log-probabilities

    def backward64(holder, a1, mask, scale):
        G2 = holder.pop()
        gb2, _ = _f64.colsum64(G2)
        gs2 = _f64.spmm64_t(rp, col, val, G2, n)
        del G2
        gw2 = _f64.tn64(a1, gs2)
        gpre1 = _f64.mm64(gs2, W2.t())
        del gs2
        for s, e in _rows_chunks(n):
            gpre1[s:e].mul_(mask[s:e].double() * scale)
        gb1, _ = _f64.colsum64(gpre1)
        gs1 = _f64.spmm64_t(rp, col, val, gpre1, n)
        del gpre1
        gw1 = _f64.tn64(x, gs1)
        return {"gc1.weight": gw1, "gc1.bias": gb1, "gc2.weight": gw2, "gc2.bias": gb2}

    def grad_rows_loss(logp64):
        """d mean_{i in idx} -logp[i, label_i] / d pre2 (zero outside idx)."""
        G2 = torch.zeros_like(logp64)
        li = labels[idx]
        sub = -logp64[idx].exp()
        sub[torch.arange(idx.numel(), device=dev), li] += 1.0
        G2[idx] = sub.mul_(-1.0 / idx.numel())
        return G2

    def compare(route, p, loss64, logp64_sampled, grads64, scheme="bf16x3"):
        loss, logp, grads, _ = dev_res[(route, p, scheme)]
        name = f"C4 {route} p={p:g}" + (f" {scheme}" if scheme != "bf16x3" else "")
        _record(name + ": loss", abs(loss - loss64), abs(loss64), 1e-5)
        if not abs(loss - loss64) <= 1e-5 * abs(loss64):
            failures.append(f"{name}: loss {loss:.8g} vs {loss64:.8g}")
        check(logp, logp64_sampled, name + ": log-probabilities, sampled rows")
        for k in grads:
            check(grads[k], grads64[k], f"{name}: {k}.grad")

    # ---- dropout 0: the three routes share the forward pass
    torch.cuda.reset_peak_memory_stats()
    a1, mask, _ = forward64(h1_plain, 0.0)
    del h1_plain
    logp64 = logits64(a1)
    loss_idx = float(-logp64[idx, labels[idx]].mean())
    loss_all = float(-logp64.gather(1, labels.view(-1, 1)).mean())
    samp, samp_idx = logp64[sample], logp64[sample_idx]       # (idx = 0, 1, …: positions = row ids)
    holder = [grad_rows_loss(logp64)]
    g_idx = backward64(holder, a1, mask, 1.0)
    compare("rows", 0.0, loss_idx, samp_idx, g_idx)
    compare("upstream-lines", 0.0, loss_idx, samp, g_idx)
    # dense loss over all vertices: coef·(onehot − exp(logp)), built in place of logp
    G2 = logp64
    del logp64
    for s, e in _rows_chunks(n):
        blk = G2[s:e]
        blk.exp_().neg_()
        blk.scatter_add_(1, labels[s:e].view(-1, 1), torch.ones(e - s, 1, dtype=torch.float64, device=dev))
        blk.mul_(-1.0 / n)
    holder = [G2]
    del G2
    compare("all-vertices", 0.0, loss_all, samp, backward64(holder, a1, mask, 1.0))
    del a1, mask
    torch.cuda.empty_cache()

    # ---- dropout 1/2 (rows route): the device's keep decisions against the oracle's keep function
    a1, mask, pre_sampled = forward64(h1_drop, 0.5)
    check_dropout_rows(pre_sampled, h1_drop[sample], sample)
    del h1_drop
    torch.cuda.empty_cache()
    logp64 = logits64(a1)
    loss_idx = float(-logp64[idx, labels[idx]].mean())
    samp_idx = logp64[sample_idx]
    holder = [grad_rows_loss(logp64)]
    del logp64
    compare("rows", 0.5, loss_idx, samp_idx, backward64(holder, a1, mask, 2.0))
    del a1, mask
    torch.cuda.empty_cache()

    # ---- the rows route under the "h2" GEMM scheme, with its own ReLU mask
    a1, mask, _ = forward64(h1_h2, 0.0)
    del h1_h2
    logp64 = logits64(a1)
    loss_idx = float(-logp64[idx, labels[idx]].mean())
    samp_idx = logp64[sample_idx]
    holder = [grad_rows_loss(logp64)]
    del logp64
    compare("rows", 0.0, loss_idx, samp_idx, backward64(holder, a1, mask, 1.0), "h2")
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print(f"C4 float64 step: peak device memory {peak:.1f} GiB")
    assert not failures, "\n".join(failures)
