"""CPU tests of the per-element judge (tests/_rowcheck.py): a correct fp32 product passes it, an
error the normwise gate cannot see fails it, and the width lists of tests/test_spmm_matrix_gpu.py
reach every kernel instantiation the host dispatch of gcn_spmm.hip can select."""
import numpy as np
import pytest
import torch

import inputs as gin
from _f64 import spmm64
from _rowcheck import (ITEM_COSTS, LONG_THRESH, N_COLS, N_ROWS, assert_rows_within, edge_graph, expected_variant,
                       host_items, log_softmax_bound, row_lengths, yardstick64)
from conftest import assert_normwise

F32, BF16 = torch.float32, torch.bfloat16

# the parameter lists of tests/test_spmm_matrix_gpu.py, restated (and compared with the module's own below)
WIDTHS = {
    (F32, "vec"): [4, 8, 12, 16, 20, 36, 68, 128, 132, 256, 260, 640],
    (F32, "scalar"): [1, 2, 3, 5, 9, 17, 33, 63, 65, 130],
    (BF16, "vec"): [8, 16, 24, 40, 72, 136, 256, 264, 512, 520, 640],
    (BF16, "scalar"): [1, 2, 3, 7, 9, 17, 33, 65, 100],
}
SLICED = [(F32, 64), (BF16, 64)]
IDX_TYPES = (torch.int32, torch.int64)
CASES = [(dt, F, False) for (dt, _), ws in WIDTHS.items() for F in ws] + [(dt, F, True) for dt, F in SLICED]


def _cpu_product(rp, col, val, B32):
    """torch's own float32 sparse product on the CPU (duplicate columns of a row are summed)."""
    a = torch.sparse_csr_tensor(rp, col.long(), val, size=(rp.numel() - 1, B32.shape[0]))
    try:
        return a @ B32
    except RuntimeError:      # (a build without a CSR kernel for the CPU: the COO product)
        return torch.sparse.mm(a.to_sparse_coo(), B32)


@pytest.fixture(scope="module")
def eg():
    g = edge_graph()
    return {k: torch.from_numpy(g[k]) for k in ("rowptr", "col", "val")}, g


def _all_widths_graph():
    """The graph and operand of tests/test_spmm_gpu.py::test_spmm_matches_oracle_all_widths at F = 64."""
    F = 64
    rng = np.random.default_rng(F)
    deg = rng.poisson(6, size=3000)
    deg[rng.integers(0, 3000, size=300)] = 0
    for r, d in ((5, 255), (6, 256), (7, 257), (100, 5000), (2999, 1025), (0, 700)):
        deg[r] = d
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    nnz = int(rowptr[-1])
    col = rng.integers(0, 2500, size=nnz).astype(np.int32)
    val = (1.0 - rng.random(nnz)).astype(np.float32)
    return torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(val), torch.from_numpy(gin.dense((2500, F), 1000 + F))


def test_edge_graph_has_the_rows_the_kernels_branch_on(eg):
    host, g = eg
    lens = row_lengths(host["rowptr"]).numpy()
    assert g["shape"] == (N_ROWS, N_COLS) and lens.sum() < 6000
    for want in (0, 1, 8, 9, 31, 32, 33, 63, 64, 65, 15 * 32, 16 * 32, 16 * 32 + 1, 33 * 32 + 5):
        assert (lens == want).any(), want
    assert lens[0] > LONG_THRESH and lens[-1] > LONG_THRESH                 # first and last row long
    assert int(host["col"].min()) >= 1                                      # column 0 unreferenced
    long_rows = np.flatnonzero(lens > LONG_THRESH)
    assert any(lens[r - 1] == 0 and lens[r + 1] == 0 for r in long_rows if 0 < r < N_ROWS - 1)
    for ic in ITEM_COSTS:
        items, longs = host_items(host["rowptr"].numpy(), ic, LONG_THRESH)
        assert longs == list(long_rows)
        ne = [int(lens[a:b].sum()) for a, b in items]
        assert any(b - a == 64 and e == 0 for (a, b), e in zip(items, ne))  # 64 empty rows in one item
        covered = sorted(r for a, b in items for r in range(a, b)) + list(long_rows)
        assert sorted(covered) == list(range(N_ROWS))
        if ic == 200:      # items with several rows on the 64-entry tile edge, and beyond it
            multi = {e for (a, b), e in zip(items, ne) if b - a > 1}
            assert {63, 64, 65} <= multi and max(multi) > 64
        else:
            assert max(e for (a, b), e in zip(items, ne) if b - a > 1) <= 64


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{'fp32' if c[0] == F32 else 'bf16'}-{c[1]}{'-slice' if c[2] else ''}")
def test_reference_product_passes_the_row_judge(eg, case):
    """torch's fp32 CPU product on the GPU tests' graph and operands is inside the bound — fp32 as
    it is, and rounded to bf16 for bf16 storage (operands rounded to bf16 first, as stored)."""
    dt, F, _ = case
    host, _ = eg
    rp, col, val = host["rowptr"], host["col"], host["val"]
    B = torch.from_numpy(gin.dense((N_COLS, F), 1000 + F)).to(dt)
    got = _cpu_product(rp, col, val, B.float()).to(dt)
    ratio = assert_rows_within(got.float(), spmm64(rp, col, val, B), yardstick64(rp, col, val, B), row_lengths(rp), dt,
                               what=f"torch CPU product F={F}")
    assert ratio <= 1.0


def test_reference_product_passes_on_the_all_widths_graph():
    rp, col, val, B = _all_widths_graph()
    ratio = assert_rows_within(_cpu_product(rp, col, val, B), spmm64(rp, col, val, B), yardstick64(rp, col, val, B),
                               row_lengths(rp), F32, what="all-widths graph F=64")
    assert ratio <= 1.0


def _ordinary_row(lens, lo=1, hi=12, skip=0):
    rows = [r for r in range(len(lens)) if lo <= lens[r] <= hi]
    return rows[skip]


@pytest.mark.parametrize("which", ["edge graph", "all-widths graph"])
def test_relative_error_1e5_in_an_ordinary_row_passes_normwise_and_fails_the_judge(eg, which):
    """The planted error: one element of an ordinary row (1 to 12 entries) times (1 + 1e-5)."""
    if which == "edge graph":
        host, _ = eg
        rp, col, val = host["rowptr"], host["col"], host["val"]
        B = torch.from_numpy(gin.dense((N_COLS, 64), 1064))
    else:
        rp, col, val, B = _all_widths_graph()
    lens = row_lengths(rp)
    ref, Y = spmm64(rp, col, val, B), yardstick64(rp, col, val, B)
    good = _cpu_product(rp, col, val, B)
    r = _ordinary_row(lens.tolist(), skip=5)
    f = int(ref[r].abs().argmax())
    bad = good.clone()
    bad[r, f] *= 1.0 + 1e-5
    assert bad[r, f] != good[r, f]
    assert_normwise(bad.numpy(), ref.numpy(), 1e-5, "planted 1e-5 relative error")       # the old gate: blind
    assert_rows_within(good, ref, Y, lens, F32, what="unplanted")
    with pytest.raises(AssertionError, match=rf"row {r} \(length {int(lens[r])}\), column {f}:.*narrow<fp32,VEC=4,LPR=16>"):
        assert_rows_within(bad, ref, Y, lens, F32, what="planted")


def test_dropping_the_last_entry_of_a_short_row_fails_the_judge(eg):
    host, _ = eg
    rp, col, val = host["rowptr"], host["col"], host["val"]
    B = torch.from_numpy(gin.dense((N_COLS, 64), 1064))
    lens = row_lengths(rp)
    ref, Y = spmm64(rp, col, val, B), yardstick64(rp, col, val, B)
    r = _ordinary_row(lens.tolist(), lo=3, hi=8, skip=2)
    val2 = val.clone()
    val2[int(rp[r + 1]) - 1] = 0.0                   # the row's last stored entry leaves the sum
    bad = _cpu_product(rp, col, val2, B)
    with pytest.raises(AssertionError, match=rf"row {r} \(length {int(lens[r])}\)"):
        assert_rows_within(bad, ref, Y, lens, F32, what="last entry dropped")
    # ... and for bf16 storage, where the bound is 2^-8 relative
    Bb = B.to(BF16)
    refb, Yb = spmm64(rp, col, val, Bb), yardstick64(rp, col, val, Bb)
    assert_rows_within(_cpu_product(rp, col, val, Bb.float()).to(BF16).float(), refb, Yb, lens, BF16, what="bf16 good")
    with pytest.raises(AssertionError, match=rf"row {r} "):
        assert_rows_within(_cpu_product(rp, col, val2, Bb.float()).to(BF16).float(), refb, Yb, lens, BF16,
                           what="bf16, last entry dropped")


def test_judge_rejects_nan_and_any_error_on_a_zero_bound():
    rp, col, val = torch.tensor([0, 1, 1]), torch.tensor([1], dtype=torch.int32), torch.tensor([0.5])
    B = torch.ones(2, 3)
    ref, Y, lens = spmm64(rp, col, val, B), yardstick64(rp, col, val, B), row_lengths(rp)
    assert assert_rows_within(ref.float(), ref, Y, lens, F32) == 0.0
    for r, v in ((0, float("nan")), (1, 1e-30)):
        bad = ref.float().clone()
        bad[r, 2] = v
        with pytest.raises(AssertionError, match=f"row {r} "):
            assert_rows_within(bad, ref, Y, lens, F32)


def test_the_width_lists_reach_every_variant():
    """The done list, from the dispatch rule alone: every narrow (T, VEC, LPR) the host code can
    select, for both row-pointer types, and the three fill classes of the wide kernel per type."""
    import test_spmm_matrix_gpu as gpu
    assert gpu.WIDTHS == WIDTHS and gpu.SLICED == SLICED and gpu.IDX_TYPES == IDX_TYPES and gpu.CASES == CASES
    selectable = set()
    for dt in (F32, BF16):
        for F in range(1, 4097):
            for aligned in (True, False):
                k, vec, w, gy = expected_variant(F, dt, aligned)
                if k == "narrow":
                    selectable.add((dt, vec, w))
    assert selectable == ({(F32, 4, l) for l in (1, 2, 4, 8, 16, 32)} | {(BF16, 8, l) for l in (1, 2, 4, 8, 16, 32)}
                          | {(dt, 1, l) for dt in (F32, BF16) for l in (1, 2, 4, 8, 16, 32, 64)})
    reached = {(dt,) + expected_variant(F, dt, not sliced) for dt, F, sliced in CASES}
    narrow = {(dt, vec, w, idx) for dt, k, vec, w, gy in reached if k == "narrow" for idx in IDX_TYPES}
    missing = {(dt, vec, lpr, idx) for dt, vec, lpr in selectable for idx in IDX_TYPES} - narrow
    assert not missing, sorted(map(str, missing))
    assert any(gy > 1 for dt, k, vec, w, gy in reached if k == "narrow")      # scalar rows wider than a wave
    for dt in (F32, BF16):
        wide = [(w, gy) for d, k, vec, w, gy in reached if k == "wide" and d == dt]
        assert any(w == 64 and gy == 1 for w, gy in wide), "exactly one full wave"
        assert any(w < 64 and gy == 1 for w, gy in wide), "one partly filled wave"
        assert any(gy > 1 and w % 64 == 1 for w, gy in wide), "a last grid.y block of a single lane"
        assert any(gy > 1 and w % 64 not in (0, 1) for w, gy in wide), "several blocks, the last partly filled"
    # a misaligned lane multiple takes the scalar kernel
    assert expected_variant(64, F32, False) == ("narrow", 1, 64, 1) and expected_variant(64, F32, True)[1] == 4


def test_log_softmax_allowance_covers_the_host(eg):
    """LOG_SOFTMAX_HOST_ERR of the GPU tests is the measured worst absolute error of torch's float32
    log_softmax (CPU) on the float32-rounded float64 product + bias of every fusable case, against
    the float64 log_softmax of the float64 product.  Re-measured here: the written figure covers it
    and is no more than twice it (vector units of another host may round a few elements differently)."""
    import test_spmm_matrix_gpu as gpu
    host, _ = eg
    rp, col, val = host["rowptr"], host["col"], host["val"]
    worst = 0.0
    for dt, F, _ in CASES:
        v = 128 // torch.finfo(dt).bits
        if not (F <= 64 or (F % v == 0 and F // v <= 64)):          # pygcn_amd.spmm.log_softmax_fusable
            continue
        B = torch.from_numpy(gin.dense((N_COLS, F), 1000 + F)).to(dt)
        z = spmm64(rp, col, val, B) + torch.from_numpy(gin.dense((F,), 3000 + F)).double()
        err = (torch.log_softmax(z.float(), 1).double() - torch.log_softmax(z, 1)).abs().max()
        worst = max(worst, float(err))
    print(f"host float32 log_softmax: worst absolute error {worst:.3e}")
    assert worst <= gpu.LOG_SOFTMAX_HOST_ERR <= 2.0 * worst
    assert gpu.LOG_SOFTMAX_T == 4 * gpu.LOG_SOFTMAX_HOST_ERR
    # the bound built from it is finite and positive where the row has a bias
    F = 16
    B = torch.from_numpy(gin.dense((N_COLS, F), 1000 + F))
    b = torch.from_numpy(gin.dense((F,), 3000 + F)).double()
    bound = log_softmax_bound(torch.log_softmax(spmm64(rp, col, val, B) + b, 1), yardstick64(rp, col, val, B, b), row_lengths(rp), F32,
                              gpu.LOG_SOFTMAX_T)
    assert bool((bound >= gpu.LOG_SOFTMAX_T).all()) and bool(torch.isfinite(bound).all())
