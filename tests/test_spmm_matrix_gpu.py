"""Every instantiation of the sparse product and of SDDMM, element by element against float64.

`gcn_spmm_csr_ep` is a family of template instantiations (gcn_spmm.hip, `spmm_typed`): storage
type x 16-byte lanes / scalar elements x narrow kernel with LPR in {1 .. 64} / wide kernel with one
or more grid.y blocks x int32 / int64 row pointer x XEPI in {0, 1, 2} x (wide) the FLAGS variant.
One test id per (storage type, width); each loops over the row-pointer type and two schedules of
ONE small graph (tests/_rowcheck.edge_graph: row lengths on every edge of the kernels' paths) and
holds every element of every result to the rounding bound of its own sum (tests/_rowcheck.py) —
next to, not instead of, the normwise gates of tests/test_spmm_gpu.py.

With PYGCN_ROW_LEDGER=<file> the worst err / bound of every (storage type, width, variant) is
written there as JSON at the end of the module (profiles/row_parity_ledger.md)."""
import json
import os

import numpy as np
import pytest
import torch

import inputs as gin
from _f64 import spmm64, spmm64_t
from _rowcheck import (ITEM_COSTS, LONG_THRESH, N_COLS, N_ROWS, U_F32, assert_rows_within, assert_within, edge_graph,
                       expected_variant, log_softmax_bound, row_lengths, variant_name, yardstick64)
from conftest import assert_normwise, load_golden  # noqa: F401  (the suite's gate and fixtures stay importable here)

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
# (storage type, path) -> widths.  "vec": F a multiple of the 16-byte lane, aligned operands;
# "scalar": the VEC = 1 fallback.  bf16 scalar 2, 9 and 17 are there for LPR 2, 16 and 32, which no
# other bf16 width reaches (tests/test_rowcheck_cpu.py::test_the_width_lists_reach_every_variant).
WIDTHS = {
    (F32, "vec"): [4, 8, 12, 16, 20, 36, 68, 128, 132, 256, 260, 640],
    (F32, "scalar"): [1, 2, 3, 5, 9, 17, 33, 63, 65, 130],
    (BF16, "vec"): [8, 16, 24, 40, 72, 136, 256, 264, 512, 520, 640],
    (BF16, "scalar"): [1, 2, 3, 7, 9, 17, 33, 65, 100],
}
SLICED = [(F32, 64), (BF16, 64)]        # a column slice at offset 1 of a wider tensor: lane multiple, misaligned base
IDX_TYPES = (torch.int32, torch.int64)
SDDMM_WIDTHS = {F32: [1, 4, 7, 64, 256, 260], BF16: [8, 24, 128, 264]}

# CASES: (storage type, F, sliced)
CASES = [(dt, F, False) for (dt, _), ws in WIDTHS.items() for F in ws] + [(dt, F, True) for dt, F in SLICED]
SDDMM_CASES = [(dt, F, False) for dt, ws in SDDMM_WIDTHS.items() for F in ws] + [(F32, 64, True), (BF16, 64, True)]

# Allowance for expf / logf in the fused log_softmax (check 3).  MEASURED, not chosen
# (tests/test_rowcheck_cpu.py::test_log_softmax_allowance_covers_the_host re-measures it): torch's float32
# log_softmax on the CPU, applied to the float32-rounded float64 product + bias of every fusable
# case of CASES, is at worst 1.647e-5 (absolute) from the float64 log_softmax of the float64 product
# (the 1061-entry row: |log-probability| beyond 128, where rounding the input and the output to
# float32 costs up to 7.6e-6 each).  Written here rounded up to 1.65e-5.
# Times 4, because expf / logf on the GPU may differ from the host's by a few ulp.
LOG_SOFTMAX_HOST_ERR = 1.65e-5
LOG_SOFTMAX_T = 4 * LOG_SOFTMAX_HOST_ERR

SENTINEL = -7.5          # exact in bf16; fills the columns past F of the strided `out`
SEED = 0x1234567890ABCDEF
_ROW_LEDGER = {}


def _name(dt):
    return "fp32" if dt == F32 else "bf16"


def _id(case):
    dt, F, sliced = case
    return f"{_name(dt)}-{F}" + ("-slice" if sliced else "")


def _note(dt, F, sliced, ratio, kernel=None, log_softmax=None):
    """(worst ratio of the product checks, worst ratio of the fused log_softmax or None) per variant."""
    key = (_name(dt), F, kernel or variant_name(F, dt, not sliced))
    _ROW_LEDGER[key] = (float(ratio), log_softmax)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pygcn_amd import _native
    _native.lib()   # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _write_row_ledger():
    yield
    path = os.environ.get("PYGCN_ROW_LEDGER")
    if path and _ROW_LEDGER:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump([{"dtype": k[0], "F": k[1], "variant": k[2], "worst_err_over_bound": v[0],
                        "log_softmax_err_over_bound": v[1]} for k, v in sorted(_ROW_LEDGER.items())], f, indent=0)


@pytest.fixture(scope="module")
def graphs(dev):
    """The edge graph on the device: {(row-pointer type, item_cost): CSRGraph}, all planned with an
    EXPLICIT long_thresh = 32 (without it bf16 storage would silently chunk at 1024), plus the host
    arrays as torch tensors."""
    from pygcn_amd import CSRGraph
    eg = edge_graph()
    host = {k: torch.from_numpy(eg[k]) for k in ("rowptr", "col", "val")}
    gs = {}
    for idx in IDX_TYPES:
        for ic in ITEM_COSTS:
            gs[idx, ic] = CSRGraph(host["rowptr"].to(idx).to(dev), host["col"].to(dev), host["val"].to(dev),
                                   eg["shape"], item_cost=ic, long_thresh=LONG_THRESH)
    stats = gs[torch.int32, 0].schedule_stats(BF16)
    assert stats["long_thresh"] == LONG_THRESH and stats["n_long"] > 0
    return gs, host, eg


def _operand(x, dt, sliced, dev):
    """`x` (float32 numpy [m, F]) in storage type dt on the device; `sliced`: as the column slice
    [:, 1:1+F] of a wider tensor — unit column stride, base off the 16-byte grid."""
    t = torch.from_numpy(x).to(dt)
    if not sliced:
        return t.to(dev)
    wide = torch.zeros((t.shape[0], t.shape[1] + 8), dtype=dt, device=dev)
    wide[:, 1:1 + t.shape[1]] = t.to(dev)
    view = wide[:, 1:1 + t.shape[1]]
    assert view.stride(1) == 1 and view.data_ptr() % 16 != 0
    return view


def _strided_out(n, F, dt, dev):
    """(wide, out): out = wide[:, :F] with ldc > F, the row pitch still a multiple of 16 bytes where
    F is a lane multiple (the 16-byte path stays selectable); the columns past F hold SENTINEL."""
    pad = 128 // torch.finfo(dt).bits
    wide = torch.full((n, F + pad), SENTINEL, dtype=dt, device=dev)
    return wide, wide[:, :F]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_spmm_variant_rows_against_float64(oracle, dev, graphs, case):
    """Checks 1-8 of one (storage type, F) over int32 / int64 row pointers and both schedules.

    The bound of every comparison is tests/_rowcheck.py's: (n + 2 + extra) * 2^-24 * sum|a||b| per
    element, plus the 2^-8 storage rounding for bf16.  Check 3 (fused log_softmax) allows
    2 * max_f E[r, f] + T with T = LOG_SOFTMAX_T = 4 * 1.65e-5 = 6.6e-5: 1.65e-5 is the measured worst
    absolute error of torch's float32 CPU log_softmax on the same cases (see LOG_SOFTMAX_HOST_ERR)."""
    from pygcn_amd import spmm_csr
    from pygcn_amd.spmm import log_softmax_fusable, pack_row_flags, row_bitmap
    dt, F, sliced = case
    gs, host, eg = graphs
    rp, col, val = host["rowptr"], host["col"], host["val"]
    n, m = N_ROWS, N_COLS
    aligned = not sliced
    kernel = expected_variant(F, dt, aligned)[0]
    n_terms = row_lengths(rp)
    empty = n_terms == 0
    assert int(col.min()) >= 1                                   # column 0 is referenced by nobody
    named = eg["named"]

    # ---- operands and float64 references, once for the four (row pointer, schedule) combinations
    Bh = gin.dense((m, F), 1000 + F)
    bh = gin.dense((F,), 3000 + F)
    B = _operand(Bh, dt, sliced, dev)
    Bc = torch.from_numpy(Bh).to(dt)                              # the operand as stored, on the host
    bias = torch.from_numpy(bh).to(dev)
    b64 = torch.from_numpy(bh).double()
    ref = spmm64(rp, col, val, Bc)
    Y = yardstick64(rp, col, val, Bc)
    ref_b, Y_b = ref + b64, Y + b64.abs()
    lsm = log_softmax_fusable(F, dt)
    ref_lsm = torch.log_softmax(ref_b, 1)
    keep = {p: torch.from_numpy(oracle.dropout_keep(SEED, np.arange(n), F, p)) for p in (0.5, 0.3)}
    rng = np.random.default_rng(77 + F)
    # row-sparse operand (check 5): density 0.05 is below both kernels' thresholds (3/4 wide, 1/8 narrow)
    live = torch.from_numpy((rng.random(m) < 0.05).astype(np.float32))
    Bsh = Bh * live.numpy()[:, None]
    Bs = _operand(Bsh, dt, sliced, dev)
    Bsc = torch.from_numpy(Bsh).to(dt)
    ref_s, Y_s = spmm64(rp, col, val, Bsc), yardstick64(rp, col, val, Bsc)
    assert 0 < 8 * (int(live.sum()) + 1) < m
    # output-row selection (check 6): a random half, one long row wanted and one not
    want = torch.from_numpy(rng.random(n) < 0.5)
    want[named["first_long"]], want[named["chunks16"]] = True, False
    want[named["len9"]], want[named["len8"]] = True, False
    # one inf in a row of B that short and long rows reference (check 7)
    c_inf = int(col[int(rp[named["len9"]])])
    Bih = Bh.copy()
    Bih[c_inf, F // 2] = np.inf
    Bi = _operand(Bih, dt, sliced, dev)
    Bic = torch.from_numpy(Bih).to(dt)
    ref_i, Y_i = spmm64(rp, col, val, Bic), yardstick64(rp, col, val, Bic)
    fin = torch.isfinite(ref_i)
    assert not bool(fin.all()) and not bool(torch.isnan(ref_i).any())
    # NaN in row 0 of B (check 7): the operands with row 0 = 0 and row 0 = NaN, dense and row-sparse
    def with_row0(x, v):
        x = x.copy()
        x[0, :] = v
        return _operand(x, dt, sliced, dev)
    # the transpose (check 8)
    Gh = gin.dense((n, F), 2000 + F)
    G = _operand(Gh, dt, sliced, dev)
    Gc = torch.from_numpy(Gh).to(dt)
    ref_t = spmm64_t(rp, col, val, Gc, m)
    Y_t = spmm64_t(rp, col, val.abs(), Gc.abs(), m)
    n_terms_t = torch.bincount(col.long(), minlength=m)
    assert int(n_terms_t[0]) == 0

    worst, worst_lsm = 0.0, None

    def judge(got, ref64, Yk, what, extra=0, mask=None, terms=n_terms):
        nonlocal worst
        worst = max(worst, assert_rows_within(got.float().cpu(), ref64, Yk, terms, dt, extra=extra, what=what,
                                              aligned=aligned, mask=mask))

    for (idx, ic), g in gs.items():
        tag = f"{_id(case)} rowptr={str(idx)[6:]} item_cost={ic}"
        assert g.rowptr.dtype == idx

        # ---- 1. plain, + bias, + bias + ReLU into a column slice of a sentinel-filled tensor (ldc > F)
        plain = None
        for kw, r64, Yk, at_empty in (({}, ref, Y, torch.zeros(F)),
                                      ({"bias": bias}, ref_b, Y_b, torch.from_numpy(bh)),
                                      ({"bias": bias, "relu": True}, ref_b.clamp_min(0), Y_b,
                                       torch.from_numpy(bh).clamp_min(0))):
            wide, out = _strided_out(n, F, dt, dev)
            assert spmm_csr(g, B, out=out, **kw) is out
            assert torch.equal(wide[:, F:], torch.full_like(wide[:, F:], SENTINEL)), f"{tag} {list(kw)}: wrote past F"
            judge(out, r64, Yk, f"{tag} {list(kw)}")
            assert torch.equal(out[empty.to(dev)].cpu(), at_empty.to(dt).expand(int(empty.sum()), F)), \
                f"{tag} {list(kw)}: rows without entries"
            if not kw:
                plain = out.clone()

        # ---- 2. XEPI = 2: output-row flags and the launch's own max|stored value|
        flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        amax = torch.zeros(1, dtype=torch.float32, device=dev)
        out = spmm_csr(g, B, c_flags=flags, c_absmax=amax)
        assert torch.equal(out, plain), f"{tag}: c_flags / c_absmax changed the result"
        assert torch.equal(flags.bool(), (out != 0).any(1)), f"{tag}: c_flags"
        assert torch.equal(amax.cpu().view(torch.int32), out.float().abs().max().reshape(1).cpu().view(torch.int32)), \
            f"{tag}: c_absmax {amax.item()!r} vs {out.float().abs().max().item()!r}"

        # ---- 3. XEPI = 1: fused log_softmax, long rows included
        if lsm:
            out = spmm_csr(g, B, bias=bias, log_softmax=True)
            bound = log_softmax_bound(ref_lsm, Y_b, n_terms, dt, LOG_SOFTMAX_T)
            worst_lsm = max(worst_lsm or 0.0, assert_within(out.float().cpu(), ref_lsm, bound, n_terms,
                                                            f"{tag} log_softmax", variant_name(F, dt, aligned)))

        # ---- 4. ReLU + dropout: the mask is oracle.dropout_keep's, kept elements are scaled
        for p in (0.5, 0.3):
            out = spmm_csr(g, B, bias=bias, relu=True, dropout_p=p, seed=SEED).float().cpu()
            assert bool((out[~keep[p]] == 0).all()), f"{tag} p={p}: a dropped element is not zero"
            scale = float(oracle.dropout_scale(p))
            judge(out, ref_b.clamp_min(0) * scale, Y_b * scale, f"{tag} dropout p={p}", extra=1, mask=keep[p])

        # ---- 5. operand hint on a row-sparse operand: both kernels take their flag path
        hint = row_bitmap(Bs)
        unhinted = spmm_csr(g, Bs)
        out = spmm_csr(g, Bs, b_hint=hint)
        judge(unhinted, ref_s, Y_s, f"{tag} row-sparse operand")
        judge(out, ref_s, Y_s, f"{tag} row-sparse operand + hint")
        if kernel == "wide":
            assert torch.equal(out, unhinted), f"{tag}: the hint changed bits in the wide kernel"

        # ---- 6. output-row selection
        bits, _ = pack_row_flags(want.to(dev))
        out = torch.full((n, F), float("nan"), dtype=dt, device=dev)
        spmm_csr(g, B, out=out, c_select=bits)
        assert torch.equal(out[want.to(dev)], plain[want.to(dev)]), f"{tag}: c_select changed a wanted row"
        assert bool(out[~want.to(dev)].isnan().all()), f"{tag}: c_select wrote an unwanted row"

        # ---- 7. masked lanes: NaN in the unreferenced row 0 of B must not reach any result
        zero0, nan0 = spmm_csr(g, with_row0(Bh, 0.0)), spmm_csr(g, with_row0(Bh, np.nan))
        assert torch.equal(zero0, nan0), f"{tag}: B[0] = NaN reached {int((zero0 != nan0).sum())} element(s)"
        Bs0, Bsn = with_row0(Bsh, 0.0), with_row0(Bsh, np.nan)
        zero0, nan0 = spmm_csr(g, Bs0, b_hint=row_bitmap(Bs0)), spmm_csr(g, Bsn, b_hint=row_bitmap(Bsn))
        assert torch.equal(zero0, nan0), f"{tag}: B[0] = NaN reached {int((zero0 != nan0).sum())} element(s), hinted"
        out = spmm_csr(g, Bi).float().cpu()
        assert torch.equal(torch.isfinite(out), fin), f"{tag}: inf in B[{c_inf}] spread to the wrong elements"
        judge(out, ref_i, Y_i, f"{tag} finite part beside an inf", mask=fin)

        # ---- 8. the transpose product, against the ORIGINAL arrays with rows and columns swapped
        judge(spmm_csr(g.t(), G), ref_t, Y_t, f"{tag} transpose", terms=n_terms_t)

    assert worst <= 1.0 and (worst_lsm or 0.0) <= 1.0
    print(f"{_id(case)} {variant_name(F, dt, aligned)}: worst err / bound {worst:.3f}, log_softmax {worst_lsm}")
    _note(dt, F, sliced, worst, log_softmax=worst_lsm)


@pytest.mark.parametrize("case", SDDMM_CASES, ids=_id)
def test_sddmm_entries_against_float64(dev, graphs, case):
    """gcn_sddmm_csr: every stored entry of every item and every long-row chunk against the float64
    dot product, within (F + 1) * 2^-24 * sum_f |G||B| (F FMAs and a six-level shuffle tree that adds
    zeros where F is small: a summation tree of depth <= F + 1; the output is fp32 for both types)."""
    from pygcn_amd.spmm import sddmm_csr
    dt, F, sliced = case
    gs, host, eg = graphs
    rp, col = host["rowptr"], host["col"]
    lens = row_lengths(rp)
    assert bool(((lens % 4) != 0).any()) and bool(((lens > LONG_THRESH) & (lens % 4 != 0)).any())   # the U = 4 tails
    rows = torch.repeat_interleave(torch.arange(N_ROWS), lens)
    Gh, Bh = gin.dense((N_ROWS, F), 4000 + F), gin.dense((N_COLS, F), 5000 + F)
    G, B = _operand(Gh, dt, sliced, dev), _operand(Bh, dt, sliced, dev)
    g64 = torch.from_numpy(Gh).to(dt).double()[rows]
    b64 = torch.from_numpy(Bh).to(dt).double()[col.long()]
    ref = (g64 * b64).sum(1, keepdim=True)
    bound = (F + 1) * U_F32 * (g64.abs() * b64.abs()).sum(1, keepdim=True)
    v = 128 // torch.finfo(dt).bits
    kernel = f"sddmm<{_name(dt)},VEC={v if (not sliced and F % v == 0) else 1}>"
    worst = 0.0
    for (idx, ic), g in gs.items():
        got = sddmm_csr(g, G, B)
        assert got.dtype == torch.float32 and got.shape == (g.nnz,)
        worst = max(worst, assert_within(got.cpu().reshape(-1, 1), ref, bound, lens[rows],
                                         f"sddmm {_id(case)} rowptr={str(idx)[6:]} item_cost={ic} (row = entry index)",
                                         kernel))
    print(f"sddmm {_id(case)} {kernel}: worst err / bound {worst:.3f}")
    _note(dt, F, sliced, worst, kernel)
