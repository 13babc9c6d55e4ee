"""The per-element judge of the sparse kernels, in plain torch on the CPU (no pygcn_amd kernel).

The normwise gate (conftest.assert_normwise) measures an error against the LARGEST element of the
whole result, which a hub row sets: an ordinary row may then be wrong by 1e-4 of itself and pass.
This judge holds every element to the forward error bound of its own sum instead:

    Y[r, f] = sum_e |val_e| * |B[col_e, f]| (+ |bias_f|)                     yardstick64
    E[r, f] = (n_terms[r] + 2 + extra) * 2^-24 * Y[r, f]
    fp32 storage:  |got - ref64| <= E
    bf16 storage:  |got - ref64| <= E + 2^-8 * (|ref64| + E)

Why the bound is rigorous.  An fp32 FMA summation of n terms in ANY order is a summation tree of
depth at most n, and its computed value differs from the exact one by at most gamma_n * sum|terms|,
gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms,
2nd ed., §4.2).  Chunk partials, lane-group shuffles and the 16 running sums of `long_row_sum`
are such trees; adding exact zeros (masked lanes, padded slots) does not round.  The `+ 2` pays for
the bias add and for gamma_n against n u (n <= 1100 here: n u / (1 - n u) < (n + 1) u); `extra = 1`
pays for one more multiplication (the dropout scale).  ReLU is 1-Lipschitz, so E holds after it.
bf16 operands convert to fp32 exactly; the only storage rounding is the final one, taken with unit
roundoff 2^-8 as everywhere in this suite.

Also here, because the CPU tests and the GPU tests must agree on them: the fixed small graph whose
row lengths sit on every edge of the kernels' paths (edge_graph) and the pure-Python restatement of
the host dispatch of gcn_spmm.hip (expected_variant)."""
import numpy as np
import torch

from _f64 import spmm64

U_F32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
KWAVE = 64

# row lengths with a name: the edges of the narrow kernel's three paths (kShort = 8), of the chunk
# length the graph is planned with (LONG_THRESH = 32) and of long_row_sum's 16-fold unroll
LONG_THRESH = 32
ITEM_COSTS = (0, 200)          # 0 = the C-ABI default (64): items of <= 64 entries; 200: items with ne > 64
N_ROWS, N_COLS = 320, 300


def _elems_per_lane(dtype):
    return 128 // torch.finfo(dtype).bits


def _next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def expected_variant(F, dtype, aligned=True):
    """(kernel, VEC, LPR or lanes, grid_y): the instantiation `spmm_typed` (gcn_spmm.hip) selects for
    a product of width F.  `aligned`: unit column stride, bases and row pitches of B and C multiples
    of 16 bytes.  Narrow kernel: third field = LPR (lanes per row segment, a power of two); wide
    kernel: third field = the number of 16-byte lanes a row needs (64 per grid.y block)."""
    v = _elems_per_lane(dtype)
    if aligned and F % v == 0:
        lanes = F // v
        if lanes > 32:
            return ("wide", v, lanes, (lanes + KWAVE - 1) // KWAVE)
        return ("narrow", v, _next_pow2(lanes), 1)
    lpr = min(KWAVE, _next_pow2(F))
    return ("narrow", 1, lpr, (F + lpr - 1) // lpr)


def variant_name(F, dtype, aligned=True):
    k, vec, w, gy = expected_variant(F, dtype, aligned)
    t = "fp32" if dtype == torch.float32 else "bf16"
    return f"{k}<{t},VEC={vec},{'LPR' if k == 'narrow' else 'lanes'}={w}> grid.y={gy}"


def row_lengths(rowptr):
    rowptr = torch.as_tensor(rowptr)
    return (rowptr[1:] - rowptr[:-1]).long()


def yardstick64(rowptr, col, val, B, bias=None):
    """Y[r, f] = sum_e |val_e| * |B[col_e, f]| (+ |bias_f|) in float64: the size of the summands of
    element (r, f), what its rounding error is proportional to."""
    Y = spmm64(torch.as_tensor(rowptr), torch.as_tensor(col), torch.as_tensor(val).abs(), torch.as_tensor(B).abs())
    if bias is not None:
        Y = Y + torch.as_tensor(bias).double().abs()
    return Y


def row_bound(ref64, Y, n_terms, storage, extra=0):
    """The allowed |got - ref64| per element (float64 [n, F])."""
    n = torch.as_tensor(n_terms).double().reshape(-1, 1)
    E = (n + 2 + extra) * U_F32 * Y
    if storage == torch.bfloat16:
        return E + U_BF16 * (ref64.abs() + E)
    if storage != torch.float32:
        raise ValueError(f"storage {storage}")
    return E


def worst_ratio(err, bound, mask=None):
    """max err / bound (an exact result on a zero bound counts 0, any error there inf)."""
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    if mask is not None:
        ratio = torch.where(mask, ratio, torch.zeros_like(ratio))
    return ratio


def assert_within(got, ref64, bound, n_terms, what="", variant="", mask=None):
    """Every (unmasked) element of `got` within `bound` of `ref64`; returns the worst err / bound."""
    got = torch.as_tensor(got).detach().cpu().double()
    ref64 = torch.as_tensor(ref64).double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    if got.numel() == 0:
        return 0.0
    if mask is not None:      # (masked-out elements may hold inf in both: keep inf - inf out of the ratio)
        got, ref64 = torch.where(mask, got, torch.zeros_like(got)), torch.where(mask, ref64, torch.zeros_like(ref64))
        bound = torch.where(mask, bound, torch.ones_like(bound))
    ratio = worst_ratio((got - ref64).abs(), bound, mask)
    worst = float(ratio.max())
    if not worst <= 1.0:
        flat = int(ratio.argmax())
        r, f = divmod(flat, got.shape[1]) if got.dim() == 2 else (flat, 0)
        n = int(torch.as_tensor(n_terms).reshape(-1)[r])
        bad = int((ratio > 1.0).sum())
        raise AssertionError(
            f"{what}: row {r} (length {n}), column {f}: got {float(got.reshape(-1)[flat])!r}, float64 "
            f"{float(ref64.reshape(-1)[flat])!r}, err / E = {worst:.3g}; {bad} element(s) outside their bound; "
            f"expected kernel {variant}")
    return worst


def assert_rows_within(got, ref64, Y, n_terms, storage, extra=0, what="", aligned=True, mask=None):
    """Every element of `got` [n, F] within its rounding bound of `ref64` (see the module docstring).
    `n_terms[r]`: stored entries of row r.  `aligned` only names the kernel variant in the message;
    `mask` (bool [n, F]) restricts the check (kept elements of a dropout, the finite part).
    Returns the worst err / bound."""
    ref64 = torch.as_tensor(ref64).double()
    F = ref64.shape[1]
    return assert_within(got, ref64, row_bound(ref64, torch.as_tensor(Y).double(), n_terms, storage, extra), n_terms,
                         what, variant_name(F, storage, aligned), mask)


def log_softmax_bound(ref64, Y, n_terms, storage, T):
    """Bound of a fused log_softmax over rows (`ref64`: the float64 log-probabilities; Y, n_terms: of
    the product under it): logsumexp is 1-Lipschitz in the max norm, so an input error of at most
    max_f E[r, f] moves every output by at most twice that; T pays for expf / logf."""
    E = row_bound(ref64, Y, n_terms, torch.float32)
    b = 2.0 * E.max(1, keepdim=True).values + T
    b = b.expand_as(ref64)
    if storage == torch.bfloat16:
        return b + U_BF16 * (ref64.abs() + b)
    return b


# ------------------------------------------------------------------ the fixed graph
def edge_graph(seed=2024):
    """One 320 x 300 CSR (int64 rowptr, int32 col, float32 val in (0, 1]) whose rows sit on the
    edges of the kernels' paths when planned with long_thresh = 32, plus `named`: {name: row}.
    Column 0 is referenced by no stored entry.  Rows (length):
      0: 33*32 + 5 (first row, long: two full unrolls of long_row_sum plus a tail); 1-2: empty;
      3: 1; 4: 8; 5: 9 (kShort edge); 6: 31; 7: 32; 8: 33 (chunk edge); 9: 63; 10: 64; 11: 65;
      12: empty; 13: 15*32; 14: empty; 15: 16*32; 16: 16*32 + 1 (15 / 16 / 17 chunks);
      17: 33 | 18-19: 32, 32 | 20: 33 | 21-22: 32, 31 | 23: 33 | 24-26: 32, 32, 1 | 27: 33
          (long rows close an item: under item_cost = 200 the items between them hold exactly
           64, 63 and 65 entries — the 64-entry tile edge of an item);
      28-98: ordinary rows of 0..12 entries; 99: 34 (long: the next item starts at row 100);
      100-169: 70 empty rows (an item with ne = 0, nr = 64);
      170-316: ordinary rows; 317-318: empty; 319: 40 (last row, long)."""
    rng = np.random.default_rng(seed)
    deg = np.minimum(rng.poisson(4, N_ROWS), 12)
    head = [33 * 32 + 5, 0, 0, 1, 8, 9, 31, 32, 33, 63, 64, 65, 0, 15 * 32, 0, 16 * 32, 16 * 32 + 1,
            33, 32, 32, 33, 32, 31, 33, 32, 32, 1, 33]
    deg[:len(head)] = head
    deg[99] = 34
    deg[100:170] = 0
    deg[317:319] = 0
    deg[319] = 40
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    nnz = int(rowptr[-1])
    col = rng.integers(1, N_COLS, size=nnz).astype(np.int32)          # column 0: never referenced
    val = (1.0 - rng.random(nnz)).astype(np.float32)
    named = {"first_long": 0, "len1": 3, "len8": 4, "len9": 5, "len31": 6, "len32": 7, "len33": 8, "len63": 9,
             "len64": 10, "len65": 11, "chunks15": 13, "chunks16": 15, "chunks17": 16, "last_long": 319}
    return {"rowptr": rowptr, "col": col, "val": val, "shape": (N_ROWS, N_COLS), "named": named}


def host_items(rowptr, item_cost, long_thresh):
    """Python restatement of the planner's rule (plan_walk in gcn_host.hip): the row-batch items
    [(ra, rb)] and the long rows of a row pointer.  For the tests' own claims about the graph."""
    item_cost = item_cost if item_cost > 0 else 64
    deg = np.diff(np.asarray(rowptr, np.int64))
    items, longs = [], []
    ra, cost = 0, 0
    for r, d in enumerate(deg):
        if d > long_thresh:
            if r > ra:
                items.append((ra, r))
            ra, cost = r + 1, 0
            longs.append(r)
            continue
        c = int(d) + 1
        if r > ra and (cost + c > item_cost or r - ra >= KWAVE):
            items.append((ra, r))
            ra, cost = r, 0
        cost += c
    if len(deg) > ra:
        items.append((ra, len(deg)))
    return items, longs
