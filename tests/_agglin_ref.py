"""The input layer of the fork's models restated in torch on the CPU, in the REFERENCE's association: per sample,
`adj @ (x_j @ W) + b` (reference pygcn/layers.py:33-38) and F.relu — what `functional.aggregate_linear` evaluates
as (adj @ x_j) @ W + b on the device.  Plain torch: nothing here calls a pygcn_amd kernel.

Also the graphs, operands and exactly summable fixtures that tests/test_agglin_cpu.py (no GPU) and
tests/test_agglin_gpu.py share, and the documented geometry of gcn_agg_linear_partial_rows (include/gcn_spmm.h)."""
import numpy as np
import torch

WIDTH = 32
FINS = (4, 8, 16, 32)


# ------------------------------------------------------------------------------------------------ the reference
def step(adj, x, w, b, g, dtype, batch=1, relu=False, mask=None):
    """(y, grad_W, grad_b) of sum(y * g) in `dtype`: x [n, batch * Fin] holds sample j in the columns
    [j * Fin, (j + 1) * Fin), y and g [n, batch * Fout] likewise; adj is a dense [n, n] tensor; b may be None
    (grad_b is then None).  `mask` (bool [n, batch * Fout], with relu): the ReLU and its derivative are this mask
    instead of torch's own `out > 0` — see flips_are_at_the_boundary."""
    fin, fout = w.shape
    adj, x, g = adj.to(dtype), x.to(dtype), g.to(dtype)
    wp = w.detach().clone().to(dtype).requires_grad_()
    bp = b.detach().clone().to(dtype).requires_grad_() if b is not None else None
    outs = []
    for j in range(batch):
        support = torch.mm(x[:, j * fin:(j + 1) * fin], wp)                  # layers.py:33
        out = torch.mm(adj, support)                                          # layers.py:34 (spmm)
        out = out + bp if bp is not None else out                             # layers.py:35-36
        if relu and mask is not None:
            out = out * mask[:, j * fout:(j + 1) * fout].to(dtype)
        outs.append(torch.relu(out) if relu and mask is None else out)
    y = torch.cat(outs, dim=1)
    y.backward(g)
    return (y.detach().numpy(), wp.grad.numpy(), bp.grad.numpy() if bp is not None else None)


def flips_are_at_the_boundary(mask, pre64, tol=1e-5):
    """A pre-activation within rounding of zero can sit on the other side of the ReLU on the device: invisible in
    the forward pass, but it switches one term of a weight / bias gradient on or off.  The derivative of ReLU at 0
    is a convention, not arithmetic — as tests/test_norm_gpu.py check_relu_masks does, the comparison is made
    well-posed by handing the reference the device's mask AFTER asserting that it differs from float64's own only
    where the float64 pre-activation is within `tol` of zero, and on fewer than 1e-4 of the elements."""
    flips = np.asarray(mask) != (pre64 > 0)
    if flips.any():
        assert float(np.abs(pre64[flips]).max()) <= tol * float(np.abs(pre64).max()), "masks differ away from 0"
    assert float(flips.mean()) < 1e-4
    return int(flips.sum())


# ------------------------------------------------------------------------------------------------ graphs
def random_csr(n, seed, exact=False):
    """(rowptr int32 [n + 1], col int32, val float32) of a random n x n CSR matrix with about 5 entries per row,
    sorted unique columns; for n >= 3, row 1 is EMPTY and row 0 is a HUB holding every column.  `exact`: values
    are signed powers of two in [2^-1, 2^1], otherwise uniform in (-1, 1)."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n):
        if n >= 3 and r == 1:
            cols = np.zeros(0, np.int64)
        elif n >= 3 and r == 0:
            cols = np.arange(n)
        else:
            cols = np.unique(rng.integers(0, n, size=min(n, int(rng.integers(1, 9)))))
        rows.append(cols)
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    col = np.concatenate(rows).astype(np.int32)
    if exact:
        val = (rng.choice([-1.0, 1.0], col.size) * 2.0 ** rng.integers(-1, 2, col.size)).astype(np.float32)
    else:
        val = rng.uniform(-1, 1, col.size).astype(np.float32)
    return torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(val)


def dense_of(rowptr, col, val, n):
    adj = torch.zeros(n, n, dtype=torch.float32)
    counts = (rowptr[1:] - rowptr[:-1]).long()
    adj[torch.repeat_interleave(torch.arange(n), counts), col.long()] = val
    return adj


# ------------------------------------------------------------------------------------------------ operands
def seeded(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def operands(n, k, fin, seed, bias=True):
    """x [n, k * fin], W [fin, 32], b [32] or None, and a cotangent g [n, k * 32]."""
    return (seeded((n, k * fin), seed), seeded((fin, WIDTH), seed + 1) / 2,
            seeded((WIDTH,), seed + 2) / 2 if bias else None, seeded((n, k * WIDTH), seed + 3))


def exact_operands(n, k, fin, seed):
    """Operands on which every partial sum of the layer and of its two gradients, in EITHER association and in
    any order, is exactly representable in float32, for n <= 1100, k <= 3, fin <= 32: x and the cotangent g are
    integers in [-2, 2], g non-zero in at most 16 rows, b integers in [-4, 4], W and the adjacency values
    (random_csr(exact=True)) signed powers of two in [2^-1, 2^1].  Every quantity is a multiple of 2^-2, so a
    sum is exact while it stays below 2^24 * 2^-2 = 2^22:
      x_j @ W            <= 2 * 2 * 32 = 2^7;      adj @ (.) over a hub row of n entries <= 2 * 2^7 * 1100 < 2^19
      z = adj @ x        <= 2 * 2 * 1100 < 2^13;   z @ W <= 2^13 * 2 * 32 = 2^19;   + b: < 2^19 + 4
      adj^T @ g_j        <= 16 rows * 2 * 2 = 2^6;  x_j^T @ (.) over n rows <= 2 * 2^6 * 1100 < 2^18, times k < 2^20
      sum_u z * gp       <= 2^13 * 2 = 2^14 per term, 16 * k = 48 terms: < 2^20;    grad_b <= 48 * 2
    (the bounds hold for the ReLU-masked cotangent too: masking only removes terms)."""
    assert n <= 1100 and k <= 3 and fin <= 32
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(-2, 3, (n, k * fin)).astype(np.float32))
    w = torch.from_numpy((rng.choice([-1.0, 1.0], (fin, WIDTH)) * 2.0 ** rng.integers(-1, 2, (fin, WIDTH)))
                         .astype(np.float32))
    b = torch.from_numpy(rng.integers(-4, 5, WIDTH).astype(np.float32))
    g = torch.from_numpy(rng.integers(-2, 3, (n, k * WIDTH)).astype(np.float32))
    if n > 16:
        keep = torch.zeros(n, dtype=torch.float32)
        keep[torch.from_numpy(rng.choice(n, 16, replace=False))] = 1.0
        g = g * keep[:, None]
    return x, w, b, g


# ------------------------------------------------------------------------------------------------ geometry
def partial_rows_formula(n, batch):
    """gcn_agg_linear_partial_rows as include/gcn_spmm.h documents it: M = n * batch, P = ceil(M / (64 * 2048)),
    R = 64 * P, B = ceil(M / R).  Returns (B, R)."""
    m = n * batch
    p = -(-m // (64 * 2048))
    r = 64 * p
    return -(-m // r), r


def n_three_blocks(query, fin, batch):
    """The smallest n whose backward sweep spans >= 3 blocks with a ragged last one, from the library's answer
    `query(n, fin, 32, batch)` held against the documented formula."""
    for n in range(1, 1 << 20):
        blocks, per_block = partial_rows_formula(n, batch)
        assert query(n, fin, WIDTH, batch) == blocks, "the row query left its documented formula"
        if blocks >= 3 and (n * batch) % per_block != 0:
            return n
    raise AssertionError("no multi-block shape below 2^20 rows")
